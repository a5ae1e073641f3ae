"""Qwen3-VL at the 2B model's widths, seeded noise for weights: what the family's two-launch qkv step costs.

    python scripts/qwen3_vl_bench.py [--out profiles/qwen3_vl_decode.txt] [--repeats 7] [--steps 96]

Language model: 28 layers, hidden 2048, 16 : 8 heads of 128, intermediate 6144, vocabulary 151936, tied head.  Tower: depth 24,
hidden 1024, 16 heads of 64, intermediate 4096, DeepStack taps behind blocks 5 / 11 / 17, patch 16.

Reported (protocol: device events around windows of captured-step replays, the median over `--repeats` windows and the spread
(max - min) / median over the same windows; every shape warmed first; the profiler in a run of its own):
  * decode tok/s at 1 and at 16 rows on the captured step (greedy, 128-token prompts, `--steps` replays per window; with the
    defaults a sequence's context runs from 128 to 992 tokens, and a first untimed pass over the same contexts leaves every
    captured step of the timed pass in the engine's cache);
  * the time of the new launch - the QK-norm form of the rotary + KV-write kernel - from `rocprofv3 --kernel-trace --stats` over
    a fresh child process that replays the same steps (kernel time, per launch; the launches of one step are 28 of them);
  * the tower's time at one 448 x 448 image (grid 28 x 28: 784 patch rows), one eager call after the other.
No target is set for any of them: nobody had measured this family before.  Needs a GPU: there is no fallback.
"""
from __future__ import annotations

import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TEXT = dict(model_type="qwen3_vl_text", hidden_size=2048, num_hidden_layers=28, intermediate_size=6144, num_attention_heads=16,
            num_key_value_heads=8, head_dim=128, rms_norm_eps=1e-6, vocab_size=151936, rope_theta=5000000.0,
            max_position_embeddings=262144, tie_word_embeddings=True,
            rope_scaling={"rope_type": "default", "mrope_section": [24, 20, 20], "mrope_interleaved": True})
VISION = dict(model_type="qwen3_vl", depth=24, hidden_size=1024, intermediate_size=4096, out_hidden_size=2048, num_heads=16,
              patch_size=16, num_position_embeddings=2304, deepstack_visual_indexes=[5, 11, 17])
KERNEL = "mrope_qknorm_kvwrite_kernel"


def seeded_model(seed=0):
    """weights drawn on the device (2 G parameters: seconds there, minutes on the host)"""
    from mlx_vlm_amd.models.qwen3_vl import Model, ModelConfig

    g = torch.Generator(device="cuda").manual_seed(seed)
    bf = torch.bfloat16

    def rn(*shape, s=0.02):
        return (torch.randn(*shape, generator=g, device="cuda") * s).to(bf)

    def near1(n):
        return (1 + torch.randn(n, generator=g, device="cuda") * 0.05).to(bf)

    t, v = TEXT, VISION
    D, hd, E, I = t["hidden_size"], t["head_dim"], v["hidden_size"], v["intermediate_size"]
    M = 4 * E
    W = {"vision_tower.patch_embed.proj.weight": rn(E, 2, 16, 16, 3), "vision_tower.patch_embed.proj.bias": rn(E),
         "vision_tower.pos_embed.weight": rn(v["num_position_embeddings"], E)}
    for i in range(v["depth"]):
        p = f"vision_tower.blocks.{i}."
        for n in ("norm1", "norm2"):
            W[p + n + ".weight"], W[p + n + ".bias"] = near1(E), rn(E)
        W[p + "attn.qkv.weight"], W[p + "attn.qkv.bias"] = rn(3 * E, E), rn(3 * E)
        W[p + "attn.proj.weight"], W[p + "attn.proj.bias"] = rn(E, E), rn(E)
        W[p + "mlp.linear_fc1.weight"], W[p + "mlp.linear_fc1.bias"] = rn(I, E), rn(I)
        W[p + "mlp.linear_fc2.weight"], W[p + "mlp.linear_fc2.bias"] = rn(E, I), rn(E)
    for p, nd in [("vision_tower.merger.", E)] + [(f"vision_tower.deepstack_merger_list.{j}.", M) for j in range(3)]:
        W[p + "norm.weight"], W[p + "norm.bias"] = near1(nd), rn(nd)
        W[p + "linear_fc1.weight"], W[p + "linear_fc1.bias"] = rn(M, M), rn(M)
        W[p + "linear_fc2.weight"], W[p + "linear_fc2.bias"] = rn(v["out_hidden_size"], M), rn(v["out_hidden_size"])
    W["language_model.model.embed_tokens.weight"] = rn(t["vocab_size"], D)
    for i in range(t["num_hidden_layers"]):
        p = f"language_model.model.layers.{i}."
        W[p + "input_layernorm.weight"], W[p + "post_attention_layernorm.weight"] = near1(D), near1(D)
        W[p + "self_attn.q_proj.weight"] = rn(t["num_attention_heads"] * hd, D)
        W[p + "self_attn.k_proj.weight"], W[p + "self_attn.v_proj.weight"] = rn(t["num_key_value_heads"] * hd, D), rn(t["num_key_value_heads"] * hd, D)
        W[p + "self_attn.o_proj.weight"] = rn(D, t["num_attention_heads"] * hd)
        W[p + "self_attn.q_norm.weight"], W[p + "self_attn.k_norm.weight"] = near1(hd), near1(hd)
        W[p + "mlp.gate_proj.weight"], W[p + "mlp.up_proj.weight"] = rn(t["intermediate_size"], D), rn(t["intermediate_size"], D)
        W[p + "mlp.down_proj.weight"] = rn(D, t["intermediate_size"])
    W["language_model.model.norm.weight"] = near1(D)
    cfg = ModelConfig.from_dict(dict(model_type="qwen3_vl", text_config=dict(TEXT), vision_config=dict(VISION),
                                     image_token_id=151655, video_token_id=151656, vision_start_token_id=151652))
    m = Model(cfg, kv_pool_tokens=32768, max_seqs=40)
    m.load_weights(W)
    return m


def decode_state(lm, B, prompt=128, room=4096):
    """B sequences with `prompt` cached tokens each, bound to the captured decode step"""
    rng = np.random.default_rng(B)
    caches = lm.make_cache_batch(B)
    ids = rng.integers(3, 150000, (B, prompt))
    emb = lm.embed_tokens(ids).reshape(B * prompt, -1)
    pos = np.broadcast_to(np.tile(np.arange(prompt), B)[None], (3, B * prompt))
    logits = lm.prefill(emb, pos, caches, [prompt] * B, "last", reserve_extra=room)
    tok0 = logits.float().argmax(-1).to(torch.int32)
    st = lm.decode_begin(caches, tok0, np.zeros((B, 1), dtype=np.int64), max_new_tokens=room)
    return st, caches


def time_windows(fn, repeats):
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    return out


def med_spread(xs):
    m = statistics.median(xs)
    return m, (max(xs) - min(xs)) / m


def decode_rates(lm, rows, steps, repeats):
    from mlx_vlm_amd.sample_utils import make_sampler

    sargs = make_sampler().engine_args()
    res = {}
    for B in rows:
        # two passes over the SAME contexts on fresh sequences: a one-row greedy step is captured once per page count of its
        # context, so the first pass leaves every graph the second one replays in the engine's cache; only the second is timed
        for timed in (False, True):
            st, caches = decode_state(lm, B, room=(repeats + 2) * steps + 8)
            lm.decode_run(st, steps, sargs)
            torch.cuda.synchronize()
            secs = time_windows(lambda: lm.decode_run(st, steps, sargs), repeats)
            for c in caches:
                c[0]._seq.release()
        rates = [B * steps / s for s in secs]
        res[B] = med_spread(rates) + (lm_launches(lm),)
    return res


def lm_launches(lm):
    from mlx_vlm_amd import _lib

    return int(_lib.lib().vlm_llm_decode_launches(lm._handle))


def tower_time(model, repeats):
    g = torch.Generator().manual_seed(1)
    pix = torch.rand(28 * 28, 3 * 2 * 16 * 16, generator=g) * 2 - 1
    thw = np.array([[1, 28, 28]])
    pix = pix.cuda()
    for _ in range(3):
        model.vision_tower(pix, thw)
    torch.cuda.synchronize()
    return med_spread([s * 1e3 for s in time_windows(lambda: [model.vision_tower(pix, thw) for _ in range(10)], repeats)])


def trace_child(steps):
    """what the profiled child runs: the captured steps at 1 and 16 rows, nothing else timed"""
    from mlx_vlm_amd.sample_utils import make_sampler

    lm = seeded_model().language_model
    sargs = make_sampler().engine_args()
    for B in (1, 16):
        st, _ = decode_state(lm, B, room=2 * steps + 8)
        lm.decode_run(st, steps, sargs)
    torch.cuda.synchronize()


def kernel_stats(trace_dir):
    """-> rows of the profiler's kernel statistics whose name contains KERNEL"""
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            rows += [r for r in csv.DictReader(f) if KERNEL in (r.get("Name") or r.get("KernelName") or "")]
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qwen3_vl_decode.txt"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=96)
    ap.add_argument("--trace-dir", default=None, help="where rocprofv3 writes (default: a temporary directory)")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qwen3_vl_bench.py needs a GPU (there is no fallback)")
    if a.trace_child:
        return trace_child(a.steps)
    model = seeded_model()
    lines = ["Qwen3-VL at 2B widths (28 layers, hidden 2048, 16:8 heads of 128, intermediate 6144, vocabulary 151936, tied head;",
             "tower depth 24, hidden 1024, 16 heads, intermediate 4096, taps behind blocks 5 / 11 / 17), seeded noise, MI355X.",
             f"median over {a.repeats} windows of {a.steps} captured-step replays (device events), contexts 128 .. {128 + (a.repeats + 1) * a.steps} tokens; spread = (max - min) / median.", ""]
    for B, (rate, spread, launches) in decode_rates(model.language_model, (1, 16), a.steps, a.repeats).items():
        lines.append(f"decode, {B:2d} row(s): {rate:9.1f} tok/s  (spread {100 * spread:.2f} %; {rate / B:.1f} steps/s, {launches} launches per step)")
    ms, spread = tower_time(model, a.repeats)
    lines.append(f"tower, one 448 x 448 image (784 patch rows, 3 taps): {ms / 10:.3f} ms per call  (spread {100 * spread:.2f} %; windows of 10 eager calls)")
    del model
    torch.cuda.empty_cache()
    if not a.no_trace:
        if a.trace_dir is None:
            import tempfile

            a.trace_dir = tempfile.mkdtemp(prefix="qwen3_vl_trace_")
        os.makedirs(a.trace_dir, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.trace_dir, "--", sys.executable,
               os.path.abspath(__file__), "--trace-child", "--steps", str(a.steps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        rows = kernel_stats(a.trace_dir)
        lines.append("")
        lines.append(f"rocprofv3 --kernel-trace --stats over a child of its own ({a.steps} steps at 1 row, then at 16 rows; rc {r.returncode}):")
        if not rows:
            lines.append(f"  no row for {KERNEL} found under {a.trace_dir}")
            lines += ["  " + ln for ln in (r.stderr or "").strip().splitlines()[-5:]]
        for row in rows:
            lines.append("  " + ", ".join(f"{k}={v}" for k, v in row.items()))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
