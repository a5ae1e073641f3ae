"""InternVL3 / InternVL3.5 at real widths, seeded noise for weights: what the layer-scale epilogue costs and what the family runs at.

    python scripts/internvl_bench.py [--out profiles/internvl3.txt] [--repeats 9] [--steps 96] [--only gemm,tower,decode]

Protocol (every figure): device events around windows of back-to-back launches, every shape warmed first, the median over
`--repeats` windows and the spread (max - min) / median over the same windows; two variants of one measurement ALTERNATE window
by window in one process, so that whatever else the host and the card are doing falls on both.

  (a) the wo-shaped and the fc2-shaped GEMM of the InternViT-300M tower at 13 tiles (13 x 1025 rows, E = 1024, K = 1024 / 4096)
      with BIAS | RESIDUAL | LAYERSCALE against BIAS | RESIDUAL on the same operands (in place, as the encoder loop runs them),
      and the same pair at 1 tile; achieved FLOP/s from 2 M N K over the window time;
  (b) the whole tower (patch GEMM, 24 encoder layers, pixel-shuffle gather, mlp1) at 1 tile and at 13 tiles, eager calls;
  (c) decode tok/s at 1 and 16 rows on the captured step at the InternVL3-8B widths (Qwen2.5-7B: hidden 3584) and the
      InternVL3.5-8B widths (Qwen3-8B: hidden 4096), through this family's classes and - same weights' shapes, same seed -
      through the Qwen2-VL / Qwen3-VL classes the decoders were built for, alternating.
No target is set for any of them: nobody had measured this family before.  Needs a GPU: there is no fallback.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def alternate(variants, repeats):
    """variants: name -> callable.  One window of each, in turn, `repeats` times -> name -> list of seconds"""
    out = {n: [] for n in variants}
    for _ in range(repeats):
        for n, fn in variants.items():
            out[n].append(window(fn))
    return out


def med_spread(xs):
    m = statistics.median(xs)
    return m, (max(xs) - min(xs)) / m


# ------------------------------------------------------------------ (a) the epilogue
def gemm_pairs(repeats, window_s=0.04):
    from mlx_vlm_amd import ops

    lines = []
    g = torch.Generator(device="cuda").manual_seed(0)
    rn = lambda *s, sc=1.0: (torch.randn(*s, generator=g, device="cuda") * sc).to(torch.bfloat16)   # noqa: E731
    for tiles in (13, 1):
        for name, K in (("wo ", 1024), ("fc2", 4096)):
            M, N = tiles * 1025, 1024
            a, w, b, x = rn(M, K), rn(N, K, sc=K ** -0.5), rn(N, sc=0.1), rn(M, N)
            ls = (0.05 + 0.1 * torch.rand(N, generator=g, device="cuda")).to(torch.bfloat16)
            b2 = ops.bias_scale(b, ls)
            base = ops.EPI_BIAS | ops.EPI_RESIDUAL
            xs = {"base": x.clone(), "ls": x.clone()}           # in place, as the encoder loop: every call reads and writes the stream
            ops.gemm(a, w, bias=b, res=xs["base"], out=xs["base"], epilogue=base)
            torch.cuda.synchronize()
            calls = max(40, int(window_s / (window(lambda: [ops.gemm(a, w, bias=b, res=xs["base"], out=xs["base"], epilogue=base)
                                                            for _ in range(20)]) / 20)))      # windows of ~40 ms
            run = {"base": lambda: [ops.gemm(a, w, bias=b, res=xs["base"], out=xs["base"], epilogue=base) for _ in range(calls)],
                   "ls": lambda: [ops.gemm(a, w, bias=b2, res=xs["ls"], out=xs["ls"], epilogue=base | ops.EPI_LAYERSCALE) for _ in range(calls)]}
            for fn in run.values():
                fn()
            torch.cuda.synchronize()
            t = alternate(run, repeats)
            (mb, sb), (ml, sl) = med_spread(t["base"]), med_spread(t["ls"])
            tf = lambda s: 2.0 * M * N * K * calls / s / 1e12   # noqa: E731
            lines.append(f"{name} GEMM, {tiles:2d} tile(s) (M {M:5d}, N {N}, K {K}): BIAS|RESIDUAL {mb / calls * 1e6:8.2f} us ({tf(mb):6.1f} TFLOP/s, spread "
                         f"{100 * sb:.2f} %)   + LAYERSCALE {ml / calls * 1e6:8.2f} us ({tf(ml):6.1f} TFLOP/s, spread {100 * sl:.2f} %)   "
                         f"difference {100 * (ml - mb) / mb:+.2f} % of the baseline (windows of {calls} calls)")
    return lines


# ------------------------------------------------------------------ models
def seeded(config: dict, arch: str, seed=0, **kw):
    """a model of `arch` (a package under mlx_vlm_amd.models) on synthetic weights drawn on the device"""
    import importlib

    from mlx_vlm_amd import synthetic

    mod = importlib.import_module(f"mlx_vlm_amd.models.{arch}")
    cfg = mod.ModelConfig.from_dict(config)
    m = mod.Model(cfg, **kw)
    m.load_weights(synthetic.random_weights(cfg, seed=seed))
    return m


def tower_times(repeats):
    from mlx_vlm_amd import synthetic

    tiny_lm = dict(synthetic.INTERNVL3_2B, text_config=dict(synthetic.INTERNVL3_2B["text_config"], num_hidden_layers=1, vocab_size=1024))
    model = seeded(tiny_lm, "internvl_chat", kv_pool_tokens=1024, max_seqs=2)          # the tower does not depend on the decoder
    lines = []
    g = torch.Generator(device="cuda").manual_seed(1)
    for tiles, calls in ((1, 10), (13, 4)):
        pix = torch.rand(tiles, 3, 448, 448, generator=g, device="cuda") * 2 - 1
        run = {"tower": lambda: [model.vision_model(pix) for _ in range(calls)],
               "tower + connector": lambda: [model.encode_image(pix) for _ in range(calls)]}
        for fn in run.values():
            fn()
        torch.cuda.synchronize()
        t = alternate(run, repeats)
        for n, xs in t.items():
            m, s = med_spread(xs)
            lines.append(f"{n:18s} {tiles:2d} tile(s) of 448 x 448 ({tiles * 1025:5d} rows, 24 layers): {m / calls * 1e3:8.3f} ms per call  "
                         f"(spread {100 * s:.2f} %; windows of {calls} eager calls)")
    del model
    torch.cuda.empty_cache()
    return lines


def decode_state(lm, B, prompt=128, room=4096):
    rng = np.random.default_rng(B)
    caches = lm.make_cache_batch(B)
    ids = rng.integers(3, 150000, (B, prompt))
    emb = lm.embed_tokens(ids).reshape(B * prompt, -1)
    pos = np.broadcast_to(np.tile(np.arange(prompt), B)[None], (3, B * prompt))
    logits = lm.prefill(emb, pos, caches, [prompt] * B, "last", reserve_extra=room)
    tok0 = logits.float().argmax(-1).to(torch.int32)
    return lm.decode_begin(caches, tok0, np.zeros((B, 1), dtype=np.int64), max_new_tokens=room), caches


def decode_rates(lms, rows, steps, repeats):
    """lms: name -> language model.  Per row count: both models step over the same contexts, alternating window by window
    (a first untimed pass leaves every captured step of the timed pass in the engines' caches)"""
    from mlx_vlm_amd.sample_utils import make_sampler

    sargs = make_sampler().engine_args()
    lines = []
    for B in rows:
        for timed in (False, True):
            states = {n: decode_state(lm, B, room=(repeats + 2) * steps + 8) for n, lm in lms.items()}
            for n, lm in lms.items():
                lm.decode_run(states[n][0], steps, sargs)
            torch.cuda.synchronize()
            t = alternate({n: (lambda n=n: lms[n].decode_run(states[n][0], steps, sargs)) for n in lms}, repeats)
            for _, caches in states.values():
                for c in caches:
                    c[0]._seq.release()
        for n, secs in t.items():
            rate, spread = med_spread([B * steps / s for s in secs])
            lines.append(f"  {n:34s} {B:2d} row(s): {rate:9.1f} tok/s  (spread {100 * spread:.2f} %)")
    return lines


def decode_compare(steps, repeats):
    from mlx_vlm_amd import synthetic

    lines = []
    tower = dict(synthetic.INTERNVL3_2B["vision_config"], num_hidden_layers=1)                  # decode does not touch the tower
    for label, conf, qwen_arch in (("InternVL3-8B widths (Qwen2.5-7B decoder: 28 layers, hidden 3584, 28:4 heads, intermediate 18944)", synthetic.INTERNVL3_8B, "qwen2_vl"),
                                   ("InternVL3.5-8B widths (Qwen3-8B decoder: 36 layers, hidden 4096, 32:8 heads, intermediate 12288)", synthetic.INTERNVL3_5_8B, "qwen3_vl")):
        t = conf["text_config"]
        ours = seeded(dict(conf, vision_config=tower), "internvl_chat", kv_pool_tokens=32768, max_seqs=40)
        if qwen_arch == "qwen2_vl":
            qc = dict(synthetic.QWEN2_VL_7B, vocab_size=t["vocab_size"], vision_config=dict(synthetic.QWEN2_VL_7B["vision_config"], depth=1))
        else:
            qc = dict(model_type="qwen3_vl", image_token_id=151655, video_token_id=151656, vision_start_token_id=151652,
                      text_config=dict(t, model_type="qwen3_vl_text", max_position_embeddings=40960,
                                       rope_scaling={"rope_type": "default", "mrope_section": [24, 20, 20], "mrope_interleaved": True}),
                      vision_config=dict(model_type="qwen3_vl", depth=1, hidden_size=1024, intermediate_size=4096, out_hidden_size=t["hidden_size"],
                                         num_heads=16, patch_size=16, num_position_embeddings=2304, deepstack_visual_indexes=[]))
        theirs = qwen_model(qc, qwen_arch)
        lines.append(label + ":")
        lines += decode_rates({"models.internvl_chat": ours.language_model, f"models.{qwen_arch} (same decoder)": theirs.language_model}, (1, 16), steps, repeats)
        del ours, theirs
        torch.cuda.empty_cache()
    return lines


def qwen_model(conf, arch):
    """the Qwen-family model of the same decoder shapes; its synthetic weights come from the family's own shape table where there
    is one (qwen2_vl), else are drawn here (qwen3_vl: the language model's names only - the tower is not run)"""
    import importlib

    from mlx_vlm_amd import synthetic

    mod = importlib.import_module(f"mlx_vlm_amd.models.{arch}")
    cfg = mod.ModelConfig.from_dict(conf)
    m = mod.Model(cfg, kv_pool_tokens=32768, max_seqs=40)
    if arch == "qwen2_vl":
        m.load_weights(synthetic.random_weights(cfg, seed=0))
        return m
    from mlx_vlm_amd.models.internvl_chat import ModelConfig as IC

    ic = IC.from_dict(dict(synthetic.INTERNVL3_5_8B, text_config=dict(conf["text_config"], model_type="qwen3")))
    W = {k[len("language_model."):]: v for k, v in synthetic.random_weights(ic, seed=0).items() if k.startswith("language_model.")}
    m.language_model.load_weights(W)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "internvl3.txt"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--steps", type=int, default=96)
    ap.add_argument("--only", default="gemm,tower,decode")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("internvl_bench.py needs a GPU (there is no fallback)")
    only = set(a.only.split(","))
    lines = ["InternVL3 / InternVL3.5 at real widths, seeded noise for weights, MI355X.",
             f"median over {a.repeats} windows (device events), variants alternating window by window; spread = (max - min) / median.", ""]
    if "gemm" in only:
        lines += ["(a) layer-scale epilogue against its BIAS | RESIDUAL sibling, same operands, in place (windows of ~40 ms):"] + gemm_pairs(a.repeats) + [""]
    if "tower" in only:
        lines += ["(b) InternViT-300M tower (E 1024, 16 heads of 64, intermediate 4096, tanh GELU, layer scale):"] + tower_times(a.repeats) + [""]
    if "decode" in only:
        lines += [f"(c) decode on the captured step, greedy, 128-token prompts, windows of {a.steps} replays:"] + decode_compare(a.steps, a.repeats) + [""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
