"""One measured run of convert(quantize=True) -> profiles/convert_quantize.txt.

    python scripts/convert_quantize_bench.py [--out FILE] [--tmp DIR]

1. A whole conversion at Qwen2-VL-2B dimensions (language model 28 x 1536 / 8960, vocabulary 151936, tied head; ViT 32 x 1280):
   a seeded random bf16 checkpoint in the HF layout is written to a scratch directory, then `convert(src, dst, quantize=True)`
   is timed with a host clock (it ends in device-to-host copies and file writes).
2. The quantizer kernel alone on the embedding-sized matrix (151936 x 1536): device events around `ops.quantize_w4`, after a
   warm-up; bytes = the bf16 source read + the Wq and Wsb words written, computed from the shape.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

TEXT = dict(hidden_size=1536, num_hidden_layers=28, intermediate_size=8960, num_attention_heads=12, num_key_value_heads=2,
            vocab_size=151936)
VISION = dict(depth=32, embed_dim=1280, hidden_size=1536, num_heads=16, patch_size=14, mlp_ratio=4, in_channels=3,
              spatial_merge_size=2, temporal_patch_size=2)


def write_source(path: str) -> int:
    from safetensors.torch import save_file

    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s, std=0.02: (torch.randn(*s, device="cuda", generator=g) * std).to(torch.bfloat16).cpu()
    t, v = TEXT, VISION
    H, D = t["hidden_size"], t["hidden_size"] // t["num_attention_heads"]
    W = {"model.embed_tokens.weight": rnd(t["vocab_size"], H), "model.norm.weight": rnd(H)}
    for i in range(t["num_hidden_layers"]):
        p = f"model.layers.{i}."
        for n, rows in (("q_proj", H), ("k_proj", t["num_key_value_heads"] * D), ("v_proj", t["num_key_value_heads"] * D)):
            W[p + f"self_attn.{n}.weight"], W[p + f"self_attn.{n}.bias"] = rnd(rows, H), rnd(rows)
        W[p + "self_attn.o_proj.weight"] = rnd(H, H)
        W[p + "mlp.gate_proj.weight"], W[p + "mlp.up_proj.weight"] = rnd(t["intermediate_size"], H), rnd(t["intermediate_size"], H)
        W[p + "mlp.down_proj.weight"] = rnd(H, t["intermediate_size"])
        W[p + "input_layernorm.weight"], W[p + "post_attention_layernorm.weight"] = rnd(H), rnd(H)
    E, M = v["embed_dim"], v["embed_dim"] * v["mlp_ratio"]
    W["visual.patch_embed.proj.weight"] = rnd(E, v["in_channels"], v["temporal_patch_size"], v["patch_size"], v["patch_size"])
    for i in range(v["depth"]):
        p = f"visual.blocks.{i}."
        for n, shape in (("norm1", (E,)), ("norm2", (E,)), ("attn.qkv", (3 * E, E)), ("attn.proj", (E, E)), ("mlp.fc1", (M, E)),
                         ("mlp.fc2", (E, M))):
            W[p + n + ".weight"], W[p + n + ".bias"] = rnd(*shape), rnd(shape[0])
    W["visual.merger.ln_q.weight"], W["visual.merger.ln_q.bias"] = rnd(E), rnd(E)
    W["visual.merger.mlp.0.weight"], W["visual.merger.mlp.0.bias"] = rnd(4 * E, 4 * E), rnd(4 * E)
    W["visual.merger.mlp.2.weight"], W["visual.merger.mlp.2.bias"] = rnd(v["hidden_size"], 4 * E), rnd(v["hidden_size"])
    os.makedirs(path, exist_ok=True)
    save_file(W, os.path.join(path, "model.safetensors"))
    conf = dict(model_type="qwen2_vl", torch_dtype="bfloat16", rms_norm_eps=1e-6, rope_theta=1000000.0, tie_word_embeddings=True,
                rope_scaling={"type": "mrope", "mrope_section": [16, 24, 24]}, image_token_id=151655, video_token_id=151656,
                vision_start_token_id=151652, vision_config=dict(model_type="qwen2_vl", **VISION), **TEXT)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(conf, f)
    return sum(x.nbytes for x in W.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convert_quantize.txt"))
    ap.add_argument("--tmp", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    from mlx_vlm_amd import convert, ops

    lines = [f"convert(quantize=True) and the 4-bit quantizer kernel, one run as measured ({torch.cuda.get_device_name(0)})", ""]
    tmp = tempfile.mkdtemp(prefix="convert_bench_", dir=a.tmp)
    try:
        src, dst = os.path.join(tmp, "hf"), os.path.join(tmp, "mlx_q4")
        src_bytes = write_source(src)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        convert(src, dst, quantize=True)
        wall = time.perf_counter() - t0
        with open(os.path.join(dst, "model.safetensors.index.json")) as f:
            n_q = sum(k.endswith(".scales") for k in json.load(f)["weight_map"])
        dst_bytes = sum(os.path.getsize(os.path.join(dst, f)) for f in os.listdir(dst) if f.endswith(".safetensors"))
        lines += ["whole conversion, Qwen2-VL-2B dimensions (random bf16 weights, HF layout -> MLX 4-bit, one process, host clock):",
                  f"  source tensors {src_bytes / 1e9:.3f} GB -> output shards {dst_bytes / 1e9:.3f} GB",
                  f"  wall time {wall:.2f} s (read + sanitize + {n_q} quantize calls with their copies + write)", ""]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

    N, K = TEXT["vocab_size"], TEXT["hidden_size"]
    w = (torch.randn(N, K, device="cuda") * 0.02).to(torch.bfloat16)
    for _ in range(3):
        ops.quantize_w4(w)
    torch.cuda.synchronize()
    reps = 50
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        ops.quantize_w4(w)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    nbytes = N * K * 2 + N * (K // 8) * 4 + N * (K // 64) * 4
    lines += [f"quantizer kernel on the embedding-sized matrix [{N} x {K}] bf16 (device events, {reps} calls after 3 warm-up calls):",
              f"  {us:.1f} us per call, {nbytes / 1e6:.1f} MB moved (source read + Wq + Wsb written) -> {nbytes / us / 1e6:.3f} TB/s achieved",
              "  (the same matrix every call: part of the 467 MB source can stay in the 256 MiB Infinity Cache between calls)"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
