"""Attention of ONE layer for a prompt chunk appended to a cache, bf16 against 8-bit, at the Qwen2-VL-2B (Hq 12, Hkv 2) and
7B (28, 4) head counts:

  (a) the bf16 onto-cache path of LanguageModel._prefill_onto_cache: vlm_kv_gather of [prefix | chunk] into a token-major
      buffer + vlm_attn_prefill with q_start - or, for a chunk of up to 64 rows, the decode-row route it takes instead
      (vlm_attn_decode_paged, one row per token);
  (b) the 8-bit path: vlm_kv_quantize_tokens for the chunk's tokens + vlm_attn_prefill_paged_q8 over the 8-bit pools;
  (c) chunks of up to 128 rows: vlm_kv_quantize_tokens + one vlm_attn_decode_paged_q8 row per token - the route the 8-bit path
      takes for chunks of up to 64 rows; (b) and (c) side by side place the crossover.

Device events around `--iters` back-to-back launches, warm-up first, the paths alternated inside every one of `--repeats`
repeats in one process; reported: median, min .. max over the repeats, the ratio b / a, and the share of the new kernel's bound
max(FLOPs / MFMA peak, bytes / HBM peak) in its time.

    python scripts/q8_prefill_attn_bench.py [--out FILE]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mlx_vlm_amd import ops  # noqa: E402

D, PAGE = 128, 64
MFMA_PEAK, HBM_PEAK = 2.5e15, 8.0e12          # MI355X: dense fp16 / bf16 FLOP/s, HBM3E bytes/s
SHAPES = [(4096, 512), (16384, 2048), (32768, 2048), (4096, 32), (4096, 64), (4096, 128)]
HEADS = [(12, 2), (28, 4)]


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters      # us per call


def setup(prefix, chunk, Hq, Hkv):
    dev, bf, i32 = "cuda", torch.bfloat16, torch.int32
    n = prefix + chunk
    pages = (n + PAGE - 1) // PAGE
    g = torch.Generator(device=dev).manual_seed(prefix + chunk + Hq)
    kpool = (torch.randn(pages * Hkv * PAGE * D, device=dev, generator=g) * 0.8).to(bf)
    vpool = (torch.randn(pages * Hkv * PAGE * D, device=dev, generator=g) * 0.8).to(bf)
    bt = torch.randperm(pages, device=dev, generator=g).to(i32).view(1, pages)
    k8, v8 = torch.zeros(kpool.numel(), dtype=torch.uint8, device=dev), torch.zeros(kpool.numel(), dtype=torch.uint8, device=dev)
    ksb, vsb = torch.zeros(kpool.numel() // 64, dtype=i32, device=dev), torch.zeros(kpool.numel() // 64, dtype=i32, device=dev)
    seq, slot = torch.zeros(n, dtype=i32, device=dev), torch.arange(n, dtype=i32, device=dev)
    ops.kv_quantize_tokens(kpool, vpool, k8, v8, ksb, vsb, seq, slot, bt, Hkv, D)          # the prefix is 8-bit already
    qkv = (torch.randn(chunk, (Hq + 2 * Hkv) * D, device=dev, generator=g)).to(bf)
    scale = D ** -0.5
    new_seq, new_slot = seq[prefix:].contiguous(), slot[prefix:].contiguous()
    paths = {}
    if chunk <= 128:
        bt_rows = bt.expand(chunk, pages).contiguous()
        row_len = (prefix + 1 + torch.arange(chunk, device=dev)).to(i32)
        nsplit = 1 if n <= 2048 else max(2, min(32, (n + 16 * PAGE - 1) // (16 * PAGE)))
        if chunk <= 64:
            paths["a"] = lambda: ops.attn_decode_paged(qkv, kpool, vpool, bt_rows, row_len, 0, Hq, Hkv, D, scale, nsplit)
        tickets = torch.zeros(chunk * Hkv, dtype=i32, device=dev)

        def c():
            ops.kv_quantize_tokens(kpool, vpool, k8, v8, ksb, vsb, new_seq, new_slot, bt, Hkv, D)
            return ops.attn_decode_paged_q8(qkv, kpool, vpool, k8, v8, ksb, vsb, bt_rows, row_len, 0, Hq, Hkv, D, scale, nsplit,
                                            quantize_new=False, tickets=tickets)
        paths["c"] = c
    if chunk > 64:
        full = torch.empty(n, (Hq + 2 * Hkv) * D, dtype=bf, device=dev)
        full[prefix:] = qkv
        cu, qs = torch.tensor([0, n], dtype=i32, device=dev), torch.tensor([prefix], dtype=i32, device=dev)
        nqb = (chunk + 127) // 128

        def a():
            ops.kv_gather_(full, Hq, Hkv, D, slot, bt, kpool, vpool, kv_seq=seq)
            return ops.attn_prefill(full, full[:, Hq * D:], full[:, (Hq + Hkv) * D:], cu, nqb, Hq, Hkv, D, scale, True, q_start=qs)
        paths["a"] = a
    seg_seq = torch.zeros(1, dtype=i32, device=dev)
    cu_q, q_start = torch.tensor([0, chunk], dtype=i32, device=dev), torch.tensor([prefix], dtype=i32, device=dev)
    nqb8 = (chunk + ops.Q8_PREFILL_QBLOCK - 1) // ops.Q8_PREFILL_QBLOCK

    def b():
        ops.kv_quantize_tokens(kpool, vpool, k8, v8, ksb, vsb, new_seq, new_slot, bt, Hkv, D)
        return ops.attn_prefill_paged_q8(qkv, k8, v8, ksb, vsb, bt, seg_seq, cu_q, q_start, nqb8, Hq, Hkv, D, scale)
    paths["b"] = b
    paths["b_attn"] = lambda: ops.attn_prefill_paged_q8(qkv, k8, v8, ksb, vsb, bt, seg_seq, cu_q, q_start, nqb8, Hq, Hkv, D, scale)
    return paths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    lines = [f"{torch.cuda.get_device_name(0)}; us per call, median [min .. max] of {args.repeats} repeats x {args.iters} launches, "
             "paths alternated in every repeat",
             "a = kv_gather + attn_prefill(q_start) (chunk <= 64: decode rows, bf16); b = kv_quantize_tokens(chunk) + "
             "attn_prefill_paged_q8; b_attn = the new kernel alone; c = kv_quantize_tokens + attn_decode_paged_q8 rows"]
    for Hq, Hkv in HEADS:
        for prefix, chunk in SHAPES:
            paths = setup(prefix, chunk, Hq, Hkv)
            for fn in paths.values():           # warm-up
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            t = {k: [] for k in paths}
            for _ in range(args.repeats):
                for k, fn in paths.items():
                    t[k].append(timed(fn, args.iters))
            med = {k: statistics.median(v) for k, v in t.items()}
            flops = 4.0 * Hq * D * (chunk * prefix + chunk * (chunk + 1) / 2)
            nbytes = (prefix + chunk) * Hkv * (2 * D + 16) + 2 * chunk * Hq * D * 2
            tf, tb = flops / MFMA_PEAK * 1e6, nbytes / HBM_PEAK * 1e6
            bound, which = max(tf, tb), "MFMA" if tf >= tb else "HBM"
            spread = max((max(v) - min(v)) / statistics.median(v) for v in t.values())
            row = f"Hq {Hq:2d} Hkv {Hkv} prefix {prefix:5d} chunk {chunk:4d}: " + "  ".join(
                f"{k} {med[k]:9.1f} [{min(t[k]):9.1f} .. {max(t[k]):9.1f}]" for k in t)
            row += (f"  | b/a {med['b'] / med['a']:.2f} (spread {spread:.1%})  bound {bound:.1f} us ({which}) = "
                    f"{bound / med['b_attn']:.1%} of b_attn")
            if "c" in med:
                row += f"  c/b {med['c'] / med['b']:.2f}"
            print(row, flush=True)
            lines.append(row)
            del paths
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
