"""Decode at Qwen2-VL-72B widths on one GPU: per-launch times, fused forms against the launches they replace.

    python scripts/wide_hidden_decode_bench.py [--layers 4] [--rounds 5] > profiles/wide_hidden_decode.txt

A synthetic model of `--layers` decoder layers at the full 72B widths (hidden 8192, intermediate 29568, 64 query heads over
8 KV heads of 128, vocabulary 152064, untied head), bf16 and MLX 4-bit.  No 72B checkpoint is involved: the 80-layer token
rate at the end is an EXTRAPOLATION from the per-layer numbers and is labelled so.

What is measured, the accounting of VERDICT.md / benchlib (HIP events around replays of one hipGraph that holds the launch
for every layer in turn - the layers' matrices together exceed the 256 MB Infinity Cache, so every launch streams from HBM):
  * every weight-streaming launch of a layer at 1, 4 and 16 rows: us per launch and its algorithmic bytes (the weights) as a
    fraction of 8 TB/s;
  * for the norm-prologue launches (qkv with its rotary + KV-write epilogue, gate/up with SwiGLU, the head) two arms taken in
    ALTERNATION (A B A B ...): the fused form, and the composition RMSNorm | projection | rotary + KV write that needs no new
    kernel.  Per arm the median over the rounds and the spread (max - min); a fused form is worth keeping where it is faster
    than the composition by more than that spread;
  * the whole captured step (generate_step / batch_generate_ids, contexts near 500 tokens): us per step.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 8e12
BF = torch.bfloat16


def graph_time(fn, per, reps=4):
    """seconds per launch group: fn() (one launch group per layer, `per` groups) captured once, HIP events over replays"""
    from benchlib.common import time_events

    fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    g.replay()
    torch.cuda.synchronize()
    return g, lambda: time_events(g.replay, reps) / per


def arms(named, rounds):
    """named: [(name, timer or None)] -> {name: (median us, spread us)}; the arms alternate within every round"""
    got = {n: [] for n, t in named if t is not None}
    for _ in range(rounds):
        for n, t in named:
            if t is not None:
                got[n].append(t() * 1e6)
    return {n: (statistics.median(v), max(v) - min(v)) for n, v in got.items()}


def try_build(fn, per):
    from mlx_vlm_amd._lib import VlmHipError

    try:
        return graph_time(fn, per)
    except VlmHipError as e:
        return None, str(e)


def bench_model(w4, args):
    from mlx_vlm_amd import ops, synthetic
    from mlx_vlm_amd.models import quantized as Qz
    from mlx_vlm_amd.models import qwen2_vl

    cfgd = dict(synthetic.QWEN2_VL_7B, hidden_size=8192, intermediate_size=29568, num_attention_heads=64, num_key_value_heads=8,
                num_hidden_layers=args.layers, vocab_size=152064, tie_word_embeddings=False,
                vision_config=dict(synthetic.QWEN2_VL_7B["vision_config"], hidden_size=8192, depth=2))
    cfg = qwen2_vl.ModelConfig.from_dict(cfgd)
    W = synthetic.random_weights(cfg, seed=0, device="cuda")
    if w4:
        synthetic.quantize_random_(W)
    nbytes = sum(v.numel() * v.element_size() for k, v in W.items() if k.startswith("language_model."))
    model = qwen2_vl.Model(cfg, device="cuda", kv_pool_tokens=16384, max_seqs=32)
    model.load_weights(W)
    del W
    torch.cuda.synchronize()
    lm = model.language_model
    tag = "4-bit" if w4 else "bf16"
    L, D, I, V, Hq, Hkv, hd = args.layers, 8192, 29568, 152064, 64, 8, 128
    QKV = (Hq + 2 * Hkv) * hd
    print(f"\n==== {tag}: {L} layers at 72B widths, language model {nbytes / 1e9:.2f} GB")

    def wb(n, k):                      # algorithmic bytes of one projection: its weights
        return n * k // 2 + n * (k // 64) * 4 if w4 else 2 * n * k

    def mat(key):
        w = lm._w[key]
        return (w.wq, w.sb) if isinstance(w, Qz.QuantW) else (w,)

    gemv = ops.gemv_w4_ws if w4 else ops.gemv_ws
    qkv_fused = ops.gemv_w4_qkv_rope_kvwrite_ws if w4 else ops.gemv_qkv_rope_kvwrite_ws
    inv = (1.0 / (1e6 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))).cuda()
    layer_sum = {}
    for B in (1, 4, 16):
        g = torch.Generator(device="cuda").manual_seed(B)
        h = torch.randn(B, D, device="cuda", generator=g).to(BF)
        act = torch.randn(B, I, device="cuda", generator=g).to(BF)
        attn = torch.randn(B, Hq * hd, device="cuda", generator=g).to(BF)
        xn = torch.empty_like(h)
        qkv = torch.zeros(B, QKV, dtype=BF, device="cuda")
        out_gu = torch.empty(B, I, dtype=BF, device="cuda")
        logits = torch.empty(B, V, dtype=BF, device="cuda")
        pos = torch.full((B,), 500, dtype=torch.int32, device="cuda")
        slot = torch.full((B,), 500, dtype=torch.int32, device="cuda")
        seq = torch.arange(B, dtype=torch.int32, device="cuda")
        max_pages = 8
        bt = torch.arange(B * max_pages, dtype=torch.int32, device="cuda").reshape(B, max_pages)
        kpool = torch.zeros(B * max_pages, Hkv, hd // 8, 64, 8, dtype=BF, device="cuda")
        vpool = torch.zeros(B * max_pages, Hkv, hd, 64, dtype=BF, device="cuda")

        def qkv_f():
            for i in range(L):
                qkv_fused(h, lm._w[f"{i}.ln1"], *mat(f"{i}.wqkv"), lm._w[f"{i}.bqkv"], Hq, Hkv, hd, pos, slot, inv, bt, kpool, vpool,
                          out=qkv)

        def qkv_c():
            for i in range(L):
                ops.rmsnorm(h, lm._w[f"{i}.ln1"], out=xn)
                gemv(xn, *mat(f"{i}.wqkv"), bias=lm._w[f"{i}.bqkv"], out=qkv, epilogue=ops.EPI_BIAS)
                ops.mrope_kvwrite_(qkv, Hq, Hkv, hd, pos, pos, pos, inv, 16, 24, kv_seq=seq, kv_slot=slot, block_table=bt, kpool=kpool,
                                   vpool=vpool)

        def gu_f():
            for i in range(L):
                gemv(h, *mat(f"{i}.wgu"), norm_w=lm._w[f"{i}.ln2"], out=out_gu, epilogue=ops.EPI_SWIGLU)

        def gu_c():
            for i in range(L):
                ops.rmsnorm(h, lm._w[f"{i}.ln2"], out=xn)
                gemv(xn, *mat(f"{i}.wgu"), out=out_gu, epilogue=ops.EPI_SWIGLU)

        def head_f():
            gemv(h, *mat("head"), norm_w=lm._w["norm"], out=logits)

        def head_c():
            ops.rmsnorm(h, lm._w["norm"], out=xn)
            gemv(xn, *mat("head"), out=logits)

        def o_f():
            for i in range(L):
                gemv(attn, *mat(f"{i}.wo"), res=h, out=h, epilogue=ops.EPI_RESIDUAL)

        def down_f():
            for i in range(L):
                gemv(act, *mat(f"{i}.wdown"), res=h, out=h, epilogue=ops.EPI_RESIDUAL)

        print(f"\n-- {tag}, {B} row(s): us per launch (median of {args.rounds} alternating rounds, spread = max - min), "
              f"fraction of 8 TB/s over the weights' bytes")
        total, untimed = 0.0, []
        for name, fused, comp, per, nb in (("qkv + rope + KV write", qkv_f, qkv_c, L, wb(QKV, D)),
                                           ("gate/up + SwiGLU", gu_f, gu_c, L, wb(2 * I, D)),
                                           ("head", head_f, head_c, 1, wb(V, D)),
                                           ("o_proj + residual", o_f, None, L, wb(D, Hq * hd)),
                                           ("down + residual", down_f, None, L, wb(D, I))):
            built = [("fused" if comp else "launch", try_build(fused, per))]
            if comp:
                built.append(("composition", try_build(comp, per)))
            res = arms([(n, b[1] if b[0] is not None else None) for n, b in built], args.rounds)
            line, best = [], None
            for n, b in built:
                if b[0] is None:
                    line.append(f"{n}: no such launch at the operator level ({b[1].split('failed: ')[-1]})")
                    continue
                med, spread = res[n]
                best = med if best is None else min(best, med)
                line.append(f"{n} {med:8.1f} us (spread {spread:5.1f}) {nb / (med * 1e-6) / HBM * 100:5.1f} %")
            verdict = ""
            if comp and "fused" in res and "composition" in res:
                f, c = res["fused"], res["composition"]
                gain, noise = c[0] - f[0], max(f[1], c[1])
                verdict = f" -> fused {'KEPT' if gain > noise else 'NOT faster than the composition by more than the spread'} (gain {gain:+.1f} us)"
            print(f"  {name:24s} {nb / 1e6:8.1f} MB  " + " | ".join(line) + verdict)
            if best is not None and per == L:
                total += best
            elif per == L:
                untimed.append(name.split(" + ")[0])
            del built
        # a launch the operator level refuses runs in the engine as slices of the weight rows / halves of the batch rows: it is part
        # of the captured step below but has no time of its own here, so the sum is labelled
        part = f"PARTIAL sum - no time for {', '.join(untimed)}, which the engine runs as slices / halves (not timed here) - of" if untimed \
            else "sum of"
        layer_sum[B] = (total, untimed)
        print(f"  {part} a layer's weight launches: {total:.1f} us")
    # ---- the captured step end to end
    from benchlib.common import build_request, run_step
    from mlx_vlm_amd.generate import batch_generate_ids

    step_us = {}
    req = build_request(model.config, 336, 355, 7)            # 144 image tokens + 2 + 355 text = 501
    run_step(model, req, 8, 8)
    _, dt, toks = run_step(model, req, 65, 8)
    step_us[1] = dt / (len(toks) - 1) * 1e6
    for B in (4, 16):
        reqs = [build_request(model.config, 336, 340 + 3 * i, 500 + i) for i in range(B)]
        ids, pix, thw = [r[0].reshape(-1) for r in reqs], [r[1] for r in reqs], [r[2] for r in reqs]
        batch_generate_ids(model, ids, pix, thw, max_tokens=8)
        torch.cuda.synchronize()
        _, stats = batch_generate_ids(model, ids, pix, thw, max_tokens=48)
        step_us[B] = B / stats.generation_tps * 1e6
    print(f"\n-- {tag}: captured step, contexts near 500 tokens, {L} layers + head + sampler")
    for B in (1, 4, 16):
        print(f"  {B:2d} row(s): {step_us[B]:8.1f} us per step = {step_us[B] / L:7.1f} us per layer with the head and the tail spread "
              f"over {L} layers; the layer's weight launches alone {layer_sum[B][0]:.1f} us"
              + (f" (PARTIAL: without {', '.join(layer_sum[B][1])})" if layer_sum[B][1] else ""))
    print(f"  EXTRAPOLATION (no 72B checkpoint was run): 80 layers x the measured weight launches + attention ~ "
          + ", ".join(f"{B} row(s) {B / ((step_us[B] - 0) / L * 80 * 1e-6):.1f} tok/s" for B in (1, 4, 16))
          + f"  (step / {L} x 80, which counts the head {80 // L} times: a lower bound)")
    del model, lm
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="", choices=["", "bf16", "w4"])
    args = ap.parse_args()
    torch.cuda.set_device(0)
    print(f"wide_hidden_decode_bench: {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}")
    for w4 in (False, True):
        if args.only and (args.only == "w4") != w4:
            continue
        bench_model(w4, args)


if __name__ == "__main__":
    main()
