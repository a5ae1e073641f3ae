"""What top_logprobs costs (profiles/top_logprobs.txt).  Two measurements, to be taken inside ONE GPU session (box-to-box
spread is 1.5x, docs/HISTORY.md):

    python scripts/top_logprobs_bench.py kernel
        microseconds of one ops.top_logprobs call at V = 151,936 for B in {1, 16, 64} and K in {5, 20, 64}: device events
        around replays of a hipGraph of 20 calls (rows of N(0, 2^2) log-probs, resident in L2 / MALL from the call before -
        as they are behind a decode step, whose sampler has just written them).

    python scripts/top_logprobs_bench.py decode --k K [--root TREE]
        decode tokens/s of BatchGenerator at Qwen2-VL-2B dimensions (synthetic weights), 16 and 64 rows, compute_logprobs=True,
        text prompts of 32 tokens, 128 new tokens per request, three repeats per row count.  --k 0 does not pass the keyword
        at all, so the same command measures a checkout of the parent commit given as --root (the tree whose package is
        imported; default: the tree this script lies in).
"""
import argparse
import os
import sys
import time


def kernel_table():
    import torch
    from mlx_vlm_amd import ops

    V = 151936
    print(f"top_logprobs_kernel, V = {V}, us per call (median of 7 replays of a graph of 20 calls; min .. max)")
    for B in (1, 16, 64, -16):
        overflow, B = B < 0, abs(B)
        g = torch.Generator().manual_seed(B)
        x = torch.randn(B, V, generator=g) * 2.0
        lp = (x - torch.logsumexp(x, -1, keepdim=True)).to(torch.bfloat16)
        if overflow:
            # every large value in the 16-byte chunks c with c % 64 < 2 (two of the kernel's 64 lane groups): ~4,750 elements pass
            # the bound, the LDS list overflows and the select runs over the row (tests/test_top_logprobs_gpu.py's row)
            hot = ((torch.arange(V) // 8) % 64) < 2
            lp = (lp.float() - 20.0).to(torch.bfloat16)
            lp[:, hot] = (-torch.rand(B, int(hot.sum()), generator=g) * 3.0 - 0.5).to(torch.bfloat16)
            print("  rows that overflow the LDS list (the select runs over the row):")
        lp = lp.cuda()
        for K in (5, 20, 64):
            out = (torch.empty(B, K, dtype=torch.int32, device="cuda"), torch.empty(B, K, dtype=torch.bfloat16, device="cuda"))
            ops.top_logprobs(lp, K, out=out)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(20):
                    ops.top_logprobs(lp, K, out=out)
            graph.replay()
            torch.cuda.synchronize()
            us = []
            for _ in range(7):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                graph.replay()
                b.record()
                b.synchronize()
                us.append(a.elapsed_time(b) * 1e3 / 20)
            us.sort()
            print(f"  B = {B:2d}  K = {K:2d}   {us[3]:7.1f}   ({us[0]:.1f} .. {us[-1]:.1f})", flush=True)


def decode_table(k, label):
    import numpy as np
    import torch
    from mlx_vlm_amd import synthetic
    from mlx_vlm_amd.batch import BatchGenerator
    from mlx_vlm_amd.models import qwen2_vl

    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = qwen2_vl.ModelConfig.from_dict(dict(synthetic.QWEN2_VL_2B))
    W = synthetic.random_weights(cfg, seed=0, device=dev)
    model = qwen2_vl.Model(cfg, device=dev, kv_pool_tokens=49152, max_seqs=2 * 64 + 8)
    model.load_weights(W)
    del W
    kw = dict(top_logprobs_k=k) if k else {}
    for rows in (16, 64):
        prompts = [np.random.default_rng(300 + i).integers(0, 151643, 32) for i in range(rows)]

        def run(new_tokens):
            gen = BatchGenerator(model, None, completion_batch_size=rows, prefill_batch_size=rows, compute_logprobs=True, **kw)
            gen.insert(prompts, new_tokens)
            n = 0
            while gen.has_work:
                for r in gen.next()[1]:
                    n += 1
                    assert (r.top_logprobs is None) == (k == 0) and (k == 0 or len(r.top_logprobs) == k)
            st = gen.stats()
            gen.close()
            return st

        run(8)
        torch.cuda.synchronize()
        res = []
        for _ in range(3):
            st = run(128)
            res.append((st.generation_tps, 1e6 * st.generation_time / max(st.decode_steps, 1)))
        tps = sorted(r[0] for r in res)
        us = sorted(r[1] for r in res)
        print(f"  {label:<22s} rows = {rows:2d}   decode tokens/s {tps[1]:9.1f}  ({tps[0]:.1f} .. {tps[2]:.1f})   "
              f"us per step {us[1]:7.1f}  ({us[0]:.1f} .. {us[2]:.1f})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "decode"])
    ap.add_argument("--k", type=int, default=0)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    t0 = time.perf_counter()
    if args.what == "kernel":
        kernel_table()
    else:
        decode_table(args.k, args.label or f"k = {args.k}")
    print(f"  ({time.perf_counter() - t0:.0f} s)", flush=True)


if __name__ == "__main__":
    main()
