#!/usr/bin/env python
"""The attention of a warm admission, new against old, at 8 segments of 32 rows over a 1024-token prefix each (Hq 12 / Hkv 2,
D 128): ops.attn_prefill_paged (csrc/attn_prefill_paged.hip) against ops.kv_gather_ + ops.attn_prefill(q_start=), the path
`_prefill_onto_cache` takes without it.  Prints the distance of the two outputs and event-timed launch times; run under
`rocprofv3 --kernel-trace --stats` (a run of its own) for the kernel times.

    python scripts/apc_attn_kernels.py [--reps 50]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    from mlx_vlm_amd import ops

    dev, bf = "cuda", torch.bfloat16
    S, rows, prefix, Hq, Hkv, D = 8, 32, 1024, 12, 2, 128
    tot = prefix + rows
    max_pages = (tot + 63) // 64 + 1
    n_pages = S * max_pages
    g = torch.Generator(device=dev).manual_seed(0)
    kpool = (torch.randn(n_pages * Hkv * 64 * D, generator=g, device=dev) * 0.8).to(bf)
    vpool = (torch.randn(n_pages * Hkv * 64 * D, generator=g, device=dev) * 0.8).to(bf)
    perm = torch.randperm(n_pages, generator=torch.Generator().manual_seed(1)).to(torch.int32).view(S, max_pages)
    bt = perm.to(dev).contiguous()
    q = torch.randn(S * rows, Hq * D, generator=g, device=dev).to(bf)
    i32 = lambda x: torch.tensor(np.asarray(x), dtype=torch.int32, device=dev)         # noqa: E731
    seg, cu, qs = i32(np.arange(S)), i32(np.arange(S + 1) * rows), i32(np.full(S, prefix))
    nqb = S * ((rows + ops.PAGED_PREFILL_QBLOCK - 1) // ops.PAGED_PREFILL_QBLOCK)

    def paged():
        return ops.attn_prefill_paged(q, kpool, vpool, bt, seg, cu, qs, nqb, Hq, Hkv, D, D ** -0.5)

    cu_full = i32(np.arange(S + 1) * tot)
    new_rows = torch.from_numpy(np.concatenate([np.arange(s * tot + prefix, (s + 1) * tot) for s in range(S)])).to(dev)
    seq_all, slot_all = i32(np.repeat(np.arange(S), tot)), i32(np.tile(np.arange(tot), S))
    nqb_g = S * ((rows + 127) // 128)

    def gathered():
        full = torch.empty(S * tot, (Hq + 2 * Hkv) * D, dtype=bf, device=dev)
        full[new_rows, : Hq * D] = q
        ops.kv_gather_(full, Hq, Hkv, D, slot_all, bt, kpool, vpool, kv_seq=seq_all)
        att = ops.attn_prefill(full, full[:, Hq * D:], full[:, (Hq + Hkv) * D:], cu_full, nqb_g, Hq, Hkv, D, D ** -0.5, True, q_start=qs)
        return att[new_rows]

    a, b = paged().float(), gathered().float()
    rel = float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())
    assert torch.isfinite(a).all() and rel < 5e-4, rel

    def timed(fn):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.reps

    res = {"paged_us": [], "gather_path_us": []}
    for _ in range(3):                                   # alternated
        res["paged_us"].append(timed(paged))
        res["gather_path_us"].append(timed(gathered))
    print("APC_ATTN " + json.dumps(dict(segments=S, rows=rows, prefix=prefix, Hq=Hq, Hkv=Hkv, rel_rms_paged_vs_gather=rel,
                                        event_timed_us_per_call=res)))


if __name__ == "__main__":
    main()
