#!/usr/bin/env python
"""Time to first token of the benchmark's request shape through BatchGenerator, cold against warm (automatic prefix caching).

Qwen2-VL-2B dimensions with synthetic weights; one 448 x 448 image (256 image tokens) + 128 text tokens; the requests share the
image and all but the last 16 tokens (the "question").  Arms, alternated trial by trial in ONE process:
    cold   a generator without a manager (every request pays the ViT and the whole prefill);
    warm   a generator with an APCManager that holds the shared prefix (5 full blocks = 320 of 386 tokens).
The clock runs from insert() to the first Response of the request (its token has reached pinned host memory behind a device
event, so the window ends in a synchronise).  `--no-apc` runs the cold arm alone (a tree without apc.py: the parent commit).

    python scripts/apc_ttft.py [--trials 30] [--no-apc]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ttft(gen, ids, kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    (uid,) = gen.insert([ids], 2, prompt_kwargs=[kw])
    t1 = None
    while gen.has_work:
        _, out = gen.next()
        if t1 is None and any(r.uid == uid for r in out):
            t1 = time.perf_counter()
    return (t1 - t0) * 1e3


def summary(x):
    x = np.sort(np.asarray(x))
    return dict(n=len(x), median_ms=float(np.median(x)), min_ms=float(x[0]), p10_ms=float(np.percentile(x, 10)),
                p90_ms=float(np.percentile(x, 90)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--no-apc", action="store_true")
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    from benchlib.common import _load_synthetic, build_request
    from mlx_vlm_amd import synthetic
    from mlx_vlm_amd.batch import BatchGenerator
    from mlx_vlm_amd.models import qwen2_vl

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    cfg, model, _ = _load_synthetic(synthetic.QWEN2_VL_2B, qwen2_vl, 0, dev, kv_pool_tokens=32768, max_seqs=40)
    ids, pix, thw = build_request(cfg, 448, 128, seed=0)
    ids = ids.reshape(-1)
    kw = dict(pixel_values=pix, image_grid_thw=thw)
    rng = np.random.default_rng(5)

    def request():
        r = ids.copy()
        r[-16:] = rng.integers(0, 151643, 16)
        return r

    arms = {"cold": BatchGenerator(model, None, max_tokens=2, compute_logprobs=False)}
    if not args.no_apc:
        from mlx_vlm_amd.apc import APCManager

        mgr = APCManager(num_blocks=64)
        arms["warm"] = BatchGenerator(model, None, max_tokens=2, compute_logprobs=False, apc_manager=mgr)
    times = {k: [] for k in arms}
    for i in range(args.warmup + args.trials):
        r = request()
        for k, g in arms.items():                       # the same request through both arms, alternating
            t = ttft(g, r, kw)
            if i >= args.warmup:
                times[k].append(t)
    out = {"tag": args.tag, "prompt_tokens": int(ids.size), "arms": {k: summary(v) for k, v in times.items()}}
    if not args.no_apc:
        s = mgr.stats_snapshot()
        out["apc"] = {k: s[k] for k in ("lookups_hit", "lookups_miss", "matched_tokens", "served_tokens", "token_hit_rate", "stores")}
    for g in arms.values():
        g.close()
    print("APC_TTFT " + json.dumps(out))


if __name__ == "__main__":
    main()
