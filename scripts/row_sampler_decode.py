"""Decode throughput of per-request samplers: the row-table step against the shared-sampler step it is built from and against
the eager step with a Python sampler callable - the only way to give rows different samplers before
(profiles/row_sampler_decode.txt).

    python scripts/row_sampler_decode.py [--rows 1 8 16] [--tokens 256] [--repeats 5]

Synthetic Qwen2-VL-2B dimensions (benchlib), text prompts of 128 tokens.  Configurations, run one after the other inside every
repeat (the same process, the same model, alternating):
  shared    BatchGenerator(sampler=S), no per-request samplers: the captured step of the scalar path
  rows      insert(samplers=[S] * rows): the row-table step, every row with the settings of S (its own seed)
  rows_half insert(samplers=...): the row-table step, the first ceil(rows / 2) rows greedy, the others S
  callable  BatchGenerator(sampler=f), f a Python callable that calls S on the log-prob rows: the eager step (forward,
            log-probs, f, advance) doing the work of `rows`
  callable_half  ... f takes the argmax of the first ceil(rows / 2) log-prob rows and calls S on the others: the eager step
            doing the work of `rows_half` (at one row: the argmax alone)
S = temperature 0.7, top-p 0.9, min-p 0.05, top-k 40.  decode tok/s is the generator's own clock (stats().generation_tps).
The first pass of every (configuration, rows) warms up (graph capture, allocator) and is dropped.  One JSON line per
(configuration, rows)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V_TOK = 151643
S = dict(temp=0.7, top_p=0.9, min_p=0.05, top_k=40)
CONFIGS = ("shared", "rows", "rows_half", "callable", "callable_half")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 8, 16])
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    from benchlib.common import _load_synthetic
    from mlx_vlm_amd import synthetic
    from mlx_vlm_amd.batch import BatchGenerator
    from mlx_vlm_amd.models import qwen2_vl
    from mlx_vlm_amd.sample_utils import make_sampler

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    cfg, model, _ = _load_synthetic(synthetic.QWEN2_VL_2B, qwen2_vl, 0, dev, kv_pool_tokens=32768, max_seqs=40)

    def one(config, rows, rep):
        n_greedy = (rows + 1) // 2 if config.endswith("_half") else 0
        shared, samplers = None, None
        if config == "shared":
            shared = make_sampler(seed=1000 + rep, **S)
        elif config == "rows":
            samplers = [make_sampler(seed=1000 + 16 * rep + i, **S) for i in range(rows)]
        elif config == "rows_half":
            samplers = [make_sampler() if i < n_greedy else make_sampler(seed=1000 + 16 * rep + i, **S) for i in range(rows)]
        else:
            smp = make_sampler(seed=1000 + rep, **S)

            def mixed(logprobs):                    # the generator-wide Python sampler: logprobs [n, V] -> tokens [n]
                if 0 < n_greedy >= logprobs.shape[0]:   # (rows are dense from 0: the greedy ones come first)
                    return torch.argmax(logprobs.float(), dim=-1).to(torch.int32)
                if n_greedy == 0:
                    return smp(logprobs)
                return torch.cat([torch.argmax(logprobs[:n_greedy].float(), dim=-1).to(torch.int32), smp(logprobs[n_greedy:])])

            shared = mixed
        prompts = [np.random.default_rng(100 + i).integers(0, V_TOK, 128) for i in range(rows)]
        gen = BatchGenerator(model, None, max_tokens=args.tokens, completion_batch_size=rows, prefill_batch_size=rows, sampler=shared)
        gen.insert(prompts, args.tokens, **({} if samplers is None else {"samplers": samplers}))
        n = 0
        while gen.has_work:
            n += len(gen.next()[1])
        st = gen.stats()
        gen.close()
        assert n == rows * args.tokens
        return st.generation_tps

    for rows in args.rows:
        rates = {c: [] for c in CONFIGS}
        for rep in range(args.repeats + 1):
            for c in CONFIGS:
                r = one(c, rows, rep)
                if rep:
                    rates[c].append(r)
        for c in CONFIGS:
            v = rates[c]
            print(json.dumps({"config": c, "rows": rows, "greedy_rows": (rows + 1) // 2 if c.endswith("_half") else 0,
                              "tokens": args.tokens, "decode_tok_s": [round(x, 1) for x in v],
                              "median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1)}), flush=True)


if __name__ == "__main__":
    main()
