"""Decode throughput of constrained rows: the mask processor on the captured step against the same constraint written as a
plain callable (the eager step) and against unconstrained rows (profiles/token_mask_decode.txt).

    python scripts/token_mask_decode.py --config mask|callable|free [--rows 1 16] [--tokens 256] [--repeats 5]

Synthetic Qwen2-VL-2B dimensions (benchlib), greedy, text prompts of 128 tokens.  At 16 rows 8 are constrained and 8 free.
The stand-in matcher allows about 30 seeded tokens per step, chosen from the step index and the token it was last handed; its
host time is accumulated separately and printed beside the decode rate (it is inside the rate's wall time in both constrained
configurations).  `callable` uses nothing this change adds, so the same file runs on a checkout without it.  One JSON line per
(config, rows)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V_TOK = 151643


class Matcher:
    spent = 0.0

    def __init__(self, seed, n_words):
        self.seed, self.n_words, self.first, self.step = seed, n_words, True, 0

    def next_tokens(self, last_token):
        t0 = time.perf_counter()
        key = 0 if self.first else int(last_token) + 1
        self.first = False
        toks = np.random.default_rng([self.seed, self.step, key]).integers(0, V_TOK, 30)
        self.step += 1
        Matcher.spent += time.perf_counter() - t0
        return toks

    def prepare_next_token_mask(self, last_token):
        toks = self.next_tokens(last_token)
        t0 = time.perf_counter()
        words = np.zeros(self.n_words, dtype=np.uint32)
        np.bitwise_or.at(words, toks >> 5, np.uint32(1) << (toks & 31).astype(np.uint32))
        Matcher.spent += time.perf_counter() - t0
        return words.view(np.int32)[None]


class AsCallable:
    def __init__(self, seed, n_words):
        self.m = Matcher(seed, n_words)

    def __call__(self, tokens, logits):
        toks = self.m.next_tokens(int(tokens[-1]))
        ok = torch.zeros(logits.shape[-1], dtype=torch.bool)
        ok[torch.from_numpy(toks)] = True
        return logits.masked_fill(~ok.to(logits.device)[None], float("-inf"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", required=True, choices=["mask", "callable", "free"])
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    from benchlib.common import _load_synthetic
    from mlx_vlm_amd import synthetic
    from mlx_vlm_amd.batch import BatchGenerator
    from mlx_vlm_amd.models import qwen2_vl

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    cfg, model, _ = _load_synthetic(synthetic.QWEN2_VL_2B, qwen2_vl, 0, dev, kv_pool_tokens=32768, max_seqs=40)
    V = model.language_model.args.vocab_size
    n_words = (V + 31) // 32
    form = {"mask": Matcher, "callable": AsCallable}.get(args.config)
    for rows in args.rows:
        n_masked = 0 if form is None else max(1, rows // 2)
        prompts = [np.random.default_rng(100 + i).integers(0, V_TOK, 128) for i in range(rows)]
        rates, host = [], []
        for rep in range(args.repeats + 1):                     # the first pass warms up (graph capture, allocator) and is dropped
            procs = [form(10 * rep + i, n_words) if i < n_masked else None for i in range(rows)]
            gen = BatchGenerator(model, None, max_tokens=args.tokens, completion_batch_size=rows, prefill_batch_size=rows)
            Matcher.spent = 0.0
            gen.insert(prompts, args.tokens, logits_processors=procs)
            n = 0
            while gen.has_work:
                n += len(gen.next()[1])
            st = gen.stats()
            gen.close()
            assert n == rows * args.tokens
            if rep:
                rates.append(st.generation_tps)
                host.append(1e6 * Matcher.spent / max(1, n_masked * args.tokens))
        print(json.dumps({"config": args.config, "rows": rows, "masked_rows": n_masked, "tokens": args.tokens,
                          "decode_tok_s": [round(r, 1) for r in rates], "median": round(float(np.median(rates)), 1),
                          "min": round(min(rates), 1), "max": round(max(rates), 1),
                          "matcher_us_per_masked_token": round(float(np.median(host)), 1)}), flush=True)


if __name__ == "__main__":
    main()
