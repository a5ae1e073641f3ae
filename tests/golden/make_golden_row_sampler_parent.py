"""Tokens of a BatchGenerator that never hears of per-request samplers, recorded ONCE from the commit before
`insert(..., samplers=)` existed: one seeded sampled run and one greedy run over the tiny Qwen2-VL of the batch tests, with the
number of launches of their last captured step.  tests/test_row_sampler_gpu.py runs `workload` on the current tree and expects
the same numbers: such a generator keeps its shared sampler, its (seed, step, row, index) draws and its launches.

    python tests/golden/make_golden_row_sampler_parent.py     # on an MI355X, from a checkout of that commit;
                                                              # writes tests/golden/row_sampler_parent_tokens.json
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "row_sampler_parent_tokens.json")

MAX_TOKENS = [5, 9, 3, 7, 12, 4, 6]


def tiny_model():
    """oracle.qwen2_vl.tiny_cfg with the seeded weights of the batch tests (seed 1234) and NO peaked head: the rows are flat
    enough that a sampled request leaves the greedy path at once.  Every comparison made with it is between runs that step
    the same rows at the same widths through the same kernels, so near-ties at the top of a row do no harm."""
    from oracle import qwen2_vl as oq
    from tests.helpers import build_product_model

    BF = torch.bfloat16
    cfg = oq.tiny_cfg()
    cfg.text.tie_word_embeddings = False
    W = oq.random_weights(cfg, seed=1234, dtype=BF, std=0.05, embed_std=0.2)
    for k in list(W):
        if k.endswith("o_proj.weight") or k.endswith("down_proj.weight"):
            W[k] = (W[k].float() * 0.5).to(BF)
    return cfg, build_product_model(cfg, W, kv_pool_tokens=32768, max_seqs=80)


def prompts(n=7, seed0=900):
    """text prompts of different lengths"""
    return [np.random.default_rng(seed0 + i).integers(3, 1000, 5 + 3 * (i % 7)) for i in range(n)]


def run(model, sampler=None, samplers=None, use_graph=True, rows=4, gen_cls=None):
    """-> (tokens per request, token_logprob per request, launches of the last step)"""
    from mlx_vlm_amd import _lib
    from mlx_vlm_amd.batch import BatchGenerator

    gen = (gen_cls or BatchGenerator)(model, None, max_tokens=8, completion_batch_size=rows, prefill_batch_size=rows,
                                      async_prefill=False, use_graph=use_graph, sampler=sampler)
    kw = {} if samplers is None else {"samplers": samplers}
    uids = gen.insert(prompts(), list(MAX_TOKENS), **kw)
    toks, lps = {u: [] for u in uids}, {u: [] for u in uids}
    while gen.has_work:
        _, out = gen.next()
        for r in out:
            toks[r.uid].append(int(r.token))
            lps[r.uid].append(float(r.token_logprob))
    launches = int(_lib.lib().vlm_llm_decode_launches(model.language_model._handle))
    gen.close()
    assert [len(toks[u]) for u in uids] == MAX_TOKENS
    return [toks[u] for u in uids], [lps[u] for u in uids], launches


def workload(model):
    from mlx_vlm_amd.sample_utils import make_sampler

    out = {}
    for name, smp in (("sampled", make_sampler(temp=0.8, top_p=0.9, min_p=0.02, top_k=50, seed=4321)), ("greedy", None)):
        toks, _, launches = run(model, sampler=smp)
        out[name] = {"tokens": toks, "launches": launches}
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    _, model = tiny_model()
    res = workload(model)
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
