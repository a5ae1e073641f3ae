"""LanguageModel._prefill_onto_cache with TWO sequences of different cache lengths (70 and 130 tokens) in one `lm.prefill` call,
once per attention route (the other tests of the non-paged routes drive one sequence per call): every route is forced by the
public means only - the chunk's length, VLM_ONTO_CACHE_DECODE_ATTN / VLM_ONTO_CACHE_QSTART, `paged_attn=True`, `quantize_kv` -
and a spy on the attention operators shows that it was the one that ran.  Per sequence: the chunk's last-row logits and the
NEXT decode step's logits (which reads the K / V the chunk wrote) against the sequence's own one-shot prefill, and the offsets.
Bars: 1e-2 rel-rms for the bf16 routes (tests/test_engine_gpu.py::test_prompt_chunk_onto_a_cache_three_attention_forms_agree),
2e-2 for the 8-bit routes (tests/test_kv_quant_prefill_gpu.py's ROW_BAR); the 8-bit reference quantises its cache after the
one-shot prefill, as that file's oracle does."""
import numpy as np
import pytest
import torch

from mlx_vlm_amd import ops
from oracle import qwen2_vl as oq
from tests.helpers import build_product_model

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
PREFIXES = (70, 130)
CHUNKS = {"short": (5, 20), "long": (70, 30)}
NEXT_TOKEN = 77
ATTN_OPS = ("attn_prefill", "attn_prefill_paged", "attn_prefill_paged_q8", "attn_decode_paged", "attn_decode_paged_q8")
# route -> (paged_attn, 8-bit cache, chunks, environment, the attention operator of the route, bar)
ROUTES = {
    "paged": (True, False, "long", {}, "attn_prefill_paged", 1e-2),
    "paged_short": (True, False, "short", {}, "attn_prefill_paged", 1e-2),
    "q8_decode": (False, True, "short", {}, "attn_decode_paged_q8", 2e-2),
    "q8_paged": (False, True, "long", {}, "attn_prefill_paged_q8", 2e-2),
    "q8_paged_by_env": (False, True, "short", {"VLM_ONTO_CACHE_DECODE_ATTN": "0"}, "attn_prefill_paged_q8", 2e-2),
    "decode": (False, False, "short", {}, "attn_decode_paged", 1e-2),
    "gather": (False, False, "long", {}, "attn_prefill", 1e-2),
    "gather_by_env": (False, False, "short", {"VLM_ONTO_CACHE_DECODE_ATTN": "0"}, "attn_prefill", 1e-2),
    "gather_zero_queries": (False, False, "long", {"VLM_ONTO_CACHE_QSTART": "0"}, "attn_prefill", 1e-2),
}


def _rel_rms(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30))


def _inputs(lm, kind):
    """per sequence: (embeddings [prefix + chunk, D], positions [3, prefix + chunk])"""
    out = []
    for s, (p, n) in enumerate(zip(PREFIXES, CHUNKS[kind])):
        ids = np.random.default_rng(1000 * p + 10 * n + s).integers(3, 1000, p + n)
        out.append((lm._w["embed"][torch.from_numpy(ids).cuda()],
                    np.broadcast_to(np.arange(p + n, dtype=np.int64)[None], (3, p + n)).copy()))
    return out


@pytest.fixture(scope="module")
def tiny():
    cfg = oq.tiny_cfg()
    W = oq.random_weights(cfg, seed=1234, dtype=BF, std=0.05, embed_std=0.2)
    lm = build_product_model(cfg, W, kv_pool_tokens=8192, max_seqs=24).language_model
    lm._rope_deltas = np.zeros((1, 1), dtype=np.int64)
    return lm


@pytest.fixture(scope="module")
def one_shot(tiny):
    """(chunks, 8-bit) -> (last-row logits, next-step logits) per sequence, each from ITS OWN one-shot prefill"""
    lm, refs = tiny, {}
    for kind in CHUNKS:
        for q8 in (False, True):
            last, nxt = [], []
            for emb, pos in _inputs(lm, kind):
                c = lm.make_cache()
                last.append(lm.prefill(emb.clone(), pos, [c], [emb.shape[0]], "last")[0].clone())
                if q8:
                    lm.quantize_kv([c[0]._seq], bits=8, group_size=64)
                nxt.append(lm(np.array([[NEXT_TOKEN]]), cache=c).logits[0, -1].clone())
                c[0]._seq.release()
            refs[kind, q8] = (last, nxt)
    return refs


@pytest.mark.parametrize("route", list(ROUTES))
def test_two_sequences_with_different_cache_lengths_in_one_call(tiny, one_shot, monkeypatch, route):
    lm = tiny
    paged_attn, q8, kind, env, attn_op, bar = ROUTES[route]
    for k in ("VLM_ONTO_CACHE_DECODE_ATTN", "VLM_ONTO_CACHE_QSTART"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    chunks = CHUNKS[kind]
    want, want_next = one_shot[kind, q8]
    inputs = _inputs(lm, kind)
    caches = lm.make_cache_batch(2)
    seqs = [c[0]._seq for c in caches]
    try:
        for c, p, n, (emb, pos) in zip(caches, PREFIXES, chunks, inputs):
            lm.prefill(emb[:p].clone(), pos[:, :p], [c], [p], "last", reserve_extra=n + 4)
        if q8:
            lm.quantize_kv(seqs, bits=8, group_size=64)
        calls = dict.fromkeys(ATTN_OPS, 0)
        for name in ATTN_OPS:
            def spy(*a, _name=name, _real=getattr(ops, name), **k):
                calls[_name] += 1
                return _real(*a, **k)
            monkeypatch.setattr(ops, name, spy)
        emb = torch.cat([e[p:] for p, (e, _) in zip(PREFIXES, inputs)]).contiguous()
        pos = np.concatenate([q[:, p:] for p, (_, q) in zip(PREFIXES, inputs)], axis=1)
        got = lm.prefill(emb, pos, caches, list(chunks), "last", reserve_extra=4, paged_attn=paged_attn)
        assert calls == {**dict.fromkeys(ATTN_OPS, 0), attn_op: lm.args.num_hidden_layers}, calls
        monkeypatch.undo()
        assert got.shape[0] == 2 and [s.offset for s in seqs] == [p + n for p, n in zip(PREFIXES, chunks)]
        assert [bool(s.q8) for s in seqs] == [q8, q8]
        for s in range(2):
            e = _rel_rms(got[s], want[s])
            print(f"{route}: sequence {s} (cache {PREFIXES[s]} + chunk {chunks[s]}) last row {e:.5f}")
            assert e < bar, (route, s, e)
        for s in range(2):
            e = _rel_rms(lm(np.array([[NEXT_TOKEN]]), cache=caches[s]).logits[0, -1], want_next[s])
            print(f"{route}: sequence {s} next step {e:.5f}")
            assert e < bar, (route, s, "next step", e)
            assert seqs[s].offset == PREFIXES[s] + chunks[s] + 1
    finally:
        for s in seqs:
            s.release()
