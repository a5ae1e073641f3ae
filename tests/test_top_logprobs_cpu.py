"""top_logprobs_k of the batch generator (reference mlx_vlm/generate/ar.py:1092-1122, 2051-2058, 1324-1334), the parts that
need no GPU:

  * the restatement of the reference's order that the GPU tests hold the kernel to - torch.argsort(stable) ascending, the last
    k, reversed: value descending and the HIGHER index first among equal values - against the reference's own three lines
    executed over oracle/mlx_shim and against a brute-force sort by (-value, -index);
  * the scheduler's side of `BatchGenerator(top_logprobs_k=k)` with a mock engine whose lists are a known function of
    (uid, token index): every Response carries its own request's list whatever the rows did meanwhile;
  * the keyword's validation and the header's statement of the mode."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from mlx_vlm_amd.batch import BatchGenerator
from mlx_vlm_amd.models.cache import KVPool, PagedSequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


def restatement(lp, k):
    """-> (indices int32 [..., k], values in lp's dtype): what the GPU tests compare the kernel with"""
    idx = torch.argsort(lp.float(), dim=-1, stable=True)[..., -k:].flip(-1)
    return idx.to(torch.int32), torch.take_along_dim(lp, idx, dim=-1)


def _rows():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4001, generator=g) * 2.0
    rnd = (x - torch.logsumexp(x, -1)).to(BF)                    # ~150 distinct values: ties inside and at the edge of the list
    equal = torch.full((300,), -5.25, dtype=BF)
    ninf = torch.full((300,), float("-inf"), dtype=BF)
    ninf[[17, 170, 299]] = torch.tensor([-1.5, -0.25, -1.5], dtype=BF)
    zeros = -torch.rand(1000, generator=g).to(BF) - 0.5
    zeros[7], zeros[900] = 0.0, -0.0
    return {"random": rnd, "all_equal": equal, "three_finite": ninf, "signed_zeros": zeros}


@pytest.mark.parametrize("name", ["random", "all_equal", "three_finite", "signed_zeros"])
@pytest.mark.parametrize("k", [1, 2, 5, 20, 64])
def test_restatement_is_the_references_expression_and_the_brute_force_order(name, k):
    lp = _rows()[name]
    idx, val = restatement(lp[None], k)
    # the reference's lines (ar.py:1114-1116) over the shim.  (The shim's indexing takes no negative step: the reversal
    # `[..., ::-1]` is a flip of the sliced array's tensor.)
    sys.path.insert(0, os.path.join(ROOT, "oracle", "mlx_shim"))
    try:
        import mlx.core as mx
    finally:
        sys.path.pop(0)
    logprobs = mx.array(lp[None])
    sort_idx = mx.argsort(logprobs, axis=-1)
    top_idx = mx.array(sort_idx[..., -k:]._t.flip(-1)).astype(mx.int32)
    top_lp = mx.take_along_axis(logprobs, top_idx, axis=-1)
    assert top_idx._t.dtype == torch.int32 and top_lp._t.dtype == BF
    assert torch.equal(top_idx._t, idx)
    assert torch.equal(top_lp._t.view(torch.int16), val.view(torch.int16))
    # brute force: sort the (value, index) pairs by value descending, then index descending
    v = lp.float().tolist()
    order = sorted(range(len(v)), key=lambda i: (-v[i], -i))[:k]
    assert idx[0].tolist() == order
    assert val[0].float().tolist() == [v[i] for i in order]


def test_restatement_edge_rows_read_as_the_issue_states_them():
    r = _rows()
    assert restatement(r["all_equal"][None], 5)[0][0].tolist() == [299, 298, 297, 296, 295]
    assert restatement(r["signed_zeros"][None], 2)[0][0].tolist() == [900, 7]          # +0.0 == -0.0: the index decides
    i, v = restatement(r["signed_zeros"][None], 2)
    assert v.view(torch.int16)[0].tolist() == [-32768, 0]                              # ... and each keeps its own bits
    assert restatement(r["three_finite"][None], 5)[0][0].tolist() == [170, 299, 17, 298, 297]


# ------------------------------------------------------------------------------------------ scheduler, mock engine
V = 5003
K = 3


def first_token(ids):
    return int((int(np.sum(ids)) * 31 + len(ids)) % V)


def next_token(tok, ctx, pos):
    return int((tok * 7 + ctx * 13 + pos * 3 + 1) % V)


def top_of(uid, j, k=K):
    """the mock engine's list of request `uid`'s token number j"""
    return [((uid * 131 + j * 17 + c) % V, -(uid + 1) * 0.5 - j * 0.125 - c) for c in range(k)]


class MockTopEngine(BatchGenerator):
    """BatchGenerator with the engine hooks replaced (as tests/test_batch_scheduler_cpu.py does) - the three hooks of
    top_logprobs_k included: they return `top_of(uid, token index)`."""

    def __init__(self, pool, **kw):
        self.sampled = {}          # uid -> tokens sampled so far (the next list's token index)
        self.top_calls = 0
        lm = SimpleNamespace(device="cpu", pool=pool)
        super().__init__(SimpleNamespace(language_model=lm), None, **kw)

    def _new_decode_state(self, cap):
        z = lambda: torch.zeros(cap, dtype=torch.int32)  # noqa: E731
        return SimpleNamespace(B=cap, tok=z(), pos=z(), ctx=z(), step=torch.zeros(1, dtype=torch.int32), nsplit=1,
                               last_lp=torch.zeros(cap))

    def _prefill_requests(self, batch):
        caches, lens, toks = [], [], []
        for uid, ids, max_tokens, kw in batch:
            seq = PagedSequence(self.lm.pool)
            seq.reserve(len(ids) + max_tokens + 2)
            seq.offset = len(ids)
            caches.append([SimpleNamespace(_seq=seq)])
            lens.append(len(ids))
            toks.append(first_token(ids))
        tok0 = torch.tensor(toks, dtype=torch.int32)
        lp0 = -tok0.float() / V if self.compute_logprobs else None
        ctx = np.asarray(lens, dtype=np.int32)
        return caches, lens, tok0, lp0, torch.from_numpy(np.stack([ctx, ctx]))

    def _decode_rows(self, width):
        st = self._st
        for r in range(width):
            st.tok[r] = next_token(int(st.tok[r]), int(st.ctx[r]), int(st.pos[r]))
            st.last_lp[r] = -float(st.tok[r]) / V
        st.ctx[:width] += 1
        st.pos[:width] += 1

    def _row_logprobs(self, n):
        return self._st.last_lp[:n].clone()

    # ---- the new hooks
    def _new_top_buffers(self, cap, k):
        return torch.full((cap, k), -1, dtype=torch.int32), torch.zeros(cap, k, dtype=torch.float32)

    def _lists(self, uids):
        self.top_calls += 1
        idx = torch.tensor([[p[0] for p in top_of(u, self.sampled.get(u, 0), self.top_logprobs_k)] for u in uids], dtype=torch.int32)
        val = torch.tensor([[p[1] for p in top_of(u, self.sampled.get(u, 0), self.top_logprobs_k)] for u in uids], dtype=torch.float32)
        for u in uids:
            self.sampled[u] = self.sampled.get(u, 0) + 1
        return idx, val

    def _prefill_top_logprobs(self, batch):
        return self._lists([b[0] for b in batch])

    def _step_top_logprobs(self, n):
        idx, val = self._lists([row.uid for row in self._rows[:n]])
        self._top_idx[:n].copy_(idx)
        self._top_val[:n].copy_(val)


def make_pool():
    return KVPool(n_layers=1, n_kv_heads=1, head_dim=128, max_tokens=64 * 64, max_seqs=16, device="cpu", layout="paged")


def _requests():
    rng = np.random.default_rng(3)
    prompts = [rng.integers(1, 999, int(rng.integers(3, 30))) for _ in range(6)]
    return prompts, [2, 9, 1, 5, 12, 4]


@pytest.mark.parametrize("ahead", [0, 2])
def test_every_response_carries_its_own_requests_list(ahead):
    """6 requests of different max_tokens through 4 rows: joins (the first token's list comes from the admission), rows that
    finish at different steps with the last row moved into the hole, a request removed while a step is in flight, and the
    two pinned slots taking turns.  Every Response - the FIRST token of a request included - carries exactly K pairs, and
    they are the list of its own uid and token index."""
    pool = make_pool()
    free_pages = len(pool._free_pages)
    prompts, max_tokens = _requests()
    gen = MockTopEngine(pool, completion_batch_size=4, prefill_batch_size=2, prefill_ahead=ahead, top_logprobs_k=K)
    uids = gen.insert(prompts, max_tokens)
    got = {u: [] for u in uids}
    removed, rounds = None, 0
    while gen.has_work:
        _, out = gen.next()
        rounds += 1
        assert rounds < 200
        for r in out:
            assert isinstance(r.top_logprobs, list) and len(r.top_logprobs) == K
            assert all(isinstance(t, int) and isinstance(v, float) for t, v in r.top_logprobs)
            want = top_of(r.uid, len(got[r.uid]))
            assert [t for t, _ in r.top_logprobs] == [t for t, _ in want], (r.uid, len(got[r.uid]))
            np.testing.assert_allclose([v for _, v in r.top_logprobs], [v for _, v in want], rtol=1e-6)
            got[r.uid].append(r.token)
        if removed is None and len(got[uids[4]]) == 3:
            removed = uids[4]                       # a step over its row is in flight: its results must be dropped, not misfiled
            assert gen.remove(removed)
    assert removed is not None
    for u, m in zip(uids, max_tokens):
        assert len(got[u]) == (3 if u == removed else m), (u, got[u])
    gen.close()
    assert len(pool._free_pages) == free_pages


def test_k_zero_reports_none_and_calls_no_new_hook():
    pool = make_pool()
    prompts, max_tokens = _requests()
    for kw in ({}, {"top_logprobs_k": 0}, {"top_logprobs_k": None}):
        gen = MockTopEngine(pool, completion_batch_size=4, prefill_batch_size=2, **kw)
        assert gen.top_logprobs_k == 0 and not hasattr(gen, "_top_idx") and not hasattr(gen, "_pin_top_idx")
        gen.insert(prompts, max_tokens)
        n = 0
        while gen.has_work:
            _, out = gen.next()
            for r in out:
                assert r.top_logprobs is None
                n += 1
        assert n == sum(max_tokens) and gen.top_calls == 0
        gen.close()


def test_compute_logprobs_false_still_reports_zero_and_the_lists():
    pool = make_pool()
    prompts, max_tokens = _requests()
    gen = MockTopEngine(pool, completion_batch_size=4, prefill_batch_size=4, compute_logprobs=False, top_logprobs_k=K)
    gen.insert(prompts, max_tokens)
    seen = {}
    while gen.has_work:
        _, out = gen.next()
        for r in out:
            assert r.token_logprob == 0.0
            assert [t for t, _ in r.top_logprobs] == [t for t, _ in top_of(r.uid, seen.get(r.uid, 0))]
            seen[r.uid] = seen.get(r.uid, 0) + 1
    gen.close()


def test_keyword_validation():
    pool = make_pool()
    with pytest.raises(NotImplementedError, match="64"):
        MockTopEngine(pool, top_logprobs_k=65)
    with pytest.raises(ValueError):
        MockTopEngine(pool, top_logprobs_k=-1)
    with pytest.raises(TypeError):
        MockTopEngine(pool, top_logprobs_k=2.5)
    with pytest.raises(TypeError):
        MockTopEngine(pool, top_logprobs_k=True)
    gen = MockTopEngine(pool, top_logprobs_k=64)
    assert gen.top_logprobs_k == 64
    gen.close()


def test_header_documents_the_mode():
    hdr = open(os.path.join(ROOT, "include", "vlm_hip.h")).read()
    at = hdr.index("input_is_logprobs == 2")
    doc = hdr[at:hdr.index("typedef struct vlm_sampler_params", at)]
    for word in ("added within ABI v8", "top_k = K", "int32 [B][K]", "bf16 [B][K]", "HIGHER index first", "min(64, V)", "+0.0 and -0.0"):
        assert word in doc, word


def test_an_engine_that_replaces_the_prefill_hook_alone_is_told_so():
    """`_prefill_top_logprobs` reads the rows `_prefill_requests` leaves behind: an engine that overrides only the latter gets
    an error that names the contract, not a failure inside the operator"""
    class Half(MockTopEngine):
        _prefill_top_logprobs = BatchGenerator._prefill_top_logprobs

    pool = make_pool()
    gen = Half(pool, completion_batch_size=2, top_logprobs_k=K)
    gen.insert([np.arange(1, 6)], [3])
    with pytest.raises(RuntimeError, match="_last_lp_rows"):
        gen.next()
