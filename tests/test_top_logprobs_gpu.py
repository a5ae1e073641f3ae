"""top_logprobs on MI355X: the selection kernel (csrc/top_logprobs.hip through vlm_sample_ex(input_is_logprobs=2),
ops.top_logprobs) and `BatchGenerator(top_logprobs_k=k)` end to end.

The operator is a SELECTION: indices must be equal to the restatement of the reference's order (ar.py:1114-1116,
torch.argsort(stable) ascending, the last k, reversed; pinned to the reference's own lines in tests/test_top_logprobs_cpu.py)
and values bit-equal - no tolerance.  The reference of a shape is computed once for K = 64 and shared: the order is total,
so the list for k is the first k entries of it."""
import functools

import numpy as np
import pytest
import torch

from oracle import ops as O
from oracle import qwen2_vl as oq
from tests.helpers import bf16_close, build_product_model, synth_request

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SHAPES = [(1, 1000, 1024), (3, 32003, 32008), (16, 151936, 151936), (64, 151936, 151936)]      # (B, V, ld)
KS = [1, 2, 5, 20, 64]


def restatement(lp, k):
    idx = torch.argsort(lp.float(), dim=-1, stable=True)[..., -k:].flip(-1)
    return idx.to(torch.int32), torch.take_along_dim(lp, idx, dim=-1)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _padded(rows, ld):
    """rows bf16 [B, V] (CPU) -> the device tensor the kernel sees: a [B, V] view of [B, ld] storage, NaN between V and ld"""
    B, V = rows.shape
    buf = torch.full((B, ld), float("nan"), dtype=BF)
    buf[:, :V] = rows
    dev = buf.cuda()
    return dev, dev[:, :V]


@functools.lru_cache(maxsize=None)
def _random_case(B, V, ld):
    """log-probs of N(0, 2^2) logits (a bf16 row of 151,936 holds ~235 distinct values: ties everywhere) + the K = 64 answer"""
    # (B = 64: the first seed of this family in which EVERY row ends its K = 64 list inside a tie, see the test)
    g = torch.Generator().manual_seed(1000 * B + V % 997 + (5 * 7919 if B == 64 else 0))
    x = torch.randn(B, V, generator=g) * 2.0
    lp = (x - torch.logsumexp(x, -1, keepdim=True)).to(BF)
    return lp, restatement(lp, min(64, V))


class _SamplerProbe:
    """A greedy and a sampled (top-p 0.9 + top-k) ops.sample call on fixed logits over ONE workspace: recorded before the first
    top_logprobs call, repeated on the same workspace after every one - the operator is handed that workspace and must leave
    it as vlm_sample expects (histogram all zero, control words re-armed)."""

    def __init__(self):
        from mlx_vlm_amd import ops
        g = torch.Generator().manual_seed(77)
        self.logits = (torch.randn(4, 151936, generator=g) * 2.0).to(BF).cuda()
        self.step = torch.full((1,), 5, dtype=torch.int32, device="cuda")
        self.ws = ops.sample_workspace(64, "cuda")
        self.want = self.tokens()
        self.ws_bytes = self.ws.clone()

    def tokens(self):
        from mlx_vlm_amd import ops
        a, _ = ops.sample(self.logits, temperature=0.0, want_logprobs=False, ws=self.ws)
        b, _ = ops.sample(self.logits, temperature=0.8, top_p=0.9, top_k=40, seed=3, step=self.step, want_logprobs=False, ws=self.ws)
        return a.tolist(), b.tolist()

    def check(self):
        assert torch.equal(self.ws, self.ws_bytes)            # not a byte of it moved ...
        assert self.tokens() == self.want                     # ... and the sampler finds what it expects


@pytest.fixture(scope="module")
def probe():
    return _SamplerProbe()


def _select(probe, rows, ld, k):
    """one operator call on `rows` (CPU bf16 [B, V]) laid out with pitch ld; checks the input and the sampler workspace after it"""
    from mlx_vlm_amd import ops
    store, view = _padded(rows, ld)
    before = _bits(store).clone()
    idx, val = ops.top_logprobs(view, k, ws=probe.ws)
    torch.cuda.synchronize()
    assert idx.dtype == torch.int32 and val.dtype == BF and tuple(idx.shape) == tuple(val.shape) == (rows.shape[0], k)
    assert torch.equal(_bits(store), before)                  # the rows - and the padding - are byte-identical
    probe.check()
    return idx.cpu(), val.cpu()


def _assert_is(idx, val, want_idx, want_val):
    assert torch.equal(idx, want_idx), (idx[(idx != want_idx).any(-1)][:2], want_idx[(idx != want_idx).any(-1)][:2])
    assert torch.equal(_bits(val), _bits(want_val))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("B,V,ld", SHAPES)
def test_operator_random_rows_equal_the_restatement(probe, B, V, ld, k):
    lp, (ref_idx, ref_val) = _random_case(B, V, ld)
    if k == 64 and V == 151936:      # the data holds what the case is for: in EVERY row the K-th value is shared (2 .. 10
        at_kth = (lp == ref_val[:, -1:]).sum(-1)      # elements equal it in these rows, 4 in the median), so every list ends inside a tie
        assert int(at_kth.min()) >= 2, at_kth.tolist()
    idx, val = _select(probe, lp, ld, k)
    _assert_is(idx, val, ref_idx[:, :k].contiguous(), ref_val[:, :k].contiguous())


def _special_rows(V):
    """name -> (row bf16 [V], k, expected indices or None = the restatement decides)"""
    g = torch.Generator().manual_seed(V)
    base = (-torch.rand(V, generator=g) * 6.0 - 4.0).to(BF)          # negatives in [-10, -4]
    out = {}
    out["all_equal"] = (torch.full((V,), -11.9375, dtype=BF), 64, list(range(V - 1, V - 65, -1)))
    ninf = torch.full((V,), float("-inf"), dtype=BF)
    ninf[[3, V // 2, V - 2]] = torch.tensor([-2.0, -0.5, -2.0], dtype=BF)
    out["three_finite_in_minus_inf"] = (ninf, 5, [V // 2, V - 2, 3, V - 1, V - 3])
    z = base.clone()
    z[7], z[900] = 0.0, -0.0
    out["signed_zeros"] = (z, 2, [900, 7])
    if V >= 4000:
        # 1,900 tokens share the crossing value, 10 lie above it: k = 20 takes the 10 HIGHEST indices of the 1,900
        t = base.clone()
        perm = torch.randperm(V, generator=g)
        t[perm[:1900]] = -3.0
        t[perm[1900:1910]] = torch.linspace(-2.5, -0.25, 10).to(BF)
        out["1900_share_the_crossing_value"] = (t, 20, None)
        out["1900_share_the_crossing_value_k64"] = (t, 64, None)
    if V >= 100000:
        # every large value sits in 16-byte chunks c with c % 64 < 2 - two of the kernel's 64 lane groups - so the bound it takes
        # from the groups' maxima lets ~V / 32 = 4,748 elements through: more than its LDS list holds, the select runs over the row
        a = (base.float() - 20.0).to(BF)
        i = torch.arange(V)
        hot = ((i // 8) % 64) < 2
        a[hot] = (-torch.rand(int(hot.sum()), generator=g) * 3.0 - 0.5).to(BF)
        out["large_values_in_two_lane_groups"] = (a, 64, None)
        out["large_values_in_two_lane_groups_k5"] = (a, 5, None)
    return out


@pytest.mark.parametrize("V,ld", [(1000, 1024), (32003, 32008), (32003, 32005), (151936, 151936)])
def test_operator_special_rows(probe, V, ld):
    """all-equal, -inf with 3 finite entries, +0.0 / -0.0, 1,900 ties at the crossing value, a row laid out against the
    kernel's thread assignment; ld = 32005 puts rows 1.. off the 16-byte alignment (the one-element-per-lane passes)."""
    cases = _special_rows(V)
    for k in sorted({c[1] for c in cases.values()}):
        names = [n for n, c in cases.items() if c[1] == k]
        rows = torch.stack([cases[n][0] for n in names])
        idx, val = _select(probe, rows, ld, k)
        want_idx, want_val = restatement(rows, k)
        _assert_is(idx, val, want_idx, want_val)
        for r, n in enumerate(names):
            if cases[n][2] is not None:
                assert idx[r].tolist() == cases[n][2], n
            if n == "signed_zeros":
                assert _bits(val)[r].tolist() == [-32768, 0]          # each zero keeps its own bits


def test_operator_refuses_k_outside_the_built_range():
    from mlx_vlm_amd import ops
    lp = torch.zeros(2, 100, dtype=BF, device="cuda")
    with pytest.raises(NotImplementedError, match="64"):
        ops.top_logprobs(lp, 65)
    with pytest.raises(ValueError):
        ops.top_logprobs(lp, 0)
    with pytest.raises(ValueError):
        ops.top_logprobs(lp[:, :40], 41)
    idx, _ = ops.top_logprobs(lp[:, :40], 40)                          # k == V: the whole row, highest index first
    assert idx.cpu()[1].tolist() == list(range(39, -1, -1))


# ------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def peaked():
    """the tiny Qwen2-VL of the batch tests in tests/test_engine_gpu.py (oracle.qwen2_vl.tiny_cfg, weights seed 1234) with the
    peaked head of tests/test_parity_decode_gpu.py: greedy decoding walks a cycle, no near-ties at the top of a row"""
    cfg = oq.tiny_cfg()
    cfg.text.tie_word_embeddings = False
    W = oq.random_weights(cfg, seed=1234, dtype=BF, std=0.05, embed_std=0.2)
    for k in list(W):
        if k.endswith("o_proj.weight") or k.endswith("down_proj.weight"):
            W[k] = (W[k].float() * 0.5).to(BF)
    W = oq.peak_head(W, cfg, gamma=4.0, stride=389, n_cycle=1000)
    model = build_product_model(cfg, W, kv_pool_tokens=32768, max_seqs=80)
    return cfg, W, model


def _requests(cfg, n, seed0=700):
    """text requests of different lengths; request 1 carries an image"""
    reqs = []
    for i in range(n):
        if i == 1:
            reqs.append(synth_request(cfg, [(56, 84)], n_text=7, seed=seed0 + i))
        else:
            reqs.append((np.random.default_rng(seed0 + i).integers(3, 1000, (1, 5 + 3 * (i % 7))), None, None))
    return reqs


MAX_TOKENS = [5, 9, 3, 7, 11, 4]


def _run(model, reqs, max_tokens, k, rows=4, processors=None, **kw):
    """-> (the Responses of every request, the step widths seen).  async_prefill=False unless asked for: the round at which
    a request joins is then a function of the requests alone, so two runs step the same rows at the same widths and their
    log-prob rows can be compared bit for bit (steps of different widths sum in different orders)."""
    from mlx_vlm_amd.batch import BatchGenerator

    kw.setdefault("async_prefill", False)
    gen = BatchGenerator(model, None, max_tokens=8, completion_batch_size=rows, prefill_batch_size=min(rows, 8), top_logprobs_k=k, **kw)
    pk = [dict(pixel_values=torch.from_numpy(p), image_grid_thw=g) if p is not None else {} for _, p, g in reqs]
    uids = gen.insert([r[0].reshape(-1) for r in reqs], list(max_tokens), prompt_kwargs=pk, logits_processors=processors)
    got = {u: [] for u in uids}
    widths = set()
    while gen.has_work:
        _, out = gen.next()
        widths.add(gen._width)
        for r in out:
            got[r.uid].append(r)
    gen.close()
    assert all(len(got[u]) == m for u, m in zip(uids, max_tokens))
    return [got[u] for u in uids], widths


def _tokens(run):
    return [[r.token for r in rs] for rs in run]


def _lists(run):
    return [[r.top_logprobs for r in rs] for rs in run]


def _check_lists(run, k, greedy=True, token_logprob=True):
    for rs in run:
        for r in rs:
            top = r.top_logprobs
            assert isinstance(top, list) and len(top) == k
            assert all(isinstance(t, int) and isinstance(v, float) for t, v in top)
            vals = [v for _, v in top]
            assert all(a >= b for a, b in zip(vals, vals[1:])), vals
            if greedy:
                assert top[0][0] == r.token                      # (the peaked head: no tie at the top of a row)
                if token_logprob:
                    assert top[0][1] == r.token_logprob
            if not token_logprob:
                assert r.token_logprob == 0.0


@pytest.fixture(scope="module")
def graph_runs(peaked):
    cfg, W, model = peaked
    reqs = _requests(cfg, 6)
    base, _ = _run(model, reqs, MAX_TOKENS, 0)
    assert all(r.top_logprobs is None for rs in base for r in rs)
    with5, widths = _run(model, reqs, MAX_TOKENS, 5)
    assert widths >= {1, 4}                       # full steps, rows that leave and are refilled, the tail of the queue
    # admissions on the side stream (the default): the first tokens' lists are selected there and join with their rows
    side, _ = _run(model, reqs, MAX_TOKENS, 5, async_prefill=True)
    assert _tokens(side) == _tokens(base)
    _check_lists(side, 5)
    return reqs, base, with5


def test_batch_generator_graph_steps_report_the_lists(graph_runs):
    _, base, with5 = graph_runs
    assert _tokens(with5) == _tokens(base)
    assert [[r.token_logprob for r in rs] for rs in with5] == [[r.token_logprob for r in rs] for rs in base]
    _check_lists(with5, 5)


def test_batch_generator_eager_steps_report_the_same_lists(peaked, graph_runs):
    cfg, W, model = peaked
    reqs, base, with5 = graph_runs
    base_e, _ = _run(model, reqs, MAX_TOKENS, 0, use_graph=False)
    eager, _ = _run(model, reqs, MAX_TOKENS, 5, use_graph=False)
    assert _tokens(eager) == _tokens(base_e) == _tokens(base)
    _check_lists(eager, 5)
    assert _lists(eager) == _lists(with5)


def test_batch_generator_python_processor_takes_the_eager_path_with_the_lists(peaked, graph_runs):
    cfg, W, model = peaked
    reqs, base, with5 = graph_runs
    calls = []

    def passthrough(tokens, logits):
        calls.append(int(tokens.numel()))
        return logits

    procs = [None, None, [passthrough], None, None, None]
    base_p, _ = _run(model, reqs, MAX_TOKENS, 0, processors=procs)
    n0 = len(calls)
    run, _ = _run(model, reqs, MAX_TOKENS, 5, processors=procs)
    assert n0 >= MAX_TOKENS[2] and len(calls) == 2 * n0          # it ran: on the first token and on every step of its row
    assert _tokens(run) == _tokens(base_p) == _tokens(base)
    _check_lists(run, 5)


def test_batch_generator_without_token_logprobs_still_reports_the_lists(peaked, graph_runs):
    cfg, W, model = peaked
    reqs, base, with5 = graph_runs
    base_n, _ = _run(model, reqs, MAX_TOKENS, 0, compute_logprobs=False)
    run, _ = _run(model, reqs, MAX_TOKENS, 5, compute_logprobs=False)
    assert _tokens(run) == _tokens(base_n) == _tokens(base)
    _check_lists(run, 5, token_logprob=False)
    assert _lists(run) == _lists(with5)


def test_batch_generator_lists_match_the_oracle(peaked, graph_runs):
    """teacher-forced oracle over the engine's own tokens: every reported value within the step bar of the engine tests
    (2 bf16 ulps + 3 % of the rms) of the oracle's log-prob at the reported index, and the oracle's argmax is the first index"""
    cfg, W, model = peaked
    reqs, base, with5 = graph_runs
    for (ids, pix, thw), rs in zip(reqs, with5):
        toks = [r.token for r in rs]
        ref = oq.decode_teacher_forced(W, cfg, ids, torch.from_numpy(pix).to(BF) if pix is not None else None, thw, toks[:-1])
        ref_lp = O.logprobs_from_logits(ref)
        assert ref_lp.shape[0] == len(rs)
        idx = torch.tensor([[t for t, _ in r.top_logprobs] for r in rs])
        val = torch.tensor([[v for _, v in r.top_logprobs] for r in rs])
        want = torch.take_along_dim(ref_lp.float(), idx, dim=-1)
        ok, rep = bf16_close(val, want, ulps=2, atol_rms=3e-2)
        print(f"lists vs oracle: {rep}")
        assert ok, rep
        assert ref_lp.float().argmax(-1).tolist() == idx[:, 0].tolist()


def test_batch_generator_processors_run_before_the_selection(peaked, graph_runs):
    from mlx_vlm_amd.sample_utils import make_logits_processors

    cfg, W, model = peaked
    reqs, base, with5 = graph_runs
    u = 3
    t = with5[u][1].token                              # the unbiased run puts it first in the list of its second token
    assert with5[u][1].top_logprobs[0][0] == t
    procs = [None] * 6
    procs[u] = make_logits_processors(logit_bias={t: -100.0})
    run, _ = _run(model, reqs, MAX_TOKENS, 5, processors=procs)
    _check_lists(run, 5)
    assert all(t not in [i for i, _ in r.top_logprobs] for r in run[u])
    assert _lists(run)[:u] == _lists(with5)[:u]        # the other requests are untouched


def test_batch_generator_wide_buffers_and_wide_steps(peaked):
    """completion_batch_size = 32.  (a) 3 SAMPLED requests (temperature 0.8, top-p 0.9: the same rows, steps and noise in
    both generators) give through the 32-row generator - list buffers [32][k], pinned [2][32][k] - exactly the lists they
    give through 4 rows.  (b) 20 greedy requests keep 17+ rows live: the 32-wide steps run the prefill GEMMs, another
    summation order than the 4-row steps, so what is demanded of their lists is what no rounding can move: k pairs, ordered,
    the token first with its own log-prob."""
    from mlx_vlm_amd.sample_utils import make_sampler

    cfg, W, model = peaked
    reqs = _requests(cfg, 3, seed0=810)
    mt = [6, 4, 8]
    smp = dict(sampler=make_sampler(temp=0.8, top_p=0.9, seed=11))
    wide, _ = _run(model, reqs, mt, 5, rows=32, **smp)
    narrow, _ = _run(model, reqs, mt, 5, rows=4, **smp)
    assert _tokens(wide) == _tokens(narrow)
    _check_lists(wide, 5, greedy=False)
    assert _lists(wide) == _lists(narrow)
    many = _requests(cfg, 20, seed0=830)
    run, widths = _run(model, many, [4 + i % 5 for i in range(20)], 5, rows=32)
    assert 32 in widths
    _check_lists(run, 5)
