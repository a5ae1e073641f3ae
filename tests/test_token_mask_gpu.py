"""Constrained decoding on MI355X: the token-bitmask kernel behind vlm_apply_logit_penalties (csrc/sample.hip::
token_mask_kernel), every sampler form over the rows it leaves, and the mask protocol end to end on captured steps.

Operator level there is no tolerance: an allowed logit keeps its bits, every other one is 0xFF80, nothing at or past V is
written.  The sampler forms are held to tests/sampler_exact.py (log-prob rows bit-identical to exact_logprobs, the draw equal
to exact_draw's winner over the kernel's own filtered row), on inputs whose logsumexp keeps the guard band.  End to end the
captured route equals the same constraint written as a plain callable on the eager route, bit for bit."""
import functools

import numpy as np
import pytest
import torch

from oracle import qwen2_vl as oq
from tests import sampler_exact as S
from tests.helpers import build_product_model, synth_request
from tests.test_top_logprobs_gpu import restatement

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = "cuda"
NINF_BITS = np.int16(-128)                                   # 0xFF80
SHAPES = [(1, 1000, 1024), (3, 32003, 32008), (16, 151936, 151936), (64, 151936, 151936)]      # (B, V, ld)
CASES = ["half", "twenty", "one_in_last_word", "short_w", "w0_interleaved", "with_penalties", "unaligned_rows"]


def words_of(V):
    return (V + 31) // 32


def pack(allowed, n_words):
    """allowed bool [32 * n_words] (or shorter) -> int32 [n_words]"""
    a = np.zeros(32 * n_words, dtype=bool)
    a[:min(len(allowed), len(a))] = allowed[:len(a)]
    return np.packbits(a.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1).view(np.int32)


def unpack(words, V):
    """the rule of the header: t is allowed iff t < 32 * W and bit t & 31 of word t >> 5 is set"""
    bits = np.unpackbits(np.asarray(words).view(np.uint8), bitorder="little").astype(bool) if len(words) else np.zeros(0, dtype=bool)
    out = np.zeros(V, dtype=bool)
    out[:min(V, len(bits))] = bits[:V]
    return out


def test_pack_and_unpack_state_the_rule():
    w = pack(np.isin(np.arange(100), [0, 31, 32, 99]), 4)
    assert w.view(np.uint32).tolist() == [0x80000001, 1, 0, 8] and unpack(w, 100).nonzero()[0].tolist() == [0, 31, 32, 99]
    assert unpack(w[:1], 100).nonzero()[0].tolist() == [0, 31] and not unpack(w[:0], 100).any()


@functools.lru_cache(maxsize=None)
def _logits(B, V, ld):
    """bf16 [B, ld] storage, N(0, 3^2) in the first V columns, NaN between V and ld"""
    g = torch.Generator().manual_seed(B * 7919 + V)
    buf = torch.full((B, ld), float("nan"), dtype=BF)
    buf[:, :V] = (torch.randn(B, V, generator=g) * 3.0).to(BF)
    return buf


def _masks(case, B, V):
    """-> per row: None (W = 0) or the int32 words of its mask"""
    MW, rng = words_of(V), np.random.default_rng(B * 31 + V + len(case))
    out = []
    for b in range(B):
        if case in ("half", "with_penalties", "unaligned_rows"):
            out.append(pack(rng.random(32 * MW) < 0.5, MW))
        elif case == "twenty":
            out.append(pack(np.isin(np.arange(32 * MW), rng.integers(0, V, 20)), MW))
        elif case == "one_in_last_word":                        # the last word of the row: partial wherever V % 32 != 0
            t = int(rng.integers(32 * (MW - 1), V))
            out.append(pack(np.arange(32 * MW) == t, MW))
        elif case == "short_w":                                 # W_b < ceil(V / 32): the tokens past the mask are disallowed
            n = max(1, MW - 1 - 7 * b)
            out.append(pack(rng.random(32 * n) < 0.5, n))
        elif case == "w0_interleaved":                          # even rows carry no mask (B = 1: the untouched row alone)
            out.append(pack(rng.random(32 * MW) < 0.5, MW) if b % 2 else None)
    return out


def _tables(B, V, masks, specs=None, hist=None):
    """the per-row form of vlm_penalty_args over fresh device tables -> (PenaltyArgs, what keeps it alive)"""
    from mlx_vlm_amd import _lib
    from mlx_vlm_amd.models.qwen2_vl.language import DecodeState

    cap = 32
    params, bidx, bval = DecodeState.pack_row_penalties(specs or [None] * B, cap, words_of(V), masks)
    h = np.zeros((B, cap), dtype=np.int32)
    n = np.zeros(B, dtype=np.int32)
    for b, t in enumerate(hist or []):
        h[b, :len(t)], n[b] = t, len(t)
    keep = [torch.from_numpy(a).to(DEV) for a in (h, n, params, bidx, bval)]
    pa = _lib.PenaltyArgs(keep[0].data_ptr(), keep[1].data_ptr(), cap, 0.0, 0, 0.0, 0, 0.0, 0, keep[3].data_ptr(), keep[4].data_ptr(), 0,
                          keep[2].data_ptr(), bidx.shape[1])
    return pa, keep


def _expected_bits(rows_bits, masks, V):
    want = rows_bits.copy()
    for b, w in enumerate(masks):
        if w is not None:
            want[b, :V][~unpack(w, V)] = NINF_BITS
    return want


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("B,V,ld", SHAPES)
def test_bitmask_kernel_is_exact(B, V, ld, case):
    from mlx_vlm_amd import ops
    from mlx_vlm_amd.sample_utils import make_logits_processors

    host = _logits(B, V, ld)
    masks = _masks(case, B, V)
    if case == "unaligned_rows":                                # row bases off the 16-byte grid: the one-token-per-thread path
        store = torch.full((B, ld + 8), float("nan"), dtype=BF)
        store[:, 1:V + 1] = host[:, :V]
        dev = store.to(DEV)
        view = dev[:, 1:V + 1]
        assert view.data_ptr() % 16 != 0
        host = store
        col0 = 1
    else:
        dev = host.to(DEV)
        view = dev[:, :V]
        col0 = 0
    specs = hist = None
    start_bits = host.view(torch.int16).numpy().copy()
    if case == "with_penalties":
        # a bias list and a repetition penalty on the masked rows: the mask comes AFTER them (penalties by the launch that has
        # always applied them - slot 7 zero - then masked_fill)
        rng = np.random.default_rng(V)
        specs = [make_logits_processors(logit_bias={int(t): float(v) for t, v in zip(rng.integers(0, V, 5), (4.0, -3.0, 2.5, 8.0, -1.0))},
                                        repetition_penalty=1.5, repetition_context_size=8) for _ in range(B)]
        hist = [rng.integers(0, V, 10).tolist() for _ in range(B)]
        ref = dev.clone()
        pa0, keep0 = _tables(B, V, [None] * B, specs, hist)
        ops.apply_logit_penalties(ref[:, :V], pa0)
        start_bits = ref.cpu().view(torch.int16).numpy().copy()
        assert (start_bits != host.view(torch.int16).numpy()).sum() >= B          # the penalties do change the rows
    pa, keep = _tables(B, V, masks, specs, hist)
    ops.apply_logit_penalties(view, pa)
    torch.cuda.synchronize()
    got = dev.cpu().view(torch.int16).numpy()
    want = start_bits.copy()
    want[:, col0:col0 + V] = _expected_bits(start_bits[:, col0:col0 + V], masks, V)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (case, B, V, len(bad), bad[:5].tolist())
    # (the padding between V and ld - NaN - is part of the comparison above: it kept its bits)
    assert np.isnan(dev[:, col0 + V:].float().cpu().numpy()).all()
    if case in ("half", "short_w") and B <= 16:
        # ops.apply_token_mask: the same launch from a [B, W] array of words (equal W per row)
        W = min(len(m) for m in masks)
        again = _logits(B, V, ld).to(DEV)
        out = ops.apply_token_mask(again[:, :V], np.stack([m[:W] for m in masks]))
        assert out.data_ptr() == again.data_ptr()
        want2 = _logits(B, V, ld).view(torch.int16).numpy().copy()
        want2[:, :V] = _expected_bits(want2[:, :V], [m[:W] for m in masks], V)
        assert np.array_equal(again.cpu().view(torch.int16).numpy(), want2)


def test_apply_token_mask_one_row_and_refusals():
    from mlx_vlm_amd import ops

    x = _logits(1, 1000, 1024)[0, :1000].contiguous()
    w = pack(np.arange(1000) % 3 == 0, words_of(1000))
    out = ops.apply_token_mask(x.to(DEV), torch.from_numpy(w).to(DEV))          # [V] logits, [W] words, words on the device
    keep = np.arange(1000) % 3 == 0
    assert np.array_equal(out.cpu().view(torch.int16).numpy()[keep], x.view(torch.int16).numpy()[keep])
    assert (out.cpu().view(torch.int16).numpy()[~keep] == NINF_BITS).all()
    with pytest.raises(ValueError):
        ops.apply_token_mask(x.to(DEV)[None], np.zeros((2, 4), dtype=np.int32))
    with pytest.raises(ValueError):
        ops.apply_token_mask(x.to(DEV).float(), w)


# ------------------------------------------------------------------------------------------ the sampler over masked rows
SPARSE = ["twenty", "three_in_one_block", "one_in_last_word", "short_w_twenty"]


@functools.lru_cache(maxsize=None)
def _sparse_rows(V):
    """One row per SPARSE case: N(0, 3^2) logits under a sparse mask - whole 1/64 blocks of -inf, a single survivor, a survivor
    only in the last (partial) word.  Seeds whose exact logsumexp falls inside the guard band are replaced (sampler_exact.py:
    a condition on the inputs).  -> (logits bf16 [4, V], masks, allowed bool [4, V], exact log-probs bf16 [4, V])"""
    MW = words_of(V)
    xs, masks, allowed = [], [], []
    for i, case in enumerate(SPARSE):
        for seed in range(100):
            rng = np.random.default_rng([V, i, seed])
            if case == "twenty":
                w = pack(np.isin(np.arange(32 * MW), rng.integers(0, V, 20)), MW)
            elif case == "three_in_one_block":
                base = S.block_per(V) * 17 if V > 64 * 20 else 0
                w = pack(np.isin(np.arange(32 * MW), base + rng.choice(min(S.block_per(V), V - base), 3, replace=False)), MW)
            elif case == "one_in_last_word":
                w = pack(np.arange(32 * MW) == int(rng.integers(32 * (MW - 1), V)), MW)
            else:
                n = MW // 2
                w = pack(np.isin(np.arange(32 * n), rng.integers(0, 32 * n, 20)), n)
            x = (torch.from_numpy(rng.standard_normal(V)) * 3.0).to(BF)
            ok = torch.from_numpy(unpack(w, V))
            xm = x.masked_fill(~ok, S.NEG_INF)
            lse = torch.logsumexp(xm.double(), -1)
            if float(lse) == 0.0:
                continue
            if float(S.exact_logprobs(xm[None])[2][0]) >= S.GUARD_BAND:
                break
        else:
            raise AssertionError("no seed outside the guard band")
        xs.append(x), masks.append(w), allowed.append(ok)
    x, allowed = torch.stack(xs), torch.stack(allowed)
    lp, _, band = S.exact_logprobs(x.masked_fill(~allowed, S.NEG_INF))
    assert float(band.min()) >= S.GUARD_BAND
    return x, tuple(masks), allowed, lp


def _masked_on_device(V):
    from mlx_vlm_amd import ops

    x, masks, allowed, lp = _sparse_rows(V)
    pa, keep = _tables(len(SPARSE), V, list(masks))
    dev = x.to(DEV)
    ops.apply_logit_penalties(dev, pa)
    assert torch.equal(S.bits(dev.cpu()), S.bits(x.masked_fill(~allowed, S.NEG_INF)))
    return dev, allowed, lp


def _argmax_first(lp):
    return torch.argmax((lp.float() == lp.float().max(-1, keepdim=True).values).to(torch.int8), dim=-1)


@pytest.mark.parametrize("V", [151936, 32003, 1000])
def test_greedy_forms_over_masked_rows(V):
    from mlx_vlm_amd import ops

    dev, allowed, lp = _masked_on_device(V)
    B = dev.shape[0]
    want = _argmax_first(lp)
    tok, got = ops.sample(dev)
    assert torch.equal(S.bits(got.cpu()), S.bits(lp)), ("plain greedy", V, (S.bits(got.cpu()) != S.bits(lp)).nonzero()[:5].tolist())
    assert tok.cpu().long().tolist() == want.tolist() and bool(allowed[torch.arange(B), tok.cpu().long()].all())
    # the fused greedy tail
    D = 64
    embed = torch.randn(V, D, generator=torch.Generator().manual_seed(V)).to(BF).to(DEV)
    ws = ops.sample_workspace(B, DEV)
    ctx = torch.arange(10, 10 + B, dtype=torch.int32, device=DEV)
    pos = torch.arange(20, 20 + B, dtype=torch.int32, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    tok2 = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    hid = torch.zeros(B, D, dtype=BF, device=DEV)
    got2 = ops.sample_greedy_advance(dev, tok2, ctx, pos, step, embed, hid, ws=ws)
    torch.cuda.synchronize()
    assert torch.equal(S.bits(got2.cpu()), S.bits(lp)), ("fused tail", V)
    assert tok2.cpu().long().tolist() == want.tolist() and torch.equal(hid, embed[want.to(DEV)]) and ops.bad_argmax_rows(ws) == 0


@pytest.mark.parametrize("kw", [dict(top_p=0.9, top_k=40), dict(min_p=0.05), dict()], ids=["top_p_top_k", "min_p", "temperature_only"])
@pytest.mark.parametrize("V", [151936, 32003, 1000])
def test_sampled_forms_over_masked_rows(V, kw):
    """the survivor rules of test_sampler_exact_gpu.py: the log-prob rows are exact, a filter only removes, at least one token
    survives, and the token is exact_draw's winner over the row the kernel itself drew from - an allowed token"""
    from mlx_vlm_amd import ops

    dev, allowed, lp = _masked_on_device(V)
    seed, temp = 23, 0.8
    for s in (0, 5, 11):
        st = torch.tensor([s], dtype=torch.int32, device=DEV)
        tok, got, filt = ops.sample(dev, temperature=temp, seed=seed, step=st, return_filtered=True, **kw)
        got, tok, filt = got.cpu(), tok.cpu().long(), filt.cpu()
        assert torch.equal(S.bits(got), S.bits(lp)), (V, kw, s, (S.bits(got) != S.bits(lp)).nonzero()[:5].tolist())
        for b, name in enumerate(SPARSE):
            kept = torch.isfinite(filt[b].float())
            assert bool(kept.any()) and not bool((kept & ~allowed[b]).any()), (V, kw, name)
            assert torch.equal(S.bits(filt[b])[kept], S.bits(lp[b])[kept]), (V, kw, name)
            assert bool(allowed[b, tok[b]]) and bool(kept[tok[b]]), (V, kw, name, int(tok[b]))
            w, gap = S.exact_draw(filt[b], temp, seed, s, b)
            if gap > S.DRAW_MARGIN:
                assert int(tok[b]) == w, (V, kw, name, s, int(tok[b]), w, gap)


@pytest.mark.parametrize("k", [5, 64])
def test_top_logprobs_with_fewer_allowed_tokens_than_k(k):
    """3 allowed tokens: the reference's order (argsort ascending, the last k, reversed), the tail of the list at -inf"""
    from mlx_vlm_amd import ops

    for V in (151936, 1000):
        lp = _sparse_rows(V)[3]
        row = SPARSE.index("three_in_one_block")
        assert int(torch.isfinite(lp[row].float()).sum()) == 3
        want_i, want_v = restatement(lp, k)
        idx, val = ops.top_logprobs(lp.to(DEV), k)
        assert torch.equal(idx.cpu(), want_i) and torch.equal(S.bits(val.cpu()), S.bits(want_v)), (V, k)
        assert bool(torch.isneginf(val[row, 3:].float()).all()) and bool(torch.isfinite(val[row, :3].float()).all())


# ------------------------------------------------------------------------------------------ end to end
VOC = 1024


class StandIn:
    """The stand-in matcher: at each step a seeded set of about 30 allowed tokens that depends on the step index and on the
    token it was last handed - a wrong or missing fed-back token changes every later mask."""

    def __init__(self, seed):
        self.seed, self.is_first_token, self.step, self.fed = seed, True, 0, []

    def allowed(self, last_token):
        key = 0 if self.is_first_token else int(last_token) + 1
        if not self.is_first_token:
            self.fed.append(int(last_token))
        self.is_first_token = False
        rng = np.random.default_rng([self.seed, self.step, key])
        self.step += 1
        return np.isin(np.arange(VOC), rng.integers(3, 1000, 30))

    def prepare_next_token_mask(self, last_token):
        self.last = self.allowed(last_token)
        return pack(self.last, words_of(VOC))[None]


class CallableForm:
    """the same constraint as a plain callable (tokens, logits) -> logits.masked_fill(~allowed, -inf): the eager route"""

    def __init__(self, seed):
        self.m = StandIn(seed)

    def __call__(self, tokens, logits):
        ok = torch.from_numpy(self.m.allowed(int(tokens[-1]))).to(logits.device)
        return logits.masked_fill(~ok[None], float("-inf"))


@pytest.fixture(scope="module")
def tiny():
    cfg = oq.tiny_cfg()
    W = oq.random_weights(cfg, seed=1234, dtype=BF, std=0.05, embed_std=0.2)
    assert cfg.text.vocab_size == VOC
    return cfg, build_product_model(cfg, W, kv_pool_tokens=16384, max_seqs=24)


def _prompts(n, seed0=900):
    return [np.random.default_rng(seed0 + i).integers(3, 1000, 6 + 2 * i) for i in range(n)]


def _run(model, prompts, max_tokens, processors, rows=4, **kw):
    from mlx_vlm_amd.batch import BatchGenerator

    gen = BatchGenerator(model, None, max_tokens=8, completion_batch_size=rows, prefill_batch_size=rows, async_prefill=False, **kw)
    uids = gen.insert(prompts, list(max_tokens), logits_processors=processors)
    got = {u: [] for u in uids}
    while gen.has_work:
        _, out = gen.next()
        for r in out:
            got[r.uid].append(r)
    steps = gen._unpipelined_steps
    gen.close()
    return [got[u] for u in uids], steps


def _stream(rs):
    return [(r.token, r.token_logprob) for r in rs]


def test_batch_generator_mask_rows_on_captured_steps(tiny, monkeypatch):
    from mlx_vlm_amd.sample_utils import make_logits_processors

    cfg, model = tiny
    lm = model.language_model
    calls = {"forward": 0}
    real = lm.decode_forward_rows

    def counted(*a, **k):
        calls["forward"] += 1
        return real(*a, **k)

    monkeypatch.setattr(lm, "decode_forward_rows", counted)
    prompts = _prompts(3)
    spec = lambda: make_logits_processors(repetition_penalty=1.3, repetition_context_size=12)      # noqa: E731
    masked = [StandIn(1), StandIn(2)]
    cap, steps = _run(model, prompts, [12, 12, 12], [masked[0], [spec(), masked[1]], None])
    assert calls["forward"] == 0 and steps >= 11               # captured steps, none of them enqueued ahead of its tokens
    eag, _ = _run(model, prompts, [12, 12, 12], [CallableForm(1), [spec(), CallableForm(2)], None])
    assert calls["forward"] >= 11                               # (the callable form does take the eager step)
    for c, e in zip(cap, eag):
        assert _stream(c) == _stream(e)                         # tokens equal, log-probs bit-equal
    for m, rs in zip(masked, cap[:2]):
        assert m.fed == [r.token for r in rs][:-1] and m.step == 12
        assert all(np.isfinite(r.token_logprob) for r in rs)
    calls["forward"] = 0
    free, steps = _run(model, prompts[2:], [12], [None])
    assert [r.token for r in free[0]] == [r.token for r in cap[2]] and steps == 0 and calls["forward"] == 0
    plain, _ = _run(model, prompts[:1], [12], [None])
    assert [r.token for r in plain[0]] != [r.token for r in cap[0]]          # the mask does change the stream


def test_batch_generator_masked_newcomer_takes_a_finished_masked_row(tiny):
    cfg, model = tiny
    prompts = _prompts(3, seed0=950)                            # queue order = length order: free, masked (3 tokens), masked (queued)
    new = StandIn(7)
    got, steps = _run(model, prompts, [12, 3, 8], [None, StandIn(5), new], rows=2)
    assert [len(g) for g in got] == [12, 3, 8] and new.fed == [r.token for r in got[2]][:-1]
    alone, _ = _run(model, prompts[2:], [8], [StandIn(7)], rows=2)
    assert [r.token for r in alone[0]] == [r.token for r in got[2]]
    old, _ = _run(model, prompts[1:2], [3], [StandIn(5)], rows=2)
    assert [r.token for r in old[0]] == [r.token for r in got[1]]
    free, _ = _run(model, prompts[:1], [12], [None], rows=2)
    assert [r.token for r in free[0]] == [r.token for r in got[0]]


def test_generate_step_mask_processor_replays_the_graph(tiny, monkeypatch):
    from mlx_vlm_amd import _lib
    from mlx_vlm_amd import generate as gen_mod

    cfg, model = tiny
    ids = _prompts(1, seed0=970)[0][None]
    n = 12
    eag = [(t, lp.float().cpu()) for t, lp in gen_mod.generate_step(ids, model, None, None, max_tokens=n, temperature=0.0,
                                                                    logits_processors=[CallableForm(3)])]

    def no_eager(*a, **k):
        raise AssertionError("_generate_step_eager entered")

    monkeypatch.setattr(gen_mod, "_generate_step_eager", no_eager)
    L = _lib.lib()
    counts = {"launch": 0, "step": 0}
    real_launch, real_step = L.vlm_llm_decode_graph_launch, L.vlm_llm_decode_step

    def launch(*a):
        counts["launch"] += 1
        return real_launch(*a)

    def step(*a):
        counts["step"] += 1
        return real_step(*a)

    monkeypatch.setattr(L, "vlm_llm_decode_graph_launch", launch)
    monkeypatch.setattr(L, "vlm_llm_decode_step", step)
    m = StandIn(3)
    cap = [(t, lp.float().cpu()) for t, lp in gen_mod.generate_step(ids, model, None, None, max_tokens=n, temperature=0.0,
                                                                    logits_processors=[m])]
    assert counts == {"launch": n - 1, "step": 0}
    assert [t for t, _ in cap] == [t for t, _ in eag] and all(torch.equal(a, b) for (_, a), (_, b) in zip(cap, eag))
    assert m.fed == [t for t, _ in cap][:-1]
    # a spec beside the mask processor: the penalties first, then the mask, still captured
    from mlx_vlm_amd.sample_utils import make_logits_processors
    spec = make_logits_processors(repetition_penalty=1.4, repetition_context_size=16)
    both = [t for t, _ in gen_mod.generate_step(ids, model, None, None, max_tokens=n, temperature=0.0, logits_processors=[spec, StandIn(3)])]
    monkeypatch.undo()
    ref = [t for t, _ in gen_mod.generate_step(ids, model, None, None, max_tokens=n, temperature=0.0,
                                               logits_processors=[spec, CallableForm(3)])]
    assert both == ref


def test_top_logprobs_of_a_masked_row_list_allowed_tokens_only(tiny):
    cfg, model = tiny
    m = StandIn(11)
    seen = []
    real = m.prepare_next_token_mask

    def spy(t):
        w = real(t)
        seen.append(m.last.copy())
        return w

    m.prepare_next_token_mask = spy
    got, _ = _run(model, _prompts(2, seed0=990), [6, 6], [m, None], top_logprobs_k=5)
    assert len(seen) == 6
    for r, ok in zip(got[0], seen):
        assert len(r.top_logprobs) == 5 and ok[r.token]
        assert all(ok[t] for t, v in r.top_logprobs if np.isfinite(v)) and sum(np.isfinite(v) for _, v in r.top_logprobs) == 5
        assert r.top_logprobs[0][1] >= r.top_logprobs[-1][1]
