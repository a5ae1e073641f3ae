"""The sampler head of csrc/sample.hip on MI355X against the exact result (tests/sampler_exact.py): for every row of the named
table the log-probs are BIT-IDENTICAL to exact_logprobs and the token equals argmax_first of them, through every form that
computes them - plain greedy (lse_partial + logprob_argmax), the fused greedy tail in its four layouts and at 16 / 64 rows
(the two-level ticket), temperature-only sampling, and the split path whose histogram launch writes the log-probs.  The draw
(Gumbel-max with the counter hash) EQUALS exact_draw's float64 winner on every draw of every case, and returns the dominant
token of a peaked row at the two (seed, step, index) where the uniform used to be 1.0.

The only two figures in this file are conditions on the INPUTS, asserted where the inputs are built and never allowances
for the kernel: the guard band (2^-12: no row's logsumexp that close to a bf16 rounding tie) and the draw margin (2^-18:
no draw whose two best are that close).  The CPU side (test_sampler_exact_cpu.py) shows that a float32 kernel attains the
bar and that six subtly wrong ones miss it.  `pytest -s` prints one line per form and row and one per draw case."""
import pytest
import torch

from tests import sampler_exact as S

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def vops():
    from mlx_vlm_amd import ops
    return ops


def _step(s):
    return torch.tensor([s], dtype=torch.int32, device=DEV)


def test_plain_greedy_is_bit_identical_on_every_row(vops):
    for V, h in S.head_rows().items():
        tok, lp = vops.sample(h.x.to(DEV))
        S.check_head("greedy", h, lp, tok)


# ------------------------------------------------------------------ the fused greedy tail
def _layout(x, layout):
    """the logits of a fused-tail call: x bf16 [B, V] on the device -> a view with the same values.  Whatever lies around the
    view is NaN: a kernel that reads outside its rows poisons them."""
    B, V = x.shape
    if layout in ("vec16", "ragged"):                       # contiguous: V % 8 == 0 -> 16-byte accesses, else the scalar loop
        assert (V % 8 == 0) == (layout == "vec16")
        return x.contiguous()
    pitch = (V + 7) // 8 * 8 + 8
    buf = torch.full((B, pitch), NAN, dtype=BF, device=x.device)
    v = buf[:, :V] if layout == "wide_pitch" else buf[:, 1:V + 1]      # ld > V on an aligned base / an unaligned row pointer
    v.copy_(x)
    assert v.stride(0) == pitch and pitch % 8 == 0 and (v.data_ptr() % 16 == 0) == (layout == "wide_pitch")
    return v


def _run_tail(vops, form, h, layout, calls=2):
    """vlm_sample_greedy_advance over the rows of h, `calls` times on ONE workspace (the tickets re-arm themselves; the second
    call sees the rows in reverse order): log-probs, tok, h = embed[tok], ctx / pos / step / token ring"""
    B, V, D, ring_len = len(h.names), h.V, 64, 4
    embed = torch.randn(V, D, generator=torch.Generator().manual_seed(V + B)).to(BF).to(DEV)
    ws = vops.sample_workspace(B, DEV)
    ctx = torch.arange(10, 10 + B, dtype=torch.int32, device=DEV)
    pos = torch.arange(20, 20 + B, dtype=torch.int32, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    ring = torch.full((ring_len, B), -1, dtype=torch.int32, device=DEV)
    tok = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    hid = torch.zeros(B, D, dtype=BF, device=DEV)
    for it in range(calls):
        hh = h if it % 2 == 0 else S.Head(V, h.names[::-1], h.x.flip(0), h.lp.flip(0), h.tok.flip(0), h.lse.flip(0), h.band.flip(0))
        logits = _layout(hh.x.to(DEV), layout)
        lp = vops.sample_greedy_advance(logits, tok, ctx, pos, step, embed, hid, out_ring=ring, ws=ws)
        torch.cuda.synchronize()
        S.check_head(f"{form} call {it}", hh, lp, tok)
        want = hh.tok.to(DEV)
        assert torch.equal(hid, embed[want]), (form, V, it)
        assert ctx.tolist() == list(range(11 + it, 11 + it + B)) and pos.tolist() == list(range(21 + it, 21 + it + B)), (form, V, it)
        assert int(step[0]) == it + 1 and torch.equal(ring[it % ring_len].long(), want), (form, V, it)
        assert vops.bad_argmax_rows(ws) == 0
    assert bool((ring[calls:] == -1).all())


@pytest.mark.parametrize("layout", ["vec16", "wide_pitch", "unaligned", "ragged"])
def test_fused_greedy_tail_is_bit_identical_on_every_row(vops, layout):
    for V, h in S.head_rows().items():
        if layout == "vec16" and V % 8 or layout == "ragged" and V % 8 == 0:
            continue
        _run_tail(vops, f"tail {layout}", h, layout)


@pytest.mark.parametrize("B", [16, 64])
@pytest.mark.parametrize("layout", ["vec16", "wide_pitch", "unaligned", "ragged"])
def test_fused_greedy_tail_wide_batches(vops, layout, B):
    """the two-level ticket (a row's 64 blocks, then the rows) at 16 and 64 DISTINCT rows of V = 8192 (V = 8191 for the layout
    whose point is V % 8 != 0)"""
    _run_tail(vops, f"tail {layout} B={B}", S.batch_rows(8191 if layout == "ragged" else 8192, B), layout)


# ------------------------------------------------------------------ the sampled forms
def test_temperature_only_logprobs_and_tokens(vops):
    """no filter: lse_partial + logprob_argmax write the log-probs, gumbel_partial draws over them"""
    seed, step, temp = S.TABLE_DRAW
    for V, h in S.head_rows().items():
        tok, lp = vops.sample(h.x.to(DEV), temperature=temp, seed=seed, step=_step(step))
        lp, tok = lp.cpu(), tok.cpu()
        assert torch.equal(S.bits(lp), S.bits(h.lp)), ("temperature-only", V, S.head_mismatch(h, lp, h.tok))
        for b, name in enumerate(h.names):
            w, gap = S.exact_draw(h.lp[b], temp, seed, step, b)
            assert gap > S.DRAW_MARGIN, (V, name, gap)      # (a condition on the inputs: the CPU test asserts it as well)
            assert int(tok[b]) == w, ("temperature-only", V, name, int(tok[b]), w, gap)
            print(f"SAMPLER-EXACT {'temperature-only':24s} V={V:<6d} {name:28s} bit-identical, token {int(tok[b])} == exact winner "
                  f"(gap {gap:.2e})")


@pytest.mark.parametrize("V", [8192, 151936])
def test_split_path_writes_exact_logprobs_from_logits(vops, V):
    """top-p from logits on an aligned row of V >= 8192: topp_hist_kernel<true> writes the log-probs inside the histogram launch"""
    h = S.head_rows()[V]
    seed, step, temp = 23, 5, 0.8
    tok, lp, filt = vops.sample(h.x.to(DEV), temperature=temp, top_p=0.9, seed=seed, step=_step(step), return_filtered=True)
    lp, tok, filt = lp.cpu(), tok.cpu(), filt.cpu()
    bad = dict(S.head_mismatch(h, lp, h.tok))
    for b, name in enumerate(h.names):
        print(f"SAMPLER-EXACT {'split top-p from logits':24s} V={V:<6d} {name:28s} " + (f"MISMATCH: {bad[name]}" if name in bad else "bit-identical"))
    assert not bad, bad
    for b, name in enumerate(h.names):                      # a filter only removes; the draw runs over what it left
        kept = torch.isfinite(filt[b].float())
        assert bool(kept.any()) and torch.equal(S.bits(filt[b])[kept], S.bits(h.lp[b])[kept]), name
        w, gap = S.exact_draw(filt[b], temp, seed, step, b)
        if gap > S.DRAW_MARGIN:
            assert int(tok[b]) == w, (name, int(tok[b]), w, gap)


@pytest.mark.parametrize("name", sorted(S.draw_cases()))
def test_every_draw_equals_the_exact_winner(vops, name):
    """30 steps over 2 - 3 rows per case: the kernel's token == exact_draw's winner over the row the kernel itself drew from
    (its log-probs - asserted exact - or its own filtered row), and no draw falls under the margin"""
    c = S.draw_cases()[name]
    x = c["x"].to(DEV)
    lp_exact = S.exact_logprobs(c["x"])[0]
    toks, rows, st = [], None, _step(0)
    for s in range(S.DRAW_STEPS):
        st.fill_(s)
        tok, lp, filt = vops.sample(x, temperature=S.DRAW_TEMP, seed=S.DRAW_SEED, step=st, return_filtered=True, **c["kw"])
        if rows is None:
            assert torch.equal(S.bits(lp.cpu()), S.bits(lp_exact)), name
            rows = filt.clone()
        else:
            assert torch.equal(S.bits(filt), S.bits(rows)), (name, s)        # the filter does not depend on the step
        toks.append(tok.clone())
    toks = torch.stack(toks).cpu()
    rows = rows.cpu()
    if c["kw"]:
        kept = torch.isfinite(rows.float())
        assert torch.equal(S.bits(rows)[kept], S.bits(lp_exact)[kept]) and 0 < int(kept.sum()) < kept.numel(), name
    S.check_draws(name, rows, toks)


@pytest.mark.parametrize("case", S.U_ONE_CASES, ids=lambda c: f"seed{c[0]}-step{c[1]}-V{c[4]}")
def test_peaked_row_draws_its_dominant_token_where_the_uniform_was_one(vops, case):
    """u[idx] was exactly 1.0 at this (seed, step, row 0): Gumbel noise +inf, and a token of probability e^-40 won"""
    seed, step, row, idx, V, dom = case
    x, lp_exact = S.peaked_row(V, dom)
    assert S.exact_draw(lp_exact[0], 1.0, seed, step, row, uniform=S.old_hash_uniform)[0] == idx
    for temp in (1.0, 0.8):
        tok, lp = vops.sample(x.to(DEV), temperature=temp, seed=seed, step=_step(step))
        assert torch.equal(S.bits(lp.cpu()), S.bits(lp_exact))
        assert int(tok[0]) == dom != idx, (case, temp, int(tok[0]))
    print(f"SAMPLER-EXACT peaked row V={V} seed={seed} step={step}: token {dom} (the dominant one), not {idx}")
