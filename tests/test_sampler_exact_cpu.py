"""The sampler head's exact bar, checked without a GPU (tests/sampler_exact.py; the GPU side is test_sampler_exact_gpu.py):

  * the row table builds: every named row keeps its promise and the guard band;
  * a float32 emulation of the kernels' own order is BIT-IDENTICAL to the exact result on every row - the bar is attainable;
  * six mutants of the same code are REJECTED by the comparison the GPU test uses, each on rows named here;
  * the RNG: hash_uniform is strictly inside (0, 1) where it used to be 1.0, bitwise unchanged everywhere else, and the draw
    over a peaked row returns the dominant token there (the old function, kept in sampler_exact, fails both);
  * no draw of the GPU test's cases falls under the margin, and the exact draw follows softmax(lp) (chi-square).  The
    distribution is checked here because the GPU test makes the kernel's tokens EQUAL to these winners."""
import math

import numpy as np
import pytest
import torch

from oracle import ops as O
from tests import sampler_exact as S

BF = torch.bfloat16


def test_row_table_is_complete_and_inside_the_guard_band():
    table = S.head_rows()
    assert tuple(table) == S.VS
    n = 0
    for V, h in table.items():
        assert h.x.dtype == BF and h.x.shape == (len(h.names), V) and len(set(h.names)) == len(h.names)
        assert float(h.band.min()) >= S.GUARD_BAND
        n += len(h.names)
        print(f"V={V:<6d} {len(h.names):2d} rows, smallest band {float(h.band.min()):.2e} ({h.names[int(h.band.argmin())]})")
    every = {n_ for h in table.values() for n_ in h.names}
    assert every == {"randn_x1.5", "randn_x3", "randn_x8", "dominant_first", "dominant_last", "dominant_mid", "flat",
                     "offset_plus200", "offset_minus200", "holes_every_7th", "hole_whole_block", "hole_first",
                     "collapsed_pair_one_chunk", "collapsed_pair_two_blocks", "ties_chunk_and_later_block"}
    assert any(V < 512 for V in table)                      # blocks with an empty range
    print(f"{n} rows")


def test_float32_emulation_of_the_kernels_order_is_bit_identical_to_the_exact_result():
    for V, h in S.head_rows().items():
        lp, tok = S.emulate_head(h.x)
        S.check_head("float32 emulation", h, lp, tok)
    for B in (16, 64):                                      # the rows of the wide-batch forms (both row lengths the GPU test uses)
        for V in (8192, 8191):
            h = S.batch_rows(V, B)
            lp, tok = S.emulate_head(h.x)
            assert not S.head_mismatch(h, lp, tok), (V, B)


# mutant -> rows (name, V) on which the comparison must reject it
REJECTED_ON = {
    "lse_f32": [("randn_x3", 151936), ("randn_x1.5", 4099), ("offset_plus200", 8192)],
    "lse_fp16": [("randn_x3", 151936), ("randn_x8", 32003)],
    # (only a row whose ragged end carries weight tells: on "flat" @ V = 4099 three of 4099 equal terms do not move the bf16 lse)
    "drop_tail": [("dominant_last", 32003), ("dominant_last", 7), ("dominant_last", 4099), ("dominant_last", 65)],
    "nan_block": [("hole_whole_block", 151936), ("hole_whole_block", 65)],
    "argmax_logits": [("collapsed_pair_one_chunk", 151936), ("collapsed_pair_two_blocks", 4099)],
    "tie_last": [("flat", 8192), ("ties_chunk_and_later_block", 65), ("collapsed_pair_two_blocks", 32003)],
}


@pytest.mark.parametrize("mutant", S.MUTANTS)
def test_mutants_of_the_kernel_are_rejected(mutant):
    table = S.head_rows()
    assert REJECTED_ON[mutant]
    for name, V in REJECTED_ON[mutant]:
        h = table[V]
        lp, tok = S.emulate_head(h.x, mutant)
        bad = dict(S.head_mismatch(h, lp, tok))
        assert name in bad, (mutant, name, V, sorted(bad))
        print(f"{mutant:14s} rejected on {name} @ V={V}: {bad[name]}")
        with pytest.raises(AssertionError):
            S.check_head(f"mutant {mutant}", h, lp, tok)


def test_hash_uniform_is_strictly_inside_the_unit_interval_and_otherwise_unchanged():
    below_one = np.nextafter(np.float32(1), np.float32(0))
    for seed, step, row, idx, V, _ in S.U_ONE_CASES:
        i = np.arange(V)
        old, new = S.old_hash_uniform(seed, step, row, i), O.hash_uniform(seed, step, row, i)
        assert new.dtype == np.float32 and old.dtype == np.float32
        assert old[idx] == np.float32(1.0) and not bool(((old > 0) & (old < 1)).all())       # the old function fails the check
        assert bool(((new > 0) & (new < 1)).all()) and new[idx] == below_one
        rest = i != idx
        assert np.array_equal(old[rest].view(np.uint32), new[rest].view(np.uint32))
        # ... and so is a neighbouring step of the same stream, every index
        assert np.array_equal(S.old_hash_uniform(seed, step + 1, row, i).view(np.uint32), O.hash_uniform(seed, step + 1, row, i).view(np.uint32))
    assert 0.0 < O.xtc_draw(3, 5, 0) < 1.0


def test_the_draw_over_a_peaked_row_returns_the_dominant_token_where_u_was_one():
    for seed, step, row, idx, V, dom in S.U_ONE_CASES:
        _, lp = S.peaked_row(V, dom)
        assert float(lp[0, dom]) == 0.0 and float(lp[0, idx]) < -30
        w_old, _ = S.exact_draw(lp[0], 1.0, seed, step, row, uniform=S.old_hash_uniform)
        assert w_old == idx                                 # the old function: a token of probability e^-40 wins
        for temp in (1.0, 0.8):
            w, gap = S.exact_draw(lp[0], temp, seed, step, row)
            assert w == dom and gap > S.DRAW_MARGIN, (seed, step, w, gap)
            assert O.categorical_gumbel(lp[0], temp, seed, step, row) == dom


def test_exact_draw_agrees_with_the_float32_oracle_and_skips_removed_tokens():
    lp = S.head_rows()[4099].lp
    names = S.head_rows()[4099].names
    for name in ("randn_x3", "holes_every_7th", "hole_whole_block"):
        r = lp[names.index(name)]
        for step in range(20):
            w, gap = S.exact_draw(r, 0.8, 5, step, 1)
            assert math.isfinite(float(r[w]))
            if gap > S.DRAW_MARGIN and not bool(torch.isinf(r).any()):       # (the float32 oracle computes -inf + g for a hole)
                assert O.categorical_gumbel(r, 0.8, 5, step, 1) == w
    one = torch.full((9,), float("-inf"), dtype=BF)
    one[4] = -2.0
    assert S.exact_draw(one, 0.8, 1, 2, 0) == (4, float("inf"))


@pytest.mark.parametrize("name", sorted(S.draw_cases()))
def test_no_draw_of_the_gpu_cases_falls_under_the_margin(name):
    """the same assertion the GPU test makes over the kernel's own filtered rows, here over the oracle's"""
    c = S.draw_cases()[name]
    lp = S.exact_logprobs(c["x"])[0]
    rows = O.sampler_filters(lp, S.DRAW_TEMP, **c["kw"]) if c["kw"] else lp
    S.check_draws(name, rows)


def test_no_draw_over_the_row_table_falls_under_the_margin():
    seed, step, temp = S.TABLE_DRAW
    for V, h in S.head_rows().items():
        gaps = [S.exact_draw(h.lp[b], temp, seed, step, b)[1] for b in range(len(h.names))]
        assert min(gaps) > S.DRAW_MARGIN, (V, h.names[int(np.argmin(gaps))], min(gaps))


def _chi2_quantile_999(dof):
    """Wilson-Hilferty: the 99.9 % quantile of chi-square (z = 3.0902); within 0.2 % of the exact value from 10 dof on"""
    return dof * (1 - 2 / (9 * dof) + 3.0902 * math.sqrt(2 / (9 * dof))) ** 3


def test_exact_draw_follows_the_distribution():
    """one V = 64 row (randn * 1.5, seed 11) at temperature 1, drawn by 16 RNG rows x 500 steps: chi-square of the winners
    against softmax(lp), bins merged (in descending probability) to an expectation of at least 20.  Measured 46.0 at 45 dof."""
    V, B, steps = 64, 16, 500
    x = (torch.randn(1, V, generator=torch.Generator().manual_seed(11)) * 1.5).to(BF)
    lp = S.exact_logprobs(x)[0][0]
    p = torch.softmax(lp.double(), -1).numpy()
    n = B * steps
    counts = np.bincount([S.exact_draw(lp, 1.0, 11, s, b)[0] for b in range(B) for s in range(steps)], minlength=V)
    bins, e, o = [], 0.0, 0
    for i in np.argsort(-p):
        e, o = e + n * p[i], o + counts[i]
        if e >= 20:
            bins.append((e, o))
            e, o = 0.0, 0
    if e > 0:                                               # the remainder joins the last bin
        bins[-1] = (bins[-1][0] + e, bins[-1][1] + o)
    assert abs(sum(e for e, _ in bins) - n) < 1e-6 and sum(o for _, o in bins) == n
    chi2, dof = sum((o - e) ** 2 / e for e, o in bins), len(bins) - 1
    q = _chi2_quantile_999(dof)
    print(f"chi-square {chi2:.1f} at {dof} dof (99.9 % quantile {q:.1f})")
    assert dof >= 40 and chi2 < q, (chi2, dof, q)
