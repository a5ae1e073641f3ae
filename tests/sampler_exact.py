"""The exact results of the sampler head (csrc/sample.hip: logits -> bf16 log-probs -> greedy argmax or Gumbel-max draw), the
named row table both sampler-head tests share, and a float32 emulation of the kernels' own order with the mutants a wrong
kernel would be.

The kernels follow the reference's typed graph (ar.py:368): the logsumexp is MATERIALISED in bf16 (L) and the log-prob is
bf16(x - L).  L is one rounding of a float32 sum; x - L is a difference of two bf16 values.  So a kernel's row is either
bit-identical to the exactly rounded one or wrong - unless the exact logsumexp sits so close to a bf16 rounding tie that a
legitimate float32 sum may land on the other neighbour.  The GUARD BAND removes that case from the inputs instead of
tolerating it in the outputs: every row of the table keeps its exact lse at least 2^-12 |lse| away from both ties next to L
(the kernels' float32 lse - 64 partial sums, one expf each, one logf - is within about 2^-22 |lse| of the exact one; the band
is 1000 times that).  About one random row in ten falls inside it and is replaced by another seed; head_rows() asserts the
band, so it is checked wherever the table is built.

The draw is z_i = lp_i * float32(1 / temp) - log(-log(u_i)) with u_i = oracle.hash_uniform(seed, step, row, i), the token is
argmax z (lowest index on a tie).  exact_draw evaluates it in float64 and returns the relative gap between the two best: the
kernel's float32 z (two logf of at most 1 ulp each and one fma) is within about 2^-22 max(1, |z|) of the exact value, so
where the gap exceeds DRAW_MARGIN = 2^-18 (16 times that) the kernel's token must EQUAL the exact winner.  draw_cases()
chooses inputs on which no draw falls under the margin; both tests assert that.

Imports without a GPU: tests/test_sampler_exact_cpu.py checks the table, the emulation, the mutants and the RNG here;
tests/test_sampler_exact_gpu.py holds the kernels to the same table."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np
import torch

from oracle import ops as O
from tests.attn_exact import rne_bf16

BF, F64 = torch.bfloat16, torch.float64
NBLK = 64                              # workgroups per vocabulary row (csrc/sample.hip)
GUARD_BAND = 2.0 ** -12                # min |lse - tie| / |lse| of every row fed to a kernel
DRAW_MARGIN = 2.0 ** -18               # min (z1 - z2) / max(1, |z1|) at which the kernel's token must equal the exact winner
VS = (151936, 32003, 8192, 4099, 513, 65, 7, 1)
NEG_INF = float("-inf")


def block_per(V: int) -> int:
    """elements per block of a row split over NBLK workgroups: per = ((V + 63) / 64 + 7) & ~7"""
    return ((V + NBLK - 1) // NBLK + 7) & ~7


def bits(x: torch.Tensor) -> torch.Tensor:
    return x.contiguous().view(torch.int16)


# ------------------------------------------------------------------ the exact results
def exact_logprobs(x: torch.Tensor):
    """x bf16 [B, V] -> (lp bf16 [B, V], lse float64 [B], band float64 [B]).  lse in float64, rounded ONCE to bf16 (L);
    lp = the nearest bf16 of x - L (one rounding of the exact difference); -inf stays -inf.  band: the distance of the exact
    lse from the nearer of the two bf16 rounding ties next to L, relative to |lse|."""
    assert x.dtype == BF and x.dim() == 2
    xd = x.to(F64)
    lse = torch.logsumexp(xd, -1)
    assert bool(torch.isfinite(lse).all()) and bool((lse != 0).all()), "a row needs a finite, non-zero logsumexp"
    L = rne_bf16(lse)
    hole = torch.isinf(xd) & (xd < 0)
    d = torch.where(hole, torch.zeros_like(xd), xd - L[:, None])
    lp = torch.where(hole, xd, rne_bf16(d)).to(BF)
    lb = bits(L.to(BF)).to(torch.int32)                     # the two bf16 neighbours of L: one step in the bit pattern either way
    up = (lb + 1).to(torch.int16).view(BF).to(F64)
    dn = (lb - 1).to(torch.int16).view(BF).to(F64)
    ties = torch.stack([(L + up) / 2, (L + dn) / 2])
    band = (lse[None] - ties).abs().min(0).values / lse.abs()
    return lp, lse, band


def exact_draw(lp: torch.Tensor, temp: float, seed: int, step: int, row: int, uniform=None):
    """lp bf16 [V] (the row the draw runs over: log-probs, or a filtered row with -inf holes) -> (winner, gap).
    Float64: z = lp * float64(float32(1) / float32(temp)) - log(-log(float64(u))), u from oracle.hash_uniform (or `uniform`,
    same signature); -inf entries are excluded; the lowest index wins a tie; gap = (z1 - z2) / max(1, |z1|) between the two
    best (inf with fewer than two candidates, or when the best is infinite)."""
    x = lp.to(F64).numpy()
    V = x.shape[-1]
    u = (uniform or O.hash_uniform)(seed, step, row, np.arange(V)).astype(np.float64)
    it = np.float64(np.float32(1) / np.float32(temp))
    with np.errstate(divide="ignore", invalid="ignore"):
        z = x * it - np.log(-np.log(u))
    z[np.isneginf(x)] = -np.inf
    w = int(np.argmax(z))                                   # np.argmax: the first index of the maximum
    z1 = float(z[w])
    assert z1 > -np.inf, "a row with every token removed has no draw"
    z[w] = -np.inf
    z2 = float(z.max()) if V > 1 else -np.inf
    gap = float("inf") if (math.isinf(z1) or z2 == -np.inf) else (z1 - z2) / max(1.0, abs(z1))
    return w, gap


# ------------------------------------------------------------------ the named row table
@dataclass(frozen=True)
class Head:
    """every row of one vocabulary size, with its exact results (computed once, never modified)"""
    V: int
    names: tuple
    x: torch.Tensor          # bf16 [B, V] logits
    lp: torch.Tensor         # bf16 [B, V] exact log-probs
    tok: torch.Tensor        # int64 [B] argmax_first(lp)
    lse: torch.Tensor        # float64 [B]
    band: torch.Tensor       # float64 [B]


def _randn(V, seed, scale=1.0):
    return torch.randn(V, generator=torch.Generator().manual_seed(seed)) * scale


def _next_bf16(v: float) -> float:
    t = torch.tensor([v], dtype=BF)
    return float((bits(t) + 1).view(BF)[0])


COLLAPSED_A = 0.5                      # the collapsed pair: two adjacent bf16 values, 2^-9 apart, over a narrow (0.05 sigma) row


def _cases(V):
    """-> [(name, builder(seed) -> float tensor [V] or [n, V])] of the cases that exist at this V"""
    per = block_per(V)
    nb = (V + per - 1) // per                               # blocks with a non-empty range
    mid = V // 2

    def put(x, idx, val):
        x = x.clone()
        x[idx] = val
        return x

    c = [(f"randn_x{s:g}", lambda sd, s=s: _randn(V, sd, s)) for s in (1.5, 3.0, 8.0)]
    c.append(("dominant_first", lambda sd: put(_randn(V, sd), 0, 40.0)))
    if V >= 3:
        c.append(("dominant_last", lambda sd: put(_randn(V, sd), V - 1, 40.0)))
        c.append(("dominant_mid", lambda sd: put(_randn(V, sd), mid, 40.0)))
    # (no seed to move: at a V where 1.5 + log V falls inside the band - V = 7 does - the row is left out, not tolerated)
    if float(exact_logprobs(torch.full((1, V), 1.5, dtype=BF))[2]) >= GUARD_BAND:
        c.append(("flat", lambda sd: torch.full((V,), 1.5)))
    # (one builder, two rows: "the same row minus 200" keeps its seed when the other one has to move out of the band)
    c.append(("offset_plus200|offset_minus200", lambda sd: torch.stack([_randn(V, sd, 3.0) + 200.0, _randn(V, sd, 3.0) - 200.0])))
    if V >= 7:
        c.append(("holes_every_7th", lambda sd: put(_randn(V, sd, 3.0), slice(3, None, 7), NEG_INF)))
    if nb >= 2:
        k = nb // 2
        c.append(("hole_whole_block", lambda sd: put(_randn(V, sd, 3.0), slice(k * per, min(V, (k + 1) * per)), NEG_INF)))
    if V >= 2:
        c.append(("hole_first", lambda sd: put(_randn(V, sd, 3.0), 0, NEG_INF)))
    if V >= 4096:                                           # |log-prob| ~ log V > 8: its bf16 step (2^-4) is 32 times the pair's distance
        b = _next_bf16(COLLAPSED_A)
        ch = 8 * (mid // 8)
        c.append(("collapsed_pair_one_chunk", lambda sd: put(put(_randn(V, sd, 0.05), ch + 1, COLLAPSED_A), ch + 6, b)))
        c.append(("collapsed_pair_two_blocks", lambda sd: put(put(_randn(V, sd, 0.05), 3 * per + 5, COLLAPSED_A), 40 * per + 2, b)))
    if nb >= 3:
        c.append(("ties_chunk_and_later_block", lambda sd: put(_randn(V, sd, 3.0), [per + 2, per + 5, (nb - 1) * per], 20.0)))
    return c


def _banded(build, seed0, what):
    """the first of seed0, seed0 + 1000, ... whose rows all keep the guard band (a deterministic row has one chance)"""
    for attempt in range(12):
        x = build(seed0 + 1000 * attempt)
        x = (x if x.dim() == 2 else x[None]).to(BF)
        if float(exact_logprobs(x)[2].min()) >= GUARD_BAND:
            return x
    raise AssertionError(f"{what}: no seed keeps the logsumexp {GUARD_BAND:g} away from a bf16 rounding tie")


def _assert_case(name, V, x, lp, tok):
    """what the table promises about a named row, checked on the exact result"""
    xf, per = x.float(), block_per(V)
    if name.startswith("dominant"):
        i = {"dominant_first": 0, "dominant_last": V - 1, "dominant_mid": V // 2}[name]
        assert tok == i and int(bits(lp)[i]) == 0, (name, V, "the winner's log-prob is +0.0")
    elif name == "flat":
        assert tok == 0 and len(set(bits(lp).tolist())) == 1, (name, V)
    elif name.startswith("collapsed_pair"):
        top = torch.topk(xf, 2)
        hi, lo = int(top.indices[0]), int(top.indices[1])
        assert float(top.values[0]) > float(top.values[1]), (name, V, "two DISTINCT bf16 logits")
        assert hi > lo, (name, V, "the larger logit sits at the higher index")
        assert int(bits(lp)[hi]) == int(bits(lp)[lo]), (name, V, "both round to the same log-prob")
        assert float(lp[lo]) > float(torch.cat([lp[:lo], lp[lo + 1:hi], lp[hi + 1:]]).float().max()), (name, V)
        assert tok == lo, (name, V, "argmax of the log-probs: the lower index, the SMALLER logit")
        same_chunk, same_block = hi // 8 == lo // 8, hi // per == lo // per
        assert same_chunk if name.endswith("one_chunk") else not same_block, (name, V, hi, lo)
    elif name == "ties_chunk_and_later_block":
        i = torch.nonzero(xf == xf.max()).flatten().tolist()
        assert len(i) == 3 and i[0] // 8 == i[1] // 8 and i[2] // per > i[1] // per and tok == i[0], (name, V, i)
    elif name == "hole_whole_block":
        k = ((V + per - 1) // per) // 2
        assert bool(torch.isneginf(xf[k * per:min(V, (k + 1) * per)]).all()) and bool(torch.isfinite(xf[:k * per]).all()), (name, V)
    elif name == "hole_first":
        assert bool(torch.isneginf(xf[0])) and tok != 0, (name, V)
    elif name == "holes_every_7th":
        assert bool(torch.isneginf(xf[3::7]).all()) and int(torch.isneginf(lp.float()).sum()) == len(range(3, V, 7)), (name, V)


@functools.lru_cache(maxsize=None)
def head_rows():
    """-> {V: Head}.  Every case at every V of VS where it exists (so each one at a V % 8 == 0 and at a V % 8 != 0), every
    row inside the guard band, every promise of a named row asserted."""
    table = {}
    for vi, V in enumerate(VS):
        names, rows = [], []
        for ci, (name, build) in enumerate(_cases(V)):
            x = _banded(build, 100 * vi + ci + 1, f"{name} @ V={V}")
            names += name.split("|")
            rows.append(x)
        x = torch.cat(rows)
        lp, lse, band = exact_logprobs(x)
        assert float(band.min()) >= GUARD_BAND, (V, names[int(band.argmin())], float(band.min()))
        tok = O.argmax_first(lp)
        for b, name in enumerate(names):
            _assert_case(name, V, x[b], lp[b], int(tok[b]))
        table[V] = Head(V, tuple(names), x, lp, tok, lse, band)
    for name in {n for h in table.values() for n in h.names}:
        at = [V for V, h in table.items() if name in h.names]
        assert any(V % 8 == 0 for V in at) and any(V % 8 for V in at), (name, at)
    return table


@functools.lru_cache(maxsize=None)
def batch_rows(V: int, B: int):
    """B DISTINCT banded rows of one V for the wide-batch forms -> Head: the table's rows at that V (if any), then random rows
    of alternating widths"""
    tab = head_rows().get(V)
    names, rows = (list(tab.names), [tab.x]) if tab is not None else ([], [])
    n = len(names)
    assert n <= B
    for i in range(B - n):
        s = (1.5, 3.0, 8.0, 0.3)[i % 4]
        rows.append(_banded(lambda sd, s=s: _randn(V, sd, s), 50000 + 7 * V + i, f"batch row {i} @ V={V}"))
        names.append(f"batch_randn_x{s:g}_{i}")
    x = torch.cat(rows)
    assert len({bytes(r.view(torch.uint8).numpy().tobytes()) for r in x}) == B, "distinct rows"
    lp, lse, band = exact_logprobs(x)
    assert float(band.min()) >= GUARD_BAND
    return Head(V, tuple(names), x, lp, O.argmax_first(lp), lse, band)


def head_mismatch(head: Head, lp, tok):
    """THE comparison of both tests: -> [(row name, what)] for every row whose log-probs are not bit-identical to the exact
    ones or whose token is not argmax_first of them.  No tolerance."""
    lp, tok = lp.detach().cpu(), tok.detach().cpu().to(torch.int64)
    assert lp.shape == head.lp.shape and lp.dtype == BF and tok.shape == head.tok.shape
    bad = []
    for b, name in enumerate(head.names):
        diff = bits(lp[b]) != bits(head.lp[b])
        if bool(diff.any()):
            i = int(torch.nonzero(diff)[0])
            bad.append((name, f"{int(diff.sum())} of {head.V} log-probs differ, first at {i}: {float(lp[b, i])!r} vs exact "
                              f"{float(head.lp[b, i])!r} (lse {float(head.lse[b]):.9g}, band {float(head.band[b]):.3g})"))
        if int(tok[b]) != int(head.tok[b]):
            bad.append((name, f"token {int(tok[b])} vs argmax_first {int(head.tok[b])}"))
    return bad


def check_head(form: str, head: Head, lp, tok):
    """assert head_mismatch finds nothing; one printed line per form and row (pytest -s shows them)"""
    bad = dict(head_mismatch(head, lp, tok))
    for b, name in enumerate(head.names):
        print(f"SAMPLER-EXACT {form:24s} V={head.V:<6d} {name:28s} "
              + (f"MISMATCH: {bad[name]}" if name in bad else f"bit-identical, token {int(head.tok[b])} (band {float(head.band[b]):.2e})"))
    assert not bad, (form, head.V, bad)


# ------------------------------------------------------------------ the kernels' own order in float32, and its mutants
MUTANTS = ("lse_f32", "lse_fp16", "drop_tail", "nan_block", "argmax_logits", "tie_last")


def emulate_head(x: torch.Tensor, mutant=None):
    """x bf16 [B, V] -> (lp bf16 [B, V], tok int64 [B]) in the order of lse_partial_kernel + logprob_argmax_kernel, float32:
    64 block partials (m_i, s_i = sum exp(x - m_i)) over `per` elements, merged as sum s_i * exp(m_i - m), lse = bf16(m + log s),
    lp = bf16(x - lse), token = the first index of the largest lp.  mutant: one of MUTANTS - the same code, subtly wrong."""
    assert mutant is None or mutant in MUTANTS
    B, V = x.shape
    per = block_per(V)
    xs = x.float().numpy()
    lps, toks = [], []
    f32 = np.float32
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for b in range(B):
            r = xs[b]
            Vs = V - V % 8 if mutant == "drop_tail" else V          # (the ragged end never reaches the sum)
            pm, ps = np.full(NBLK, -np.inf, f32), np.zeros(NBLK, f32)
            for k in range(NBLK):
                lo, hi = k * per, min(Vs, k * per + per)
                if hi <= lo:
                    continue
                pm[k] = r[lo:hi].max()
                if pm[k] > -np.inf or mutant == "nan_block":        # (exp(-inf - -inf) = NaN without the guard)
                    ps[k] = np.exp(r[lo:hi] - pm[k], dtype=f32).sum(dtype=f32)
            m = pm.max()
            w = ps * np.exp(pm - m, dtype=f32)
            if mutant != "nan_block":
                w = np.where(pm > -np.inf, w, f32(0))
            lse = f32(m + np.log(w.sum(dtype=f32), dtype=f32))
            if mutant == "lse_fp16":
                lse = f32(np.float16(lse))
            elif mutant != "lse_f32":
                lse = torch.tensor([lse], dtype=torch.float32).to(BF).float().numpy()[0]
            lp = torch.from_numpy((r - lse).astype(f32)).to(BF)
            key = x[b].float() if mutant == "argmax_logits" else lp.float()
            hit = torch.nonzero(key == key.max()).flatten()
            toks.append(int(hit[-1] if mutant == "tie_last" else hit[0]) if hit.numel() else 0)
            lps.append(lp)
    return torch.stack(lps), torch.tensor(toks, dtype=torch.int64)


# ------------------------------------------------------------------ the draw
def old_hash_uniform(seed, step, row, idx):
    """oracle.hash_uniform as it was before the clamp (and as csrc/sample.hip computed it): returns exactly 1.0 where
    x >> 8 == 0xFFFFFF.  Kept for the tests that show what the clamp repairs; nothing else may call it."""
    M = np.uint64(0xFFFFFFFF)
    x = (np.uint64(seed) ^ np.uint64(0x9E3779B9)) & M
    x = (x + (np.uint64(step) + np.uint64(1)) * np.uint64(0x85EBCA6B)) & M
    x = (x ^ ((np.uint64(row) + np.uint64(1)) * np.uint64(0xC2B2AE35))) & M
    x = (x + np.asarray(idx).astype(np.uint64) * np.uint64(0x27D4EB2F)) & M
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M
    x ^= x >> np.uint64(16)
    return ((x >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


# (seed, step, row, index, V): elements whose old uniform was exactly 1.0, and the dominant token of the peaked row drawn there
U_ONE_CASES = ((85, 46, 0, 103, 4096, 1000), (7, 66, 0, 77877, 151936, 5000))


@functools.lru_cache(maxsize=None)
def peaked_row(V: int, dominant: int):
    """one logit 40 over N(0, 1): the best token has p = 1 - 1e-12 -> (x bf16 [1, V], exact lp bf16 [1, V])"""
    def build(sd):
        x = _randn(V, sd)
        x[dominant] = 40.0
        return x

    x = _banded(build, 7000 + V, f"peaked row @ V={V}")
    return x, exact_logprobs(x)[0]


TABLE_DRAW = (17, 3, 0.8)             # (seed, step, temperature) of the one draw over every row of the table
DRAW_STEPS = 30
DRAW_TEMP = 0.8
DRAW_SEED = 29


@functools.lru_cache(maxsize=None)
def draw_cases():
    """-> {name: dict(V, x bf16 [B, V] logits, kw: the filter arguments of ops.sample / oracle.sampler_filters)}.  Every case
    is drawn DRAW_STEPS times at DRAW_TEMP; on all of them the smallest gap stays above DRAW_MARGIN (asserted by both tests:
    on the CPU over the oracle's filtered rows, on the GPU over the kernel's own)."""
    cases = {}

    def rows(V, seed, B, holes=False):
        out = []
        for b in range(B):
            def build(sd, b=b):
                x = _randn(V, sd, (2.0, 1.5, 3.0)[b % 3])
                if holes:
                    per, nb = block_per(V), (V + block_per(V) - 1) // block_per(V)
                    x[3::7] = NEG_INF
                    x[(nb // 3) * per:(nb // 3 + 1) * per] = NEG_INF
                return x
            out.append(_banded(build, seed + 31 * b, f"draw row {b} @ V={V}"))
        return torch.cat(out)

    for V, B in ((4099, 3), (32003, 3), (151936, 2)):
        cases[f"temperature_only-V{V}"] = dict(V=V, x=rows(V, 9100 + V, B), kw={})
        cases[f"holes-V{V}"] = dict(V=V, x=rows(V, 9200 + V, B, holes=True), kw={})
        cases[f"top_k-V{V}"] = dict(V=V, x=rows(V, 9300 + V, B), kw=dict(top_k=40))       # (V = 151936: the split path)
    for V, B in ((32003, 2), (151936, 2)):                                              # (one-workgroup kernel / split path)
        cases[f"top_p_min_p-V{V}"] = dict(V=V, x=rows(V, 9400 + V, B), kw=dict(top_p=0.9, min_p=0.02))
    return cases


def check_draws(name, rows, toks=None, seed=DRAW_SEED, temp=DRAW_TEMP, steps=DRAW_STEPS):
    """rows bf16 [B, V]: what the draw runs over.  Every (step, row) draw has gap > DRAW_MARGIN (a condition on the INPUTS)
    and, with toks int [steps, B] given, the kernel's token EQUALS the exact winner on every one.  -> the smallest gap."""
    B = rows.shape[0]
    worst, wrong = float("inf"), []
    for s in range(steps):
        for b in range(B):
            w, gap = exact_draw(rows[b], temp, seed, s, b)
            worst = min(worst, gap)
            if toks is not None and int(toks[s][b]) != w:
                wrong.append((s, b, int(toks[s][b]), w, gap))
    print(f"SAMPLER-EXACT draw {name:28s} {steps} steps x {B} rows: smallest gap {worst:.3e} (margin {DRAW_MARGIN:.3e})"
          + ("" if toks is None else f", {steps * B - len(wrong)} of {steps * B} tokens equal the exact winner"))
    assert worst > DRAW_MARGIN, (name, worst)
    assert not wrong, (name, wrong[:5])
    return worst
