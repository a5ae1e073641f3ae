"""The attention bars can fail: for every case of the shared shape tables (tests/attn_exact.py), the float64 mutants of a
subtly wrong kernel - scale / logits / log2(e) / P / denominator at a lower precision, the scale off by 2^-8, one key
dropped at the end of what a query sees or at the first slot of its last page - are rounded to bf16 like a kernel output
and handed to the checker of the case's class.  The class must reject every mutant it is meant to catch (attn_exact.CATCHES);
one bf16 P operand is what the "single" class exists for and must pass it."""
import pytest
import torch

from tests import attn_exact as A


def _verdicts(make_exact, cls, segments):
    exact = make_exact(None)
    ok, rel, _, rep = A.measure(exact, exact, cls, segments)
    assert ok and rel == 0.0, rep
    for d in A.CATCHES[cls]:
        mutant = make_exact(d)
        if d == "scale_bf16" and torch.equal(mutant, exact):
            continue                                    # a scale that IS a bf16 value (64 ** -0.5): nothing to catch
        ok, _, _, rep = A.measure(mutant, exact, cls, segments)
        assert not ok, (d, rep)
    if cls in ("single", "q8"):
        # (rel-rms only: this float64 model of one bf16 P rounds against the row's final max, a flash kernel against a
        # running one; the kernels' own elementwise numbers are measured on hardware)
        _, rel, _, rep = A.measure(make_exact("p_bf16"), exact, cls, segments)
        assert rel <= A.BARS[cls].rel_rms, ("p_bf16", rep)


def _decode_segments(B, Hq):
    return [(b, b + 1) for b in range(B)]


@pytest.mark.parametrize("case", A.DECODE_CASES, ids=A.case_id)
def test_decode_bars_reject_the_mutants(case):
    q, ks, vs = A.decode_inputs(case["lens"], case["Hq"], case["Hkv"], seed=1000 + case["G"])
    _verdicts(lambda d: A.decode_exact(q, ks, vs, 128 ** -0.5, defect=d), "hilo", _decode_segments(len(ks), case["Hq"]))


@pytest.mark.parametrize("case", A.PAD_DECODE_CASES, ids=A.case_id)
def test_padded_decode_bars_reject_the_mutants(case):
    q, ks, vs = A.decode_inputs(case["lens"], case["Hq"], case["Hkv"], seed=1100 + case["real"], real=case["real"])
    _verdicts(lambda d: A.decode_exact(q, ks, vs, case["real"] ** -0.5, real=case["real"], defect=d), "hilo",
              _decode_segments(len(ks), case["Hq"]))


@pytest.mark.parametrize("case", A.Q8_CASES, ids=A.case_id)
def test_q8_decode_bars_reject_the_mutants(case):
    q, ks, vs = A.decode_inputs(case["lens"], case["Hq"], case["Hkv"], seed=1200 + case["G"], kscale=0.8, outlier=True)
    _verdicts(lambda d: A.decode_q8_exact(q, ks, vs, 128 ** -0.5, defect=d), "q8", _decode_segments(len(ks), case["Hq"]))


def _prefill(case, seed, starts=None):
    D, real = case["D"], case.get("real")
    q, k, v = A.prefill_inputs(case["lens"], case["Hq"], case["Hkv"], D, seed=seed, real=real)
    is_q, segs = A.query_rows(case["lens"], starts)
    cls = A.prefill_class(D)

    def make(d):
        return A.prefill_exact(q, k, v, case["lens"], (real or D) ** -0.5, case["causal"], starts=starts, real=real, defect=d)[is_q]

    _verdicts(make, cls, segs)


@pytest.mark.parametrize("case", A.PREFILL_CASES, ids=A.case_id)
def test_prefill_bars_reject_the_mutants(case):
    _prefill(case, seed=1300 + case["D"] + case["G"])


@pytest.mark.parametrize("case", A.QSTART_CASES, ids=A.case_id)
def test_q_start_prefill_bars_reject_the_mutants(case):
    _prefill(case, seed=1400 + case["D"] + case["G"], starts=case["starts"])


@pytest.mark.parametrize("case", A.PAD_PREFILL_CASES, ids=A.case_id)
def test_padded_prefill_bars_reject_the_mutants(case):
    _prefill(case, seed=1500 + case["real"])


def test_rne_bf16_rounds_once_to_nearest_even():
    # 1 + 2^-8 is a tie between 1 and 1 + 2^-7: even -> 1; one fp32 ulp above it must round up (a cast through fp32 of
    # 1 + 2^-8 + 2^-40 would first land on the tie and then go down)
    x = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -40, -3.0, 0.0], dtype=torch.float64)
    assert A.rne_bf16(x).tolist() == [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, -3.0, 0.0]
    y = torch.randn(10000, dtype=torch.float64)
    r = A.rne_bf16(y)
    assert torch.equal(r, r.to(torch.bfloat16).to(torch.float64))
    assert bool(((r - y).abs() <= 2.0 ** -8 * y.abs()).all())
