"""The bars of the 8-bit prompt-chunk attention (tests/test_attn_q8_prefill_gpu.py) can fail, and the reference's own typed
graph meets them - on the CPU, over the table of tests/attn_q8_prefill_exact.py:

  * float64 mutants of a subtly wrong kernel (the scale off by 2^-8, the last visible key dropped, the first key of the last
    visible page dropped) are rejected by the existing "q8" class on every entry with a chunk of 64 rows or more.  The 5-row
    entry does not separate scale_2m8 (and the 1-row entry is the decode case, covered by test_attn_bars_cpu.py): they are
    left out of THIS claim only, the GPU test runs them;
  * the oracle's typed graph (oracle/quant.py quantized_sdpa, causal, bf16) passes the class on every entry - its distance is
    P's own bf16 rounding, the same thing that sets the decode class;
  * the C ABI declares the kernel and the Python layers bind it (this part needs the feature to exist)."""
import os
import re

import pytest

from tests import attn_exact as A
from tests import attn_q8_prefill_exact as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 128 ** -0.5


def _seed(i):
    return 3000 + 10 * i


@pytest.mark.parametrize("i", range(len(X.CASES)), ids=[X.case_id(c) for c in X.CASES])
def test_q8_prefill_bars_reject_the_mutants_and_pass_the_typed_graph(i):
    prefix, chunk, Hq, Hkv, outlier = X.CASES[i]
    q, k, v = X.inputs(prefix, chunk, Hq, Hkv, _seed(i), outlier)
    exact = X.prefill_q8_exact(q, k, v, prefix, SCALE)
    segs = [(0, chunk)]
    ok, rel, _, rep = A.measure(exact, exact, "q8", segs)
    assert ok and rel == 0.0, rep
    ok, rel, need, rep = A.measure(X.oracle_typed(q, k, v, SCALE), exact, "q8", segs)
    print(f"typed graph {X.case_id(X.CASES[i])}: {rep}")
    assert ok, ("the reference's typed graph", rep)
    if chunk < 64:
        return
    for d in A.CATCHES["q8"]:
        ok, _, _, rep = A.measure(X.prefill_q8_exact(q, k, v, prefix, SCALE, defect=d), exact, "q8", segs)
        assert not ok, (d, rep)


def test_the_c_abi_and_the_python_layers_expose_the_kernel():
    hdr = open(os.path.join(ROOT, "include", "vlm_hip.h")).read()
    assert re.search(r"\bint\s+vlm_attn_prefill_paged_q8\s*\(", hdr)
    assert len(set(re.findall(r"\b(vlm_[a-z0-9_]+)\s*\(", hdr))) == 60
    from mlx_vlm_amd import _lib, ops

    assert "vlm_attn_prefill_paged_q8" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["vlm_attn_prefill_paged_q8"][1]) == 20
    assert set(re.findall(r"\b(vlm_[a-z0-9_]+)\s*\(", hdr)) == set(_lib.SIGNATURES)
    assert callable(ops.attn_prefill_paged_q8)
