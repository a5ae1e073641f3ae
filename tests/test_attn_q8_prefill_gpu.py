"""vlm_attn_prefill_paged_q8 - a prompt chunk attending over the uniform 8-bit KV cache - against the exactly rounded result
(tests/attn_q8_prefill_exact.py), held to the existing "q8" class of tests/attn_exact.py (rel-rms 3e-3, 2 ulps, atol_rms 2e-2:
the class of the 8-bit decode kernel, which the reference's own typed graph meets on this table - see
tests/test_attn_q8_prefill_bars_cpu.py).  The whole sequence (prefix and chunk) is written to NaN-filled bf16 pools on shuffled
pages and quantised with vlm_kv_quantize_tokens into 8-bit pools whose every other byte / (scale | bias) word is a NaN
pattern: slots past a row's own position, unused slots of the last page and pages the table does not name must not reach a
result.  Also the row produced by the reference's own files (tests/golden/kvquant_ref.npz: 4 rows onto 2 cached)."""
import os

import numpy as np
import pytest
import torch

from tests import attn_exact as A
from tests import attn_q8_prefill_exact as X
from tests.helpers import bf16_close

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = "cuda"
SCALE = 128 ** -0.5
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kvquant_ref.npz")


@pytest.fixture(scope="module")
def vops():
    from mlx_vlm_amd import ops

    return ops


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def _quantised_pools(vops, ks, vs, seed, identity=False):
    """every token of the sequences ks / vs on (shuffled) pages of NaN-filled pools, quantised -> (bt, k8, v8, ksb, vsb)"""
    Hkv = ks[0].shape[1]
    bt, kpool, vpool, _ = A.build_pools(ks, vs, seed=seed, identity=identity)
    k8, v8, ksb, vsb = X.nan_q8_pools(kpool)
    seq = torch.cat([torch.full((k.shape[0],), b, dtype=torch.int32) for b, k in enumerate(ks)])
    slot = torch.cat([torch.arange(k.shape[0], dtype=torch.int32) for k in ks])
    btd = bt.cuda()
    vops.kv_quantize_tokens(kpool.cuda(), vpool.cuda(), k8, v8, ksb, vsb, seq.cuda(), slot.cuda(), btd, Hkv, X.D)
    return btd, k8, v8, ksb, vsb


def _launch(vops, q, pools, seg_seq, chunks, prefixes, Hq, Hkv):
    btd, k8, v8, ksb, vsb = pools
    cu = np.concatenate([[0], np.cumsum(chunks)]).tolist()
    nqb = sum((n + vops.Q8_PREFILL_QBLOCK - 1) // vops.Q8_PREFILL_QBLOCK for n in chunks)
    out = torch.full((q.shape[0], Hq * X.D), 7.0, dtype=BF, device=DEV)
    vops.attn_prefill_paged_q8(q.reshape(q.shape[0], -1).cuda(), k8, v8, ksb, vsb, btd, _i32(seg_seq), _i32(cu), _i32(prefixes), nqb,
                               Hq, Hkv, X.D, SCALE, out=out)
    return out.cpu().view(q.shape[0], Hq, X.D)


@pytest.mark.parametrize("identity", [False, True])
@pytest.mark.parametrize("i", range(len(X.CASES)), ids=[X.case_id(c) for c in X.CASES])
def test_q8_prefill_exact(vops, i, identity):
    """the table: from a first chunk (no prefix) and a 1-row chunk up to 257 rows onto 4100 cached tokens, G = 2 .. 7, page and
    32-key unit edges on both sides, outlier channels; two launches give identical bits"""
    prefix, chunk, Hq, Hkv, outlier = X.CASES[i]
    q, k, v = X.inputs(prefix, chunk, Hq, Hkv, 3000 + 10 * i, outlier)
    pools = _quantised_pools(vops, [k], [v], seed=3100 + i, identity=identity)
    out = _launch(vops, q, pools, [0], [chunk], [prefix], Hq, Hkv)
    A.check(f"q8 prefill {X.case_id(X.CASES[i])} {'identity' if identity else 'scattered pages'}", out,
            X.prefill_q8_exact(q, k, v, prefix, SCALE, dev=DEV), "q8", [(0, chunk)])
    again = _launch(vops, q, pools, [0], [chunk], [prefix], Hq, Hkv)
    assert torch.equal(out.view(torch.int16), again.view(torch.int16))


def test_q8_prefill_three_segments_in_one_launch(vops):
    """three sequences of different prefix / chunk lengths, their block-table rows out of order"""
    Hq, Hkv, segs, seg_seq = X.MULTI["Hq"], X.MULTI["Hkv"], X.MULTI["segs"], X.MULTI["seg_seq"]
    data = [X.inputs(p, c, Hq, Hkv, 3300 + 10 * s, outlier=(s == 1)) for s, (p, c) in enumerate(segs)]
    # sequence seg_seq[s] of the pools holds segment s
    order = sorted(range(len(segs)), key=lambda s: seg_seq[s])
    pools = _quantised_pools(vops, [data[s][1] for s in order], [data[s][2] for s in order], seed=3400)
    q = torch.cat([d[0] for d in data])
    chunks, prefixes = [c for _, c in segs], [p for p, _ in segs]
    out = _launch(vops, q, pools, seg_seq, chunks, prefixes, Hq, Hkv)
    exact = torch.cat([X.prefill_q8_exact(d[0], d[1], d[2], p, SCALE, dev=DEV) for d, (p, _) in zip(data, segs)])
    cu = np.concatenate([[0], np.cumsum(chunks)])
    A.check("q8 prefill, 3 segments in one launch", out, exact, "q8", [(int(cu[s]), int(cu[s + 1])) for s in range(len(segs))])


def test_q8_prefill_rows_of_other_segments_and_strides(vops):
    """q / out with a row stride beyond Hq * D (the q columns of a qkv buffer): only the chunk's rows and columns are touched"""
    prefix, chunk, Hq, Hkv = 70, 40, 12, 2
    q, k, v = X.inputs(prefix, chunk, Hq, Hkv, 3500)
    btd, k8, v8, ksb, vsb = _quantised_pools(vops, [k], [v], seed=3501)
    qkv = torch.full((chunk, (Hq + 2 * Hkv) * X.D), float("nan"), dtype=BF, device=DEV)
    qkv[:, : Hq * X.D] = q.reshape(chunk, -1).cuda()
    out = vops.attn_prefill_paged_q8(qkv, k8, v8, ksb, vsb, btd, _i32([0]), _i32([0, chunk]), _i32([prefix]), 1, Hq, Hkv, X.D, SCALE)
    A.check("q8 prefill, q inside a qkv buffer", out.cpu().view(chunk, Hq, X.D), X.prefill_q8_exact(q, k, v, prefix, SCALE, dev=DEV),
            "q8", [(0, chunk)])


def test_q8_prefill_golden_row_of_the_reference(vops):
    """the fixture the reference's own files produced: quantise k1 | k2 and v1 | v2 (6 tokens), run q_multi (4 rows onto 2
    cached) and compare with its quantized_scaled_dot_product_attention under the causal mask - the oracle assertion and bars of
    tests/test_ops_gpu.py::test_attn_decode_paged_q8_vs_oracle (2 ulps + 2 % of the rms)"""
    R = np.load(GOLD)
    bf = lambda a: torch.from_numpy(np.asarray(a)).to(BF)           # noqa: E731
    k = torch.cat([bf(R["op.k1"]), bf(R["op.k2"])], dim=2)[0].permute(1, 0, 2).contiguous()      # [6, 2, 128]
    v = torch.cat([bf(R["op.v1"]), bf(R["op.v2"])], dim=2)[0].permute(1, 0, 2).contiguous()
    q = bf(R["op.q_multi"])[0].permute(1, 0, 2).contiguous()                                       # [4, 4, 128]
    ref = bf(R["op.sdpa_causal"])[0].permute(1, 0, 2)
    L, Hq, Hkv = q.shape[0], q.shape[1], k.shape[1]
    prefix = k.shape[0] - L
    assert (L, prefix) == (4, 2)
    pools = _quantised_pools(vops, [k], [v], seed=3600)
    out = _launch(vops, q, pools, [0], [L], [prefix], Hq, Hkv)
    ok, rep = bf16_close(out, ref, ulps=2, atol_rms=2e-2)
    assert ok, rep
    A.check("q8 prefill, golden row", out, X.prefill_q8_exact(q, k, v, prefix, SCALE, dev=DEV), "q8", [(0, L)])


def test_q8_prefill_argument_checks(vops):
    q, k, v = X.inputs(0, 5, 4, 2, 3700)
    btd, k8, v8, ksb, vsb = _quantised_pools(vops, [k], [v], seed=3701)
    qd = q.reshape(5, -1).cuda()
    with pytest.raises(ValueError):
        vops.attn_prefill_paged_q8(qd, k8, v8, ksb, vsb, btd, _i32([0]), _i32([0, 5, 9]), _i32([0]), 1, 4, 2, X.D, SCALE)
    with pytest.raises(RuntimeError):
        vops.attn_prefill_paged_q8(qd, k8, v8, ksb, vsb, btd, _i32([0]), _i32([0, 5]), _i32([0]), 1, 4, 3, X.D, SCALE)     # Hq % Hkv
