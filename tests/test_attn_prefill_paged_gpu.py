"""ops.attn_prefill_paged - a prompt chunk attending straight over the bf16 paged KV pools (csrc/attn_prefill_paged.hip, the
attention of a warm prefix-cache admission) - against the exactly rounded result tests/attn_exact.py::prefill_exact(...,
causal=True, starts=prefixes), held to the existing "hilo" class (rel-rms 5e-4, 1 ulp, atol_rms 2e-3: every bf16 kernel at
D = 128).  The whole sequence (prefix and chunk) sits on pages of NaN-filled pools, scattered or in the identity layout: slots
past a row's own position, unused slots of the last page and pages the table does not name must not reach a result.  The shape
table is the 8-bit sibling's (tests/attn_q8_prefill_exact.py::CASES and MULTI) plus one GQA 7:1 case."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import attn_exact as A
from tests import attn_q8_prefill_exact as X

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = "cuda"
SCALE = 128 ** -0.5
CASES = list(X.CASES) + [(100, 77, 14, 2, False)]       # + GQA 7:1


@pytest.fixture(scope="module")
def vops():
    from mlx_vlm_amd import ops

    return ops


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def _pools(ks, vs, seed, identity=False):
    bt, kpool, vpool, _ = A.build_pools(ks, vs, seed=seed, identity=identity, fill=float("nan"))
    return bt.cuda(), kpool.cuda(), vpool.cuda()


def _launch(vops, q, pools, seg_seq, chunks, prefixes, Hq, Hkv):
    btd, kp, vp = pools
    cu = np.concatenate([[0], np.cumsum(chunks)]).tolist()
    nqb = sum((n + vops.PAGED_PREFILL_QBLOCK - 1) // vops.PAGED_PREFILL_QBLOCK for n in chunks)
    out = torch.full((q.shape[0], Hq * X.D), 7.0, dtype=BF, device=DEV)
    vops.attn_prefill_paged(q.reshape(q.shape[0], -1).cuda(), kp, vp, btd, _i32(seg_seq), _i32(cu), _i32(prefixes), nqb, Hq, Hkv, X.D,
                            SCALE, out=out)
    return out.cpu().view(q.shape[0], Hq, X.D)


def _exact(q, k, v, prefix):
    """the chunk's rows of prefill_exact over [prefix | chunk] with starts = [prefix] (the prefix rows are keys only)"""
    full_q = torch.cat([torch.zeros(prefix, *q.shape[1:], dtype=BF), q])
    return A.prefill_exact(full_q, k, v, [k.shape[0]], SCALE, True, starts=[prefix], dev=DEV)[prefix:]


def _gather_path(vops, q, ks, vs, pools, seg_order, chunks, prefixes, Hq, Hkv):
    """the path the op replaces: ops.kv_gather_ into a full-length token-major buffer + ops.attn_prefill(q_start=)"""
    btd, kp, vp = pools
    D = X.D
    tot = [p + c for p, c in zip(prefixes, chunks)]
    cu_full = np.concatenate([[0], np.cumsum(tot)]).astype(np.int32)
    full = torch.zeros(int(cu_full[-1]), (Hq + 2 * Hkv) * D, dtype=BF, device=DEV)
    new_rows = np.concatenate([np.arange(cu_full[i] + prefixes[i], cu_full[i + 1]) for i in range(len(tot))])
    full[torch.from_numpy(new_rows).cuda(), : Hq * D] = q.reshape(q.shape[0], -1).cuda()
    seq = np.concatenate([np.full(tot[i], seg_order[i], np.int32) for i in range(len(tot))])
    slot = np.concatenate([np.arange(tot[i], dtype=np.int32) for i in range(len(tot))])
    vops.kv_gather_(full, Hq, Hkv, D, _i32(slot), btd, kp, vp, kv_seq=_i32(seq))
    nqb = sum((c + 127) // 128 for c in chunks)
    att = vops.attn_prefill(full, full[:, Hq * D:], full[:, (Hq + Hkv) * D:], _i32(cu_full), nqb, Hq, Hkv, D, SCALE, True,
                            q_start=_i32(prefixes))
    return att[torch.from_numpy(new_rows).cuda()].cpu().view(q.shape[0], Hq, D)


@pytest.mark.parametrize("identity", [False, True])
@pytest.mark.parametrize("i", range(len(CASES)), ids=[X.case_id(c) for c in CASES])
def test_paged_prefill_exact(vops, i, identity):
    """the table: from a first chunk (no prefix) and a 1-row chunk up to 257 rows onto 4100 cached tokens, G = 2 .. 7, page and
    32-key unit edges on both sides; two launches give identical bits"""
    prefix, chunk, Hq, Hkv, outlier = CASES[i]
    q, k, v = X.inputs(prefix, chunk, Hq, Hkv, 5000 + 10 * i, outlier)
    pools = _pools([k], [v], seed=5100 + i, identity=identity)
    out = _launch(vops, q, pools, [0], [chunk], [prefix], Hq, Hkv)
    assert bool(torch.isfinite(out.float()).all())
    A.check(f"paged prefill {X.case_id(CASES[i])} {'identity' if identity else 'scattered pages'}", out, _exact(q, k, v, prefix),
            "hilo", [(0, chunk)])
    again = _launch(vops, q, pools, [0], [chunk], [prefix], Hq, Hkv)
    assert torch.equal(out.view(torch.int16), again.view(torch.int16))


def _multi():
    Hq, Hkv, segs, seg_seq = X.MULTI["Hq"], X.MULTI["Hkv"], X.MULTI["segs"], X.MULTI["seg_seq"]
    data = [X.inputs(p, c, Hq, Hkv, 5300 + 10 * s, outlier=(s == 1)) for s, (p, c) in enumerate(segs)]
    order = sorted(range(len(segs)), key=lambda s: seg_seq[s])          # sequence seg_seq[s] of the pools holds segment s
    return Hq, Hkv, segs, seg_seq, data, order


def test_paged_prefill_three_segments_in_one_launch(vops):
    """three sequences of different prefix / chunk lengths, their block-table rows out of order"""
    Hq, Hkv, segs, seg_seq, data, order = _multi()
    pools = _pools([data[s][1] for s in order], [data[s][2] for s in order], seed=5400)
    q = torch.cat([d[0] for d in data])
    chunks, prefixes = [c for _, c in segs], [p for p, _ in segs]
    out = _launch(vops, q, pools, seg_seq, chunks, prefixes, Hq, Hkv)
    assert bool(torch.isfinite(out.float()).all())
    exact = torch.cat([_exact(d[0], d[1], d[2], p) for d, (p, _) in zip(data, segs)])
    cu = np.concatenate([[0], np.cumsum(chunks)])
    segments = [(int(cu[s]), int(cu[s + 1])) for s in range(len(segs))]
    A.check("paged prefill, 3 segments in one launch", out, exact, "hilo", segments)
    # ... and the path it replaces (gather + attn_prefill(q_start=)) within the same bar: the summation order differs
    gathered = _gather_path(vops, q, None, None, pools, seg_seq, chunks, prefixes, Hq, Hkv)
    A.check("paged prefill vs gather path, 3 segments", out, gathered, "hilo", segments)


@pytest.mark.parametrize("i", [1, 4], ids=[X.case_id(CASES[1]), X.case_id(CASES[4])])
def test_paged_prefill_agrees_with_gather_path(vops, i):
    prefix, chunk, Hq, Hkv, outlier = CASES[i]
    q, k, v = X.inputs(prefix, chunk, Hq, Hkv, 5600 + 10 * i, outlier)
    pools = _pools([k], [v], seed=5700 + i)
    out = _launch(vops, q, pools, [0], [chunk], [prefix], Hq, Hkv)
    gathered = _gather_path(vops, q, None, None, pools, [0], [chunk], [prefix], Hq, Hkv)
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(gathered.float()).all())
    A.check(f"paged prefill vs gather path {X.case_id(CASES[i])}", out, gathered, "hilo", [(0, chunk)])


def test_paged_prefill_q_inside_a_qkv_buffer(vops):
    """q with a row stride beyond Hq * D (the q columns of a qkv buffer): only the chunk's rows and columns are read"""
    prefix, chunk, Hq, Hkv = 70, 40, 12, 2
    q, k, v = X.inputs(prefix, chunk, Hq, Hkv, 5800)
    btd, kp, vp = _pools([k], [v], seed=5801)
    qkv = torch.full((chunk, (Hq + 2 * Hkv) * X.D), float("nan"), dtype=BF, device=DEV)
    qkv[:, : Hq * X.D] = q.reshape(chunk, -1).cuda()
    out = vops.attn_prefill_paged(qkv, kp, vp, btd, _i32([0]), _i32([0, chunk]), _i32([prefix]), 1, Hq, Hkv, X.D, SCALE)
    A.check("paged prefill, q inside a qkv buffer", out.cpu().view(chunk, Hq, X.D), _exact(q, k, v, prefix), "hilo", [(0, chunk)])


def test_paged_prefill_argument_checks(vops):
    from mlx_vlm_amd import _lib

    q, k, v = X.inputs(0, 5, 4, 2, 5900)
    btd, kp, vp = _pools([k], [v], seed=5901)
    qd = q.reshape(5, -1).cuda()
    with pytest.raises(ValueError):
        vops.attn_prefill_paged(qd, kp, vp, btd, _i32([0]), _i32([0, 5, 9]), _i32([0]), 1, 4, 2, X.D, SCALE)
    with pytest.raises(RuntimeError):
        vops.attn_prefill_paged(qd, kp, vp, btd, _i32([0]), _i32([0, 5]), _i32([0]), 1, 4, 3, X.D, SCALE)     # Hq % Hkv
    # ONE NULL scale pointer through the raw symbol: neither the 8-bit nor the bf16 form
    out = torch.empty(5, 4 * X.D, dtype=BF, device=DEV)
    words = torch.zeros(kp.numel() // 64, dtype=torch.int32, device=DEV)
    seg, cu, qs = _i32([0]), _i32([0, 5]), _i32([0])
    p = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
    for ksb, vsb in ((p(words), None), (None, p(words))):
        rc = _lib.lib().vlm_attn_prefill_paged_q8(p(qd), qd.stride(0), p(out), out.stride(0), p(kp), p(vp), ksb, vsb, p(btd),
                                                  btd.shape[1], p(seg), p(cu), p(qs), 1, 1, 4, 2, X.D, SCALE, None)
        assert rc == 1, rc
    torch.cuda.synchronize()
