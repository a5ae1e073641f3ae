"""Decode projections at hidden sizes past 4096 (Qwen2-VL-72B: 8192), operator level.

The norm-prologue GEMVs (gate/up + SwiGLU, the head) and the qkv form with its bias + M-RoPE + paged-KV-write epilogue,
bf16 and MLX 4-bit weights, against oracle/ops.py chained exactly as tests/test_ops_gpu.py chains it and held to that
file's bars for the same operator: bf16_close(ulps=3) for norm + SwiGLU, ulps=2 for norm + head and for
qkv + rope + KV write with the "nothing else was written" count.  The bars carry over: fp32 accumulation over 8192 terms
adds error of order sqrt(K) * 2^-24, far under one bf16 ulp, and bf16_close's atol_rms term covers cancellation.

Shapes: K = 4224 (the first chunk past the register form of K <= 4096), 5120 (no multiple of 1024), 8192 (the limit);
1, 2, 4, 8 rows (the dot-product forms) and 5, 9, 16 rows (the matrix-core forms); N small.

Which launches exist past K = 4096 was decided by measurement (profiles/wide_hidden_decode.txt): on
the dot-product kernels the composition - vlm_rmsnorm_residual, the GEMV without a prologue (bf16: the split-K kernel, which
got a SwiGLU epilogue for this), the rotary + KV-write launch - beat a fused norm-prologue kernel everywhere except the
4-bit qkv form, which keeps its prologue up to K = 8192; the matrix-core forms (with the workspace: 8 rows of the qkv form
past K = 4096, 5..16 rows otherwise) take K <= 8192 as they are.  So every case holds the composition to the bar; a fused
entry either runs - then it is held to the same bar and compared with the composition - or must refuse with "unsupported
shape" and write nothing.

The inputs are drawn so that the oracle has one answer at fp32 (_inputs: no rsqrt-sensitive row, no qkv projection output
within fp32 summation error of a bf16 rounding tie); every comparison is tests/helpers.py::bf16_close, unchanged.

The long rows of a real 72B layer (K = 29568: the down projection) are at the end of the file.

The SuScaledRoPE (`long_from`) epilogue has no operator-level door - the C ABI's qkv entries take no long_from, the engine
passes it through the library-internal forms - so its cases at these widths are engine-level:
tests/test_wide_hidden_decode_gpu.py::test_su_rope_regime_at_hidden_8192.
"""
import functools

import pytest
import torch

from oracle import ops as O
from tests.attn_exact import VSLOT
from tests.helpers import bf16_close

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
KS = [4224, 5120, 8192]
I_GU, N_HEAD = 1024, 1000          # gate/up: 2 x 1024 rows; head: 1000 rows (not a multiple of 16: the padding path)
HQ, HKV, D = 8, 1, 128             # qkv: (8 + 2 * 1) * 128 rows, GQA 8 : 1


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


@pytest.fixture(scope="module")
def vops():
    from mlx_vlm_amd import ops

    return ops


def _refused(fn, codes=("rc=2 ",)):
    """-> (result, None), or (None, message) when the library answers "unsupported shape" (rc = 2); anything else raises"""
    from mlx_vlm_amd._lib import VlmHipError

    try:
        return fn(), None
    except VlmHipError as e:
        assert any(c in str(e) for c in codes), e
        return None, str(e)


def _composed(fn):
    """the GEMV without a prologue over normalised rows (None where the library refuses it)"""
    return _refused(fn)[0]


@functools.lru_cache(maxsize=None)
def _qkv_weights(K):
    return rnd((HQ + 2 * HKV) * D, K, seed=62, scale=0.05), rnd((HQ + 2 * HKV) * D, seed=63, scale=0.3)


@functools.lru_cache(maxsize=None)
def _qkv_exact(K, bits):
    """-> (w64 [N, K], b64 [N] or None): the qkv projection's exact operands in float64.  bf16: x W^T + b is rounded once;
    4-bit: the affine weights scale * q + bias, the matmul is rounded before the bias add (a second typed op), so the tie
    question is the matmul's alone"""
    from oracle import quant as Q

    if bits == 16:
        w, b = _qkv_weights(K)
        return w.double(), b.double()
    ws = []
    for n, seed in ((HQ * D, 230), (HKV * D, 231), (HKV * D, 232)):
        wq, sc, bi = Q.quantize_affine(rnd(n, K, seed=seed, scale=0.05))
        ws.append((Q.unpack(wq, 4).double().view(n, K // 64, 64) * sc.double()[..., None] + bi.double()[..., None]).view(n, K))
    return torch.cat(ws, 0), None


def _tie_rows(xn, exact):
    """per row of xn: how many projection outputs have an exact value within 2^-22 of its magnitude - four fp32 ulps, what two
    fp32 summation orders of 8192 terms differ by - of a bf16 rounding tie.  There the fp32 oracle is not determined: its
    matmul gave -3.34375 and the fp32 dot product of the same row and column -3.359375 for an exact -3.35156268 (tie at
    -3.3515625; the kernels gave the correctly rounded -3.359375)."""
    w64, b64 = exact
    t = xn.double() @ w64.T
    if b64 is not None:
        t = t + b64
    e = t.abs().clamp_min(2.0 ** -126) * 2.0 ** -22
    return ((t - e).to(BF) != (t + e).to(BF)).sum(-1)


@functools.lru_cache(maxsize=None)
def _inputs(K):
    """activations of 16 rows, norm weight and the bf16 matrices of one K (shared by every case; never modified).

    The rows are the first 16 of 96 seeded ones for which the ORACLE ITSELF has one answer at fp32 (both criteria are computed
    from the reference alone, on the CPU):
      * its normalised row keeps its bits when its fp32 rsqrt moves by 2 ulps either way.  A row whose 1 / rms makes many
        products x * inv land on rounding ties (row 4 of the plain draw at K = 8192: 72 of 8192 elements flip with ONE ulp of
        inv, and with them 1 in 4 of that row's projection outputs) measures the rsqrt's last bit, not a projection;
      * none of its qkv projection outputs, bf16 or 4-bit weights, is a near-tie (_tie_rows; about one output in 4000 is, so
        about half of the rows qualify).  Behind the rotation's cancellation one ulp of such an output (0.0156) is a rotated
        output of 0.21 off by 0.0127 against bf16_close's bound of 0.0122."""
    cand = rnd(96, K, seed=10)
    xf = cand.float()
    inv = torch.rsqrt((xf * xf).mean(-1, keepdim=True) + 1e-6)
    base = (xf * inv).to(BF)
    stable = torch.ones(96, dtype=torch.bool)
    for toward in (0.0, 2.0):
        p = inv
        for _ in range(2):
            p = torch.nextafter(p, torch.full_like(p, toward))
        stable &= ((xf * p).to(BF) == base).all(-1)
    nw = (1 + 0.1 * torch.randn(K, generator=torch.Generator().manual_seed(11))).to(BF)
    xn = O.rms_norm(cand, nw, 1e-6)
    stable &= (_tie_rows(xn, _qkv_exact(K, 16)) == 0) & (_tie_rows(xn, _qkv_exact(K, 4)) == 0)
    h = cand[stable][:16].contiguous()
    assert h.shape[0] == 16, int(stable.sum())
    wgu = rnd(2 * I_GU, K, seed=12, scale=0.05)
    wh = rnd(N_HEAD, K, seed=13, scale=0.05)
    wqkv, bqkv = _qkv_weights(K)
    return h, nw, wgu, wh, wqkv, bqkv


@functools.lru_cache(maxsize=None)
def _q4(N, K, seed):
    """-> (oracle QW, device QuantW) of one seeded matrix, quantized the way mx.quantize does (oracle/quant.py)"""
    from mlx_vlm_amd.models import quantized as Qz
    from oracle import quant as Q

    w = rnd(N, K, seed=seed, scale=0.05)
    wq, s, b = Q.quantize_affine(w)
    dq = Qz.take({"p.weight": wq.view(torch.uint32), "p.scales": s, "p.biases": b}, "p")
    return Q.QW(wq, s, b), dq.to("cuda")


# rows whose fused norm-prologue launch (gate/up, head) must exist: the matrix-core forms with their workspace at K <= 8192
# (4-bit: K in whole chunks of 256)
def _must_fuse(M, bits, ws, K):
    return ws and M >= 5 and (bits == 16 or K % 256 == 0)


def _judge(fused, comp, ref, ulps, must_fuse, why):
    """each form that exists against the oracle at the operator's bar, the two against each other at 2 ulps"""
    assert fused is not None or not must_fuse, why
    for name, got in (("fused", fused), ("composition", comp)):
        if got is not None:
            ok, rep = bf16_close(got, ref, ulps=ulps)
            print(f"    {name}: {rep}")
            assert ok, (name, rep)
    if fused is not None and comp is not None:
        ok, rep = bf16_close(fused, comp, ulps=2)
        assert ok, ("fused vs composition", rep)


@pytest.mark.parametrize("M", [1, 2, 4, 8, 5, 9, 16])
@pytest.mark.parametrize("K", KS)
def test_norm_prologue_swiglu_and_head_bf16(vops, M, K):
    h, nw, wgu, wh, _, _ = _inputs(K)
    h = h[:M]
    xn = O.rms_norm(h, nw, 1e-6)
    ref_gu = O.swiglu(O.linear(xn, wgu[0::2]), O.linear(xn, wgu[1::2]))
    ref_h = O.linear(xn, wh)
    hc, nwc, wguc, whc = h.cuda(), nw.cuda(), wgu.cuda(), wh.cuda()
    xnc = vops.rmsnorm(hc, nwc, eps=1e-6)
    for ws in (False, True):
        gemv = vops.gemv_ws if ws else vops.gemv
        if M not in (1, 2, 4, 8) and not ws:
            continue                 # 5, 9, 16 rows exist on the workspace entries only
        for w, ref, epi, ulps in ((wguc, ref_gu, vops.EPI_SWIGLU, 3), (whc, ref_h, vops.EPI_NONE, 2)):
            fused, why = _refused(lambda: gemv(hc, w, norm_w=nwc, eps=1e-6, epilogue=epi))
            comp = _composed(lambda: gemv(xnc, w, epilogue=epi))  # launches that exist at any K: the engine's fall-back
            print(f"bf16 M={M} K={K} ws={ws} epi={epi}: fused {'refused' if fused is None else 'runs'}, "
                  f"composition {'absent' if comp is None else 'runs'}")
            assert comp is not None, "the composition must exist for every row count"
            _judge(fused, comp, ref, ulps, _must_fuse(M, 16, ws, K), why)


@pytest.mark.parametrize("M", [1, 2, 4, 8, 5, 9, 16])
@pytest.mark.parametrize("K", KS)
def test_norm_prologue_swiglu_and_head_w4(vops, M, K):
    from mlx_vlm_amd.models import quantized as Qz

    h, nw = _inputs(K)[:2]
    h = h[:M]
    og, dg = _q4(I_GU, K, 222)
    ou, du = _q4(I_GU, K, 223)
    oh, dh = _q4(N_HEAD, K, 224)
    dgu = Qz.interleave_rows(dg, du)
    xn = O.rms_norm(h, nw, 1e-6)
    ref_gu = O.swiglu(og.linear(xn), ou.linear(xn))
    ref_h = oh.linear(xn)
    hc, nwc = h.cuda(), nw.cuda()
    xnc = vops.rmsnorm(hc, nwc, eps=1e-6)
    for ws in (False, True):
        gemv = vops.gemv_w4_ws if ws else vops.gemv_w4
        if M not in (1, 2, 4, 8) and not ws:
            continue
        for q, ref, epi, ulps in ((dgu, ref_gu, vops.EPI_SWIGLU, 3), (dh, ref_h, vops.EPI_NONE, 2)):
            fused, why = _refused(lambda: gemv(hc, q.wq, q.sb, norm_w=nwc, eps=1e-6, epilogue=epi))
            comp = _composed(lambda: gemv(xnc, q.wq, q.sb, epilogue=epi))
            print(f"w4 M={M} K={K} ws={ws} epi={epi}: fused {'refused' if fused is None else 'runs'}, "
                  f"composition {'absent' if comp is None else 'runs'}")
            assert comp is not None, "the composition must exist for every row count"
            _judge(fused, comp, ref, ulps, _must_fuse(M, 4, ws, K), why)


def _qkv_case(M):
    """positions, slots on both sides of a page boundary (63 | 64, 127 | 128), a scattered block table"""
    g = torch.Generator().manual_seed(64 + M)
    pos = torch.randint(0, 3000, (M,), generator=g, dtype=torch.int32)
    max_pages = 4
    slot = torch.tensor(([63, 64, 127, 128, 0, 255] * 3)[:M], dtype=torch.int32)
    n_pages = M * max_pages
    bt = torch.randperm(n_pages, generator=g).to(torch.int32).reshape(M, max_pages)
    return pos, slot, max_pages, n_pages, bt


def _check_qkv(out, kpool, vpool, qr, kr, vref, bt, slot, M, n_pages, what):
    ok, rep = bf16_close(out.view(M, HQ + 2 * HKV, D)[:, :HQ], qr, ulps=2)
    print(f"    {what}: q {rep}")
    assert ok, (what, rep)
    kp = kpool.cpu().permute(0, 1, 3, 2, 4).reshape(n_pages, HKV, 64, D)
    vp = vpool.cpu()[..., VSLOT].permute(0, 1, 3, 2)
    for m in range(M):
        page, within = int(bt[m, int(slot[m]) // 64]), int(slot[m]) % 64
        ok, rep = bf16_close(kp[page, :, within], kr[m], ulps=2)
        assert ok, (what, m, rep)
        ok, rep = bf16_close(vp[page, :, within], vref[m], ulps=2)
        assert ok, (what, m, rep)
    # nothing else was written
    assert int((kpool != 0).sum().cpu()) <= M * HKV * D and int((vpool != 0).sum().cpu()) <= M * HKV * D


@pytest.mark.parametrize("bits", [16, 4])
@pytest.mark.parametrize("M", [1, 2, 4, 8, 5, 9, 16])
@pytest.mark.parametrize("K", KS)
def test_qkv_rope_kvwrite(vops, M, K, bits):
    """[RMSNorm + qkv + bias + M-RoPE + paged KV write] at GQA 8 : 1, block-table and identity layouts (bit-equal to each
    other), and the three launches RMSNorm | projection + bias | rotary + KV write held to the same bar."""
    from mlx_vlm_amd.models import quantized as Qz

    h, nw, _, _, wqkv, bqkv = _inputs(K)
    h = h[:M]
    pos, slot, max_pages, n_pages, bt = _qkv_case(M)
    inv = O.mrope_inv_freq(D, 1e6)
    sel = O.chunked_position_selector([16, 24, 24], D // 2)
    xn = O.rms_norm(h, nw, 1e-6)
    if bits == 4:
        parts = [_q4(HQ * D, K, 230), _q4(HKV * D, K, 231), _q4(HKV * D, K, 232)]
        dq = Qz.cat_rows([p[1] for p in parts])
        bs = [bqkv[:HQ * D], bqkv[HQ * D:(HQ + HKV) * D], bqkv[(HQ + HKV) * D:]]
        qkv = torch.cat([p[0].linear(xn, b) for p, b in zip(parts, bs)], -1)
    else:
        qkv = O.linear(xn, wqkv, bqkv)
    # the rows were drawn so that the oracle's projection is determined: no output within fp32 summation error of a tie
    assert _tie_rows(xn, _qkv_exact(K, bits)).sum() == 0
    qkv = qkv.view(M, HQ + 2 * HKV, D)
    p3 = pos.long()[None, :, None].expand(3, M, 1)
    qr = O.mrope_apply(qkv[:, :HQ][:, :, None], p3, inv, sel, "fused")[:, :, 0]
    kr = O.mrope_apply(qkv[:, HQ:HQ + HKV][:, :, None], p3, inv, sel, "fused")[:, :, 0]
    vref = qkv[:, HQ + HKV:]
    hc, nwc, bc, posc, slotc, invc = h.cuda(), nw.cuda(), bqkv.cuda(), pos.cuda(), slot.cuda(), inv.cuda()
    wc = wqkv.cuda() if bits == 16 else None

    def pools():
        return (torch.zeros(n_pages, HKV, D // 8, 64, 8, dtype=BF, device="cuda"),
                torch.zeros(n_pages, HKV, D, 64, dtype=BF, device="cuda"))

    def fused(ws, table):
        kpool, vpool = pools()
        if bits == 4:
            f = vops.gemv_w4_qkv_rope_kvwrite_ws if ws else vops.gemv_w4_qkv_rope_kvwrite
            out = f(hc, nwc, dq.wq, dq.sb, bc, HQ, HKV, D, posc, slotc, invc, table, kpool, vpool, max_pages=max_pages)
        else:
            f = vops.gemv_qkv_rope_kvwrite_ws if ws else vops.gemv_qkv_rope_kvwrite
            out = f(hc, nwc, wc, bc, HQ, HKV, D, posc, slotc, invc, table, kpool, vpool, max_pages=max_pages)
        return out, kpool, vpool

    # the composition: RMSNorm, projection + bias, rotary + KV write (row m is sequence m at slot[m])
    xnc = vops.rmsnorm(hc, nwc, eps=1e-6)
    ws_rows = M not in (1, 2, 4, 8)
    if bits == 4:
        comp = (vops.gemv_w4_ws if ws_rows else vops.gemv_w4)(xnc, dq.wq, dq.sb, bias=bc, epilogue=vops.EPI_BIAS)
    else:
        comp = (vops.gemv_ws if ws_rows else vops.gemv)(xnc, wc, bias=bc, epilogue=vops.EPI_BIAS)
    ckpool, cvpool = pools()
    vops.mrope_kvwrite_(comp, HQ, HKV, D, posc, posc, posc, invc, 16, 24, kv_seq=torch.arange(M, dtype=torch.int32, device="cuda"),
                        kv_slot=slotc, block_table=bt.cuda(), kpool=ckpool, vpool=cvpool)
    print(f"qkv bits={bits} M={M} K={K}")
    _check_qkv(comp, ckpool, cvpool, qr, kr, vref, bt, slot, M, n_pages, "composition")

    ran = 0
    for ws in (False, True):
        if ws_rows and not ws:
            continue
        got, why = _refused(lambda: fused(ws, bt.cuda()))
        if got is None:
            # bf16 on the dot-product kernels past K = 4096: the composition ships; 5 rows: no qkv form at any K
            assert not (bits == 4 and M in (1, 2, 4, 8)), why
            print(f"    fused ws={ws}: refused")
            continue
        ran += 1
        out, kpool, vpool = got
        _check_qkv(out, kpool, vpool, qr, kr, vref, bt, slot, M, n_pages, f"fused ws={ws}")
        ok, rep = bf16_close(out[:, :HQ * D], comp[:, :HQ * D], ulps=2)
        assert ok, ("fused vs composition", rep)
        ok, rep = bf16_close(kpool, ckpool, ulps=2)
        assert ok, ("fused vs composition, k pool", rep)
        ok, rep = bf16_close(vpool, cvpool, ulps=2)
        assert ok, ("fused vs composition, v pool", rep)
        # identity layout == the block-table path over the same pages
        ident = torch.arange(n_pages, dtype=torch.int32).reshape(M, max_pages).cuda()
        a, b = fused(ws, ident), fused(ws, None)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        assert int((b[1] != 0).sum()) > 0
    # a fused qkv form must exist: 4-bit at 1, 2, 4, 8 rows (the dot-product kernel) and past that where K is whole chunks of
    # 256 (its matrix-core forms); bf16 from 8 rows on (the matrix-core forms).  5 rows have no qkv form at any K.
    if M != 5 and ((bits == 4 and (M <= 8 or K % 256 == 0)) or (bits == 16 and M >= 8)):
        assert ran > 0, "no fused qkv form took these rows"


@pytest.mark.parametrize("M", [1, 4, 16])
def test_k_8320_is_refused_and_enqueues_nothing(vops, M):
    """past the limit: every norm-prologue entry answers "unsupported shape" and leaves its outputs untouched"""
    from mlx_vlm_amd.models import quantized as Qz

    K = 8320
    h = rnd(M, K, seed=10).cuda()
    nw = torch.ones(K, dtype=BF, device="cuda")
    w = rnd(256, K, seed=12, scale=0.05).cuda()
    _, dq = _q4(256, K, 240)
    for ws in (False, True):
        if M == 16 and not ws:
            continue
        out = torch.full((M, 256), 7.0, dtype=BF, device="cuda")
        for call in (lambda: (vops.gemv_ws if ws else vops.gemv)(h, w, norm_w=nw, out=out),
                     lambda: (vops.gemv_w4_ws if ws else vops.gemv_w4)(h, dq.wq, dq.sb, norm_w=nw, out=out)):
            got, why = _refused(call)
            assert got is None, "K = 8320 was taken"
            torch.cuda.synchronize()
            assert bool((out == 7.0).all())
    # qkv: 1 + 2 * 1 heads of 128
    wq, bq = rnd(3 * D, K, seed=62, scale=0.05).cuda(), rnd(3 * D, seed=63, scale=0.3).cuda()
    dqq = Qz.cat_rows([_q4(D, K, 241)[1], _q4(D, K, 242)[1], _q4(D, K, 243)[1]])
    pos = torch.zeros(M, dtype=torch.int32, device="cuda")
    inv = O.mrope_inv_freq(D, 1e6).cuda()
    for ws in (False, True):
        if M == 16 and not ws:
            continue
        kpool = torch.zeros(M, 1, D // 8, 64, 8, dtype=BF, device="cuda")
        vpool = torch.zeros(M, 1, D, 64, dtype=BF, device="cuda")
        out = torch.full((M, 3 * D), 7.0, dtype=BF, device="cuda")
        f16 = vops.gemv_qkv_rope_kvwrite_ws if ws else vops.gemv_qkv_rope_kvwrite
        f4 = vops.gemv_w4_qkv_rope_kvwrite_ws if ws else vops.gemv_w4_qkv_rope_kvwrite
        for call in (lambda: f16(h, nw, wq, bq, 1, 1, D, pos, pos, inv, None, kpool, vpool, out=out, max_pages=1),
                     lambda: f4(h, nw, dqq.wq, dqq.sb, bq, 1, 1, D, pos, pos, inv, None, kpool, vpool, out=out, max_pages=1)):
            got, why = _refused(call)
            assert got is None, "K = 8320 was taken"
            torch.cuda.synchronize()
            assert bool((out == 7.0).all()) and int((kpool != 0).sum()) == 0 and int((vpool != 0).sum()) == 0


@pytest.mark.parametrize("bits", [16, 4])
@pytest.mark.parametrize("M", [1, 2, 4])
def test_down_projection_at_72b_length_k_29568(vops, M, bits):
    """h + act W^T at K = 29568 (the 72B intermediate size), N = 136 (not a multiple of 16), RESIDUAL epilogue, against
    oracle/ops at test_ops_gpu.py's bar for this operator (ulps=2): the split-K kernel at 15 chunks per thread (bf16, up to 4
    rows) and the 4-bit kernel at 15 chunks per lane.  4 rows over 4-bit weights stage 231 KiB of activations - more than a
    workgroup has - and must be refused with nothing written: the engine runs them as two launches of 2 rows, the same here."""
    K, N = 29568, 136
    act, res = rnd(M, K, seed=300), rnd(M, N, seed=301)
    if bits == 16:
        w = rnd(N, K, seed=302, scale=0.05)
        ref = O.add(res, O.linear(act, w))
        call = lambda a, r: vops.gemv(a, w.cuda(), res=r, out=r, epilogue=vops.EPI_RESIDUAL)
    else:
        ow, dw = _q4(N, K, 303)
        ref = O.add(res, ow.linear(act))
        call = lambda a, r: vops.gemv_w4(a, dw.wq, dw.sb, res=r, out=r, epilogue=vops.EPI_RESIDUAL)
    ac, rc = act.cuda(), res.cuda().clone()
    got, why = _refused(lambda: call(ac, rc))
    if bits == 4 and M == 4:
        assert got is None, "4 rows of 29568 do not fit a workgroup's staged activations"
        torch.cuda.synchronize()
        assert torch.equal(rc.cpu(), res)
        got = torch.cat([call(ac[:2].contiguous(), res[:2].cuda().clone()), call(ac[2:].contiguous(), res[2:].cuda().clone())])
    assert got is not None, why
    ok, rep = bf16_close(got, ref, ulps=2)
    print(f"down K=29568 bits={bits} M={M}: {rep}")
    assert ok, rep
