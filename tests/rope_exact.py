"""Lattice inputs, the exact rotation and the checker that the rotary / KV-write tests share.

Six kernels rotate q / k and write the paged KV pools (csrc/rope.hip, the qkv epilogues of gemv_bf16 / gemv_w4 / gemv_mfma /
gemv_mfma2, rope2d_vision).  A shape policy picks one from (rows, K, 4-bit, workspace); the caller cannot see which.  Held
against `GEMV + rope` of the oracle at 2 bf16 ulps, the GEMV's summation noise covers the rotation's own error.  Here the qkv
product is EXACT in every summation order (lattice_qkv), so the rotation, the pair addressing and the pool layout are all
that is left to differ, and they are held without a bf16-ulp tolerance:

    ex   the rotation in float64 of the kernels' contract - angle = fp32(fp32(pos) * inv_freq[f]) (ONE fp32 rounding), cos / sin
         of that fp32 value, z = bf16(y * qk_scale) where a scale applies, ex = z_d c - z_p s | z_p c + z_d s, NOT rounded
    bar  out is the correct bf16 rounding of SOME value within fp32 evaluation error of ex:
         rne_bf16(ex - delta) <= out <= rne_bf16(ex + delta),  delta = C * 2^-24 * (|z_d| + |z_p|)
         (where the two roundings are neighbours or equal - everywhere but under heavy cancellation - this says "out is one
         of the two"; under cancellation ex's own bf16 step is below delta and every bf16 value between them is the rounding
         of a value within delta)
    cap  at most CAP of a case's elements differ from rne_bf16(ex) at all

C = 4 is derived, not measured: 2 fp32 ulps each for sine and cosine (<= 2^-24 each in absolute terms, |sin|, |cos| <= 1),
half an ulp per product, half an ulp for the sum.  Honest fp32 evaluation on the CPU needs 0.44 on the case table (rot_report's
measure, see C_FP32 below) and leaves up to 9.2e-5 of a case's elements off rne_bf16(ex).

Imports without a GPU: tests/test_rope_exact_cpu.py builds mutants of a subtly wrong kernel from the same functions and case
tables and asserts that the checker rejects each of them."""
from __future__ import annotations

import functools
import math

import torch

from oracle import ops as O
from oracle import quant as Q
from tests.attn_exact import VSLOT, rne_bf16

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
PAGE = 64
C_FP32 = 4.0
# Worst seen on an MI355X over tests/test_rope_exact_gpu.py (c needed / share of elements != rne_bf16(ex)):
#   v_dot2c epilogues 0.20 / 8.1e-5 (bf16), 0.012 / 8.1e-5 (4-bit); first MFMA form 0.044 / 3.6e-5 (bf16), 0.14 / 3.6e-5 (4-bit);
#   second MFMA form 0.14 / 1.5e-5 (bf16), 0.14 / 3.6e-5 (4-bit); mrope_kvwrite_ 0.76 / 1.7e-4; rope2d_vision_ 0.28 / 2.0e-5
# ("c needed" is the distance from ex to the nearest value that rounds to the kernel's output, in units of 2^-24 * mag: 0 for
# every element that IS rne_bf16(ex), so it is set by the few elements that sit next to a rounding boundary)
CAP = 1e-3
SENTINEL = 0x5A5A                       # bf16 1.5e16: no lattice value, no rotation of one
EPS = 1e-6

# (Hq, Hkv, D, K, theta): the families' own head counts, so that the shape policy picks the forms the models get
GEOMETRIES = [
    (12, 2, 128, 1536, 1e6),            # Qwen2-VL-2B
    (28, 4, 128, 3584, 1e6),            # Qwen2-VL-7B
    (32, 8, 128, 4096, 1e4),            # Mistral: the only width at which the bf16 second MFMA form is chosen
    (32, 32, 96, 3072, 1e4),            # Phi-3.5: MHA, half >> 3 = 6 tiles per head
    (16, 16, 64, 1024, 1e6),            # nanoLLaVA
]
POSITIONS = [0, 1, 63, 4095, 4096, 32767, 131071, 1000003, 16777215, 2999]
MAX_PAGES = 4
SLOTS = [0, 63, 64, 127, 64 * MAX_PAGES - 1, 5, 100, 130, 200, 77, 191, 192, 33, 254, 128, 1]
SECTIONS = [(16, 24, 24), (10, 27, 27)]          # the second one is deliberately not aligned to the kernels' 8-wide chunks
QK_SCALE = 1.1875                                # 19 / 16: y * scale needs more than 8 bits for most lattice values


def geo_id(g):
    return f"Hq{g[0]}-Hkv{g[1]}-D{g[2]}-K{g[3]}"


# ------------------------------------------------------------------ lattice inputs
def assert_lattice(y: torch.Tensor, D: int):
    """y [rows, H, D] float64: multiples of 1/16 below 16 (exact in bf16), and an address swap is visible: the value at
    (head, d) differs from its neighbours (head, d + 1), (head + 1, d), (head, d + D/2) at >= 95 % of the positions"""
    assert y.dtype == F64 and y.shape[-1] == D
    assert bool((y * 16 == torch.round(y * 16)).all()) and float(y.abs().max()) < 16
    assert torch.equal(y.to(BF).to(F64), y)
    for name, other in (("d+1", torch.roll(y, -1, -1)), ("head+1", torch.roll(y, -1, -2)), ("d+D/2", torch.roll(y, D // 2, -1))):
        share = float((y != other).to(F64).mean(dim=(-1, -2)).min())
        assert share >= 0.95, (name, share)


def lattice_y(T, H, D, seed):
    """[T, H, D] float64 lattice values for the kernels that take a finished qkv buffer"""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(-255, 256, (T, H, D), generator=g).to(F64) / 16
    assert_lattice(y, D)
    return y


@functools.lru_cache(maxsize=1)
def _lattice16(Hq, Hkv, D, K, seed):
    """the 16-row build every row count of a geometry slices (rows 0 and 1 are negatives of each other, so every column
    is one where the rows of h differ whenever there is more than one row)"""
    M, N, G = 16, (Hq + 2 * Hkv) * D, K // 64
    assert K % 64 == 0 and G % 2 == 0
    g = torch.Generator().manual_seed(seed)
    h = (torch.randint(0, 2, (M, K), generator=g) * 2 - 1).to(F64)
    h[1] = -h[0]
    norm_w = torch.tensor([0.5, 1.0, 2.0], dtype=F64)[torch.randint(0, 3, (K,), generator=g)]
    # 4-bit anchors: two fixed columns of every 64-wide group hold -1 and 7/8 (-> scale 1/8, bias -1, lossless); their h
    # alternates in sign over the groups, identically in every row, and their norm weight is 1: the contribution cancels
    A0, A1 = 5, 42
    anchor = torch.zeros(K, dtype=torch.bool)
    anchor[A0::64] = True
    anchor[A1::64] = True
    sign = torch.tensor([1.0, -1.0], dtype=F64)[torch.arange(G) % 2]
    h[:, A0::64] = sign
    h[:, A1::64] = sign
    norm_w[anchor] = 1.0
    x = h * norm_w                                                          # the normalised activations, exactly
    # payload: four columns per output row, one per quarter of K (so every K split, wave and lane sees some), none an anchor
    free = torch.nonzero(~anchor).flatten()
    per = free.numel() // 4
    cols = torch.stack([free[q * per + torch.randint(0, per, (N,), generator=g)] for q in range(4)], 1)      # [N, 4]
    wk = torch.randint(-8, 8, (N, 4), generator=g).to(F64) / 8
    W = torch.zeros(N, K, dtype=BF)
    W[torch.arange(N)[:, None], cols] = wk.to(BF)
    n = torch.arange(N)
    bias = ((37 * n) % 193 - 96).to(F64) / 16
    terms = x[:, cols] * wk                                                 # [M, N, 4], multiples of 1/16
    y = bias + terms.sum(-1)
    # every partial sum, in any order and any split, is a sum of multiples of 1/16 bounded by this: exact in fp32
    bound = float(bias.abs().max() + terms.abs().sum(-1).max() + 2 * G)     # (+ the 4-bit anchors: at most 2 per group)
    assert bound * 16 < 2 ** 24
    # (the 4-bit kernels' affine form scale * (sum (128 + q) x - 128 sum x) + bias * sum x: a group's sums are multiples of
    # 1/2 below 64 * 143 * 2 < 2^15, scale and bias are powers of two - exact as well)
    assert bool((terms * 16 == torch.round(terms * 16)).all())
    W4 = W.clone()
    W4[:, A0::64] = -1.0
    W4[:, A1::64] = 7.0 / 8
    assert torch.equal(x[:, anchor] @ W4[:4, anchor].to(F64).T, torch.zeros(M, 4, dtype=F64))      # the anchors cancel
    return dict(h=h, norm_w=norm_w, x=x, W=W, W4=W4, bias=bias, y=y, cols=cols)


def lattice_qkv(M, Hq, Hkv, D, K, w4: bool, seed):
    """-> h [M, K] bf16 (+-1: mean square exactly 1), norm_w [K] bf16 ({0.5, 1, 2}), W (bf16 [N, K], or the packed 4-bit
    triple (wq, scales, biases) of oracle.quant.quantize_affine), bias [N] bf16, y [M, N] float64: the pre-rotation values
    RMSNorm(h) @ W.T + bias, which every kernel must produce EXACTLY whatever its K split and accumulation order."""
    b = _lattice16(Hq, Hkv, D, K, seed)
    h, nw, y = b["h"][:M].to(BF), b["norm_w"].to(BF), b["y"][:M]
    xn = O.rms_norm(h, nw, EPS)
    assert torch.equal(xn.to(F64), b["x"][:M])                              # the typed RMSNorm gives +-{0.5, 1, 2} exactly
    if M > 1:
        assert bool((b["h"][:M, b["cols"]].amax(0) != b["h"][:M, b["cols"]].amin(0)).all())      # payload where the rows differ
    assert_lattice(y.view(M, Hq + 2 * Hkv, D), D)
    if not w4:
        return h, nw, b["W"], b["bias"].to(BF), y
    if "q4" not in b:
        wq, s, bi = Q.quantize_affine(b["W4"])
        assert bool((s.to(F64) == 0.125).all()) and bool((bi.to(F64) == -1).all())
        assert torch.equal(Q.dequantize(wq, s, bi), b["W4"])                # lossless
        b["q4"] = (wq, s, bi)
    return h, nw, b["q4"], b["bias"].to(BF), y


# ------------------------------------------------------------------ the exact rotation
def selector(sections, half):
    """frequency index -> position axis, as the kernels decide it: f < s0 -> t, f < s0 + s1 -> h, else w"""
    f = torch.arange(half)
    return (f >= sections[0]).long() + (f >= sections[0] + sections[1]).long()


def angles_f32(pos, inv_freq_f32):
    """fp32(fp32(pos) * inv_freq[f]): one fp32 rounding - the kernels' contract.  pos int [..., half or 1]"""
    assert int(pos.max()) < 2 ** 24 and inv_freq_f32.dtype == F32
    return pos.to(F32) * inv_freq_f32


def rotate_exact(y_pair, pos, inv_freq_f32, qk_scale=1.0):
    """y_pair = (y_d, y_p) float64 [..., half] (element d of a head and its partner d + D/2), pos int broadcastable to it
    -> ((ex_d, ex_p) float64, unrounded; mag = |z_d| + |z_p|)"""
    ang = angles_f32(pos, inv_freq_f32).to(F64)
    c, s = torch.cos(ang), torch.sin(ang)
    zd, zp = y_pair
    if qk_scale != 1.0:
        zd, zp = rne_bf16(zd * qk_scale), rne_bf16(zp * qk_scale)
    return (zd * c - zp * s, zp * c + zd * s), zd.abs() + zp.abs()


def rotate_heads(y, posf, inv_freq_f32, qk_scale=1.0):
    """y [rows, H, D] float64, posf int [rows, half] (or [rows, 1]) -> (ex, mag) [rows, H, D]"""
    half = y.shape[-1] // 2
    (ed, ep), mag = rotate_exact((y[..., :half], y[..., half:]), posf[:, None, :], inv_freq_f32, qk_scale)
    return torch.cat([ed, ep], -1), torch.cat([mag, mag], -1)


def rotate_table(y, cos_f32, sin_f32):
    """the vision form: the kernel is GIVEN fp32 cos / sin tables [rows, half]; ex from those values"""
    half = y.shape[-1] // 2
    c, s = cos_f32.to(F64)[:, None, :], sin_f32.to(F64)[:, None, :]
    zd, zp = y[..., :half], y[..., half:]
    mag = zd.abs() + zp.abs()
    return torch.cat([zd * c - zp * s, zp * c + zd * s], -1), torch.cat([mag, mag], -1)


# ------------------------------------------------------------------ the checker
def _round_interval(v):
    """bf16 values v (float64) -> the interval of reals that round to v"""
    a = v.abs()
    m, e = torch.frexp(a)
    ulp = torch.ldexp(torch.ones_like(a), e - 8)                            # spacing above |v|
    below = torch.where(m == 0.5, ulp / 2, ulp)                             # spacing below a power of two is half of it
    lo_a, hi_a = a - below / 2, a + ulp / 2
    zero = a == 0
    lo_a, hi_a = torch.where(zero, a, lo_a), torch.where(zero, a, hi_a)
    neg = v < 0
    return torch.where(neg, -hi_a, lo_a), torch.where(neg, -lo_a, hi_a)


def rot_report(out_bf16, ex, mag, c=C_FP32):
    """-> (n_bad, c_needed, share): elements outside the bar at c, the smallest c that would pass, the share of elements
    that differ from rne_bf16(ex)"""
    out = out_bf16.detach().to("cpu", F64).reshape(-1)
    ex, mag = ex.reshape(-1), mag.reshape(-1)
    assert out.shape == ex.shape == mag.shape, (out.shape, ex.shape, mag.shape)
    finite = torch.isfinite(out)
    delta = c * 2.0 ** -24 * mag
    ok = finite & (rne_bf16(ex - delta) <= out) & (out <= rne_bf16(ex + delta))
    lo, hi = _round_interval(torch.where(finite, out, torch.zeros_like(out)))
    dist = torch.maximum(torch.maximum(lo - ex, ex - hi), torch.zeros_like(ex))
    need = torch.where(mag > 0, dist / (2.0 ** -24 * mag.clamp_min(1e-300)),
                       torch.where(dist > 0, torch.full_like(dist, float("inf")), torch.zeros_like(dist)))
    need = torch.where(finite, need, torch.full_like(need, float("inf")))
    share = float((out != rne_bf16(ex)).to(F64).mean())
    return int((~ok).sum()), float(need.max()), share


def check_rot(name, out_bf16, ex, mag, c=C_FP32, cap=True):
    """assert the bar and the cap; prints the smallest c that would pass and the mismatch share (pytest -s shows them).
    cap=False: the caller applies the cap to the whole case (several tensors of one launch) -> (c needed, share, elements)"""
    bad, need, share = rot_report(out_bf16, ex, mag, c)
    print(f"ROPE-EXACT {name:60s} c needed {need:6.3f} (bar {c:g}, {bad} over)  != rne(ex): {share:.2e} (cap {CAP:g})")
    assert bad == 0 and (share <= CAP or not cap), (name, bad, need, share)
    return need, share, ex.numel()


def passes(out_bf16, ex, mag, c=C_FP32):
    bad, _, share = rot_report(out_bf16, ex, mag, c)
    return bad == 0 and share <= CAP


# ------------------------------------------------------------------ fp32 evaluation: the honest one and the mutants
ROT_MUTANTS = ("inv_shift", "pos_bf16", "cs_bf16", "range_reduce", "sin_flip_hi", "partner_m1", "sel_shift", "scale_unrounded")
POOL_MUTANTS = ("k_slot_p1", "v_natural")


def rotate_fp32(y, pos3, inv_freq_f32, sections, qk_scale=1.0, defect=None):
    """what a kernel computes, in fp32 on the CPU: y [rows, H, D] float64 lattice values, pos3 int [3, rows] -> bf16.
    defect: one of ROT_MUTANTS - a subtly wrong kernel."""
    rows, H, D = y.shape
    half = D // 2
    sel = selector(sections, half)
    inv = inv_freq_f32
    if defect == "sel_shift":
        sel = torch.roll(sel, 1)
        sel[0] = 0
    if defect == "inv_shift":                                    # the top eight frequencies read their neighbour's entry
        idx = torch.arange(half)
        idx[half - 8:] -= 1
        inv = inv[idx]
    p = pos3[sel].T.to(F32)                                      # [rows, half]
    if defect == "pos_bf16":
        p = p.to(BF).to(F32)
    ang = p * inv
    if defect == "range_reduce":                                 # one fp32 constant for 2 pi
        two_pi = torch.tensor(2 * math.pi, dtype=F32)
        ang = ang - torch.round(ang * torch.tensor(1 / (2 * math.pi), dtype=F32)) * two_pi
    c, s = torch.cos(ang)[:, None, :], torch.sin(ang)[:, None, :]
    if defect == "cs_bf16":
        c, s = c.to(BF).to(F32), s.to(BF).to(F32)
    z = y.to(F32)
    if qk_scale != 1.0:
        z = z * torch.tensor(qk_scale, dtype=F32)
        if defect != "scale_unrounded":
            z = z.to(BF).to(F32)
    zd, zp = z[..., :half], z[..., half:]
    if defect == "partner_m1":
        zp = torch.roll(zp, 1, -1)
    hi = zp * c - zd * s if defect == "sin_flip_hi" else zp * c + zd * s
    return torch.cat([zd * c - zp * s, hi], -1).to(BF)


def cpu_case(geo, seed=0):
    """one case of the CPU table: the 16 lattice rows of a geometry's q and k heads, three distinct position axes"""
    Hq, Hkv, D, K, theta = geo
    y = lattice_qkv(16, Hq, Hkv, D, K, False, seed)[4].view(16, Hq + 2 * Hkv, D)[:, :Hq + Hkv]
    pt = torch.tensor([POSITIONS[(7 + 3 * m) % 10] for m in range(16)])
    ph = torch.tensor([POSITIONS[(2 + 7 * m) % 10] for m in range(16)])
    pw = torch.tensor([POSITIONS[(5 + 9 * m) % 10] for m in range(16)])
    ph[pt == 0] = 0                                              # a row at position 0 on every axis: the identity
    pw[pt == 0] = 0
    return y, torch.stack([pt, ph, pw]), O.mrope_inv_freq(D, theta)


def exact_mrope(y, pos3, inv_freq_f32, sections, qk_scale=1.0):
    posf = pos3[selector(sections, y.shape[-1] // 2)].T          # [rows, half]
    return rotate_heads(y, posf, inv_freq_f32, qk_scale)


# ------------------------------------------------------------------ the paged pools
def pools_new(n_pages, Hkv, D, device="cpu"):
    """K pool [page][Hkv][D/8][64][8], V pool [page][Hkv][D][64 slots], every 16-bit word the sentinel"""
    k = torch.full((n_pages, Hkv, D // 8, PAGE, 8), SENTINEL, dtype=torch.int16, device=device).view(BF)
    v = torch.full((n_pages, Hkv, D, PAGE), SENTINEL, dtype=torch.int16, device=device).view(BF)
    return k, v


def pools_write(kpool, vpool, k_rows, v_rows, pages, within, defect=None):
    """the CPU model of the pool write: k_rows / v_rows [T, Hkv, D] bf16 at (pages[t], within[t]).  defect: POOL_MUTANTS"""
    T, Hkv, D = k_rows.shape
    for t in range(T):
        w = int(within[t])
        kw = min(w + 1, PAGE - 1) if defect == "k_slot_p1" else w
        kpool[int(pages[t]), :, :, kw, :] = k_rows[t].view(Hkv, D // 8, 8)
        vpool[int(pages[t]), :, :, w if defect == "v_natural" else VSLOT[w]] = v_rows[t]


def pools_read(kpool, vpool, pages, within):
    """-> (k rows [T, Hkv, D], v rows [T, Hkv, D] as stored at (pages[t], within[t]); the number of 16-bit words of both pools
    that are NOT at one of those places and do not hold the sentinel)"""
    dev = kpool.device
    pages = torch.as_tensor(pages, dtype=torch.long, device=dev)
    within = torch.as_tensor(within, dtype=torch.long, device=dev)
    vs = torch.tensor(VSLOT, dtype=torch.long, device=dev)[within]
    assert len(set(zip(pages.tolist(), within.tolist()))) == pages.numel()
    T, Hkv, D = pages.numel(), kpool.shape[1], vpool.shape[2]
    k_rows = kpool[pages, :, :, within, :].reshape(T, Hkv, D)
    v_rows = vpool[pages, :, :, vs]
    ki, vi = kpool.view(torch.int16).clone(), vpool.view(torch.int16).clone()
    ki[pages, :, :, within, :] = SENTINEL
    vi[pages, :, :, vs] = SENTINEL
    stray = int((ki != SENTINEL).sum()) + int((vi != SENTINEL).sum())
    return k_rows.cpu(), v_rows.cpu(), stray


def check_pools(name, k_rows, v_rows, stray, ex_k, mag_k, y_v):
    """the K pool at (page, head, slot) passes check_rot, the V pool in VSLOT order equals y bit for bit, every other
    16-bit word of both pools still holds the sentinel"""
    assert stray == 0, (name, "words written outside the rows' slots", stray)
    assert torch.equal(v_rows.to(F64), y_v), (name, "V pool")
    return check_rot(name + " K pool", k_rows, ex_k, mag_k, cap=False)


# ------------------------------------------------------------------ the fused decode forms: case table, inputs, runner
ENTRIES = {
    # entry point of mlx_vlm_amd.ops -> (4-bit weights, workspace, the row counts of the table)
    "gemv_qkv_rope_kvwrite": (False, False, (1, 2, 3, 4, 5, 8, 9)),
    "gemv_qkv_rope_kvwrite_ws": (False, True, (9, 13, 16)),
    "gemv_w4_qkv_rope_kvwrite": (True, False, (1, 2, 4)),
    "gemv_w4_qkv_rope_kvwrite_ws": (True, True, (9, 16)),
}


def form_of(w4, ws, M, K, mfma2=True):
    """which kernel a call reaches, or None where the entry point refuses it - read off vlm_gemv_qkv_rope_kvwrite_ex,
    vlm_gemv_w4_qkv_rope_kvwrite_ex and the two mfma `_try` functions (csrc/gemv_bf16.hip, gemv_w4.hip, gemv_mfma.hip,
    gemv_mfma2.hip):
      - the matrix-core forms take the rope epilogue from 9 rows; the second one needs the workspace (its norm prologue's
        scratch) and, over bf16 weights, K >= 4096; the first one splits K above 28 chunks of 128, which needs the workspace
      - below that the v_dot2c kernels: 1 / 2 / 4 / 8 rows, K <= 4096, the activations within 64 KiB"""
    if M >= 9:
        if ws and mfma2 and K % (256 if w4 else 128) == 0 and (w4 or K >= 4096):
            return "mfma2"
        if K % 128 == 0 and (ws or K <= 28 * 128):
            return "mfma"
    if M in (1, 2, 4, 8) and K <= 4096 and M * K * 2 <= 64 * 1024:
        return "dot2c"
    return None


def fused_cases():
    out = []
    for gi, geo in enumerate(GEOMETRIES):
        for entry, (w4, ws, rows) in ENTRIES.items():
            for M in rows:
                out.append(dict(entry=entry, gi=gi, M=M, form=form_of(w4, ws, M, geo[3])))
    return out


FUSED_CASES = [c for c in fused_cases() if c["form"] is not None]
REFUSED_CASES = [c for c in fused_cases() if c["form"] is None]


def fused_id(c):
    return f"{c['entry']}-{geo_id(GEOMETRIES[c['gi']])}-M{c['M']}"


def fused_inputs(case, paged):
    """host tensors of one fused call + what it must leave behind"""
    Hq, Hkv, D, K, theta = GEOMETRIES[case["gi"]]
    M, w4 = case["M"], ENTRIES[case["entry"]][0]
    h, nw, W, bias, y = lattice_qkv(M, Hq, Hkv, D, K, w4, seed=100 + case["gi"])
    pos = torch.tensor([POSITIONS[(7 + 3 * m) % 10] for m in range(M)], dtype=torch.int32)
    slot = torch.tensor([SLOTS[(m + M) % 16] for m in range(M)], dtype=torch.int32)
    n_pages = M * MAX_PAGES + (3 if paged else 0)
    if paged:
        perm = torch.randperm(n_pages, generator=torch.Generator().manual_seed(7 * M + case["gi"]))
        bt = perm[:M * MAX_PAGES].to(torch.int32).reshape(M, MAX_PAGES)
    else:
        bt = torch.arange(n_pages, dtype=torch.int32).reshape(M, MAX_PAGES)
    inv = O.mrope_inv_freq(D, theta)
    y3 = y.view(M, Hq + 2 * Hkv, D)
    ex, mag = rotate_heads(y3[:, :Hq + Hkv], pos.long()[:, None], inv)
    pages = bt[torch.arange(M), (slot // PAGE).long()].long()
    return dict(h=h, nw=nw, W=W, bias=bias, pos=pos, slot=slot, bt=bt, paged=paged, n_pages=n_pages, inv=inv, y3=y3, ex=ex, mag=mag,
                pages=pages, within=(slot % PAGE).long(), dims=(Hq, Hkv, D, K, M), w4=w4)


def run_fused(vops, case, paged, device="cuda", refused=False):
    """one call of the entry point on fresh sentinel pools -> (q columns [M, Hq, D], k rows, v rows, stray), all on the host.
    refused: the call must raise; -> the number of pool words it wrote all the same"""
    i = fused_inputs(case, paged)
    Hq, Hkv, D, K, M = i["dims"]
    kpool, vpool = pools_new(i["n_pages"], Hkv, D, device)
    d = lambda t: t.to(device)
    bt = d(i["bt"]) if paged else None
    fn = getattr(vops, case["entry"])
    if refused:
        try:
            fn(d(i["h"]), d(i["nw"]), d(i["W"]), d(i["bias"]), Hq, Hkv, D, d(i["pos"]), d(i["slot"]), d(i["inv"]), bt, kpool, vpool,
               eps=EPS, max_pages=MAX_PAGES)
        except RuntimeError:
            return int((kpool.view(torch.int16) != SENTINEL).sum()) + int((vpool.view(torch.int16) != SENTINEL).sum())
        raise AssertionError(f"{fused_id(case)}: the entry point took a shape no kernel is built for")
    if i["w4"]:
        from mlx_vlm_amd.models import quantized as Qz

        wq, s, b = i["W"]
        dq = Qz.take({"p.weight": wq, "p.scales": s, "p.biases": b}, "p").to(device)
        out = fn(d(i["h"]), d(i["nw"]), dq.wq, dq.sb, d(i["bias"]), Hq, Hkv, D, d(i["pos"]), d(i["slot"]), d(i["inv"]), bt, kpool, vpool,
                 eps=EPS, max_pages=MAX_PAGES)
    else:
        out = fn(d(i["h"]), d(i["nw"]), d(i["W"]), d(i["bias"]), Hq, Hkv, D, d(i["pos"]), d(i["slot"]), d(i["inv"]), bt, kpool, vpool,
                 eps=EPS, max_pages=MAX_PAGES)
    k_rows, v_rows, stray = pools_read(kpool, vpool, i["pages"], i["within"])
    return out.view(M, Hq + 2 * Hkv, D)[:, :Hq].cpu(), k_rows, v_rows, stray


def check_fused(name, case, paged, q, k_rows, v_rows, stray):
    i = fused_inputs(case, paged)
    Hq, Hkv, D, K, M = i["dims"]
    _, sq, nq = check_rot(name + " q", q, i["ex"][:, :Hq], i["mag"][:, :Hq], cap=False)
    _, sk, nk = check_pools(name, k_rows, v_rows, stray, i["ex"][:, Hq:], i["mag"][:, Hq:], i["y3"][:, Hq + Hkv:])
    assert (sq * nq + sk * nk) / (nq + nk) <= CAP, (name, "cap over the case: q and the K pool", sq, sk)
    at0 = i["pos"] == 0                                          # position 0: the identity, bit for bit
    assert torch.equal(q[at0].to(F64), i["y3"][at0][:, :Hq]) and torch.equal(k_rows[at0].to(F64), i["y3"][at0][:, Hq:Hq + Hkv]), name
