"""Exactly rounded attention references, the paged-pool builders and the bar classes every attention test shares.

A reference here is the operation in float64, rounded ONCE to bf16 at the end - or, where the product follows the reference
model's typed graph on purpose, at exactly those rounding points and no others.  The kernels' distance from it is what the
bar classes bound:

    "hilo"    P as two bf16 MFMA operands (hi = bf16(p), lo = bf16(p - hi)): every bf16 decode form and prefill at D = 128.
              Measured 1e-6 .. 1e-5 (decode) and 7e-5 (prefill) rel-rms; only an fp32 summation order separates them from
              the exact result, so almost every output element IS the exactly rounded value.
    "single"  P as ONE bf16 operand: prefill at D = 64 / 80 (the vision default: hi + lo costs +25 % of that launch) and
              the 8-bit decode kernel, which follows quantized_scaled_dot_product_attention's typed graph (its
              probabilities are a bf16 tensor).  Relative noise of 2^-9 per probability, averaged over the keys: ~2e-3.

The 8-bit reference keeps the typed rounding points the product reproduces on purpose - bf16(scale) (the weak python scalar
takes the array's dtype), q * scale rounded to bf16, the scores rounded to bf16 - and takes the keys / values as the exact
dequantised values scale * n + bias of oracle/quant.py's mx.quantize; the probabilities and P . V stay exact.

rel-rms is normalised per segment (a decode row, a prefill segment's query rows): sqrt(sum_s |a_s - b_s|^2 / rms(b_s)^2 / N).
With one segment it is the plain whole-tensor rel-rms; with mixed lengths a long context (output rms ~ n^-1/2) counts as
much per element as a one-token row (rms ~ 1).  The elementwise check is bf16_close per segment (atol scaled by the
segment's rms).

Imports without a GPU: the CPU test tests/test_attn_bars_cpu.py builds float64 mutants from the same functions and shape
tables and asserts that every class rejects what it is meant to catch."""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

BF, F64 = torch.bfloat16, torch.float64
PAGE = 64
LOG2E = 1.4426950408889634
# V pool key-slot order inside a page (csrc/common.hpp vlm_vslot)
VSLOT = [(w & 32) + 8 * (((w & 31) & 15) >> 2) + 4 * ((w & 31) >> 4) + (w & 3) for w in range(64)]


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def rne_bf16(x: torch.Tensor) -> torch.Tensor:
    """float64 -> the nearest bf16 value (ties to even) as float64, in ONE rounding (a cast through fp32 would round twice)"""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.round(torch.ldexp(m, torch.full_like(e, 8))), e - 8)


def bf16_of(s: float) -> float:
    return float(rne_bf16(torch.tensor([s], dtype=F64))[0])


# ------------------------------------------------------------------ bar classes and the checker
@dataclass(frozen=True)
class Bar:
    rel_rms: float
    ulps: float
    atol_rms: float


BARS = {
    "hilo": Bar(rel_rms=5e-4, ulps=1, atol_rms=2e-3),
    "single": Bar(rel_rms=3e-3, ulps=2, atol_rms=2e-2),
    "q8": Bar(rel_rms=3e-3, ulps=2, atol_rms=2e-2),
}
# Worst measured on an MI355X over every attention test that checks a class (the whole GPU suite): hilo rel-rms 2.6e-4,
# elementwise needs atol_rms 9.4e-4 at 1 ulp; single 2.63e-3 / 1.5e-2 at 2 ulps; q8 2.61e-3 / 5.7e-3 at 2 ulps.
# which defects (DEFECTS below) each class must reject; the rest are legitimate in that class
CATCHES = {
    "hilo": ("scale_bf16", "logits_bf16", "log2e_bf16", "p_bf16", "p_fp16", "den_bf16", "scale_2m8", "drop_end", "drop_page"),
    # (bf16 logits sit at 2.7e-3 .. 4.5e-3 here, one bf16 P at 1.8e-3 .. 2.5e-3 and the kernels at up to 2.55e-3: no rel-rms
    # bar separates them on the causal short-segment packs, so this class does not claim to)
    "single": ("scale_2m8", "drop_end", "drop_page"),
    "q8": ("scale_2m8", "drop_end", "drop_page"),          # (its scores ARE bf16: the typed graph's rounding point)
}
DEFECTS = ("scale_bf16", "logits_bf16", "log2e_bf16", "p_bf16", "p_fp16", "den_bf16", "scale_2m8", "drop_end", "drop_page")


def prefill_class(D: int) -> str:
    return "hilo" if D == 128 else "single"


def _segments(n, segments):
    return [(0, n)] if segments is None else list(segments)


def measure(out, exact, cls, segments=None):
    """-> (ok, rel_rms, atol_needed, report).  out / exact [rows, ...]; segments: (row0, row1) ranges of rows, each normalised
    by its own rms.  atol_needed: the smallest atol_rms (per segment rms) for which bf16_close at the class's ulps passes."""
    bar = BARS[cls]
    a = out.detach().to("cpu", F64).reshape(out.shape[0], -1)
    b = exact.detach().to("cpu", F64).reshape(exact.shape[0], -1)
    assert a.shape == b.shape, (a.shape, b.shape)
    num, cnt, need, nbad = 0.0, 0, 0.0, 0
    finite = bool(torch.isfinite(a).all())
    for r0, r1 in _segments(a.shape[0], segments):
        sa, sb = a[r0:r1], b[r0:r1]
        rms = float(sb.pow(2).mean().sqrt()) + 1e-30
        err = (sa - sb).abs()
        num += float(err.pow(2).sum()) / rms ** 2
        cnt += sb.numel()
        over = (err - bar.ulps * 2.0 ** -7 * sb.abs()).clamp_min(0) / rms
        need = max(need, float(over.max()))
        nbad += int((over > bar.atol_rms).sum())
    rel = math.sqrt(num / max(cnt, 1)) if finite else float("inf")
    ok = finite and rel <= bar.rel_rms and nbad == 0
    rep = (f"[{cls}] rel-rms {rel:.3e} (bar {bar.rel_rms:.0e})  elementwise at {bar.ulps:g} ulp needs atol_rms {need:.3e} "
           f"(bar {bar.atol_rms:.0e}, {nbad} over)")
    return ok, rel, need, rep


def check(name, out, exact, cls, segments=None):
    """assert both bars of the class; prints both numbers (pytest -s shows them: the bars are set from them)"""
    ok, rel, need, rep = measure(out, exact, cls, segments)
    print(f"ATTN-EXACT {name:64s} {rep}")
    assert ok, (name, rep)
    return rel, need


# ------------------------------------------------------------------ float64 attention core (+ the defects of a wrong kernel)
def _attend(q, k, v, scale, visible=None, defect=None, round_logits=False):
    """q [H, Lq, D], k / v [H, Lk, D] float64; visible [Lq, Lk] bool (None = all) -> o [H, Lq, D] float64 (not rounded).
    round_logits: the scores are a bf16 tensor (the 8-bit path's typed graph)."""
    Lq, Lk = q.shape[1], k.shape[1]
    if visible is None:
        visible = torch.ones(Lq, Lk, dtype=torch.bool, device=q.device)
    if defect in ("drop_end", "drop_page"):
        # each query row loses the last key it sees (drop_end) or the first key of the 64-key page / tile holding it
        last = (torch.arange(Lk, device=q.device)[None, :] * visible).amax(-1)
        drop = last if defect == "drop_end" else (last // PAGE) * PAGE
        visible = visible.clone()
        visible[torch.arange(Lq, device=q.device), drop] = False
    if defect == "scale_bf16":
        scale = bf16_of(scale)
    elif defect == "scale_2m8":
        scale = scale * (1 + 2.0 ** -8)
    s = (q @ k.transpose(-1, -2)) * scale
    if round_logits or defect == "logits_bf16":
        s = rne_bf16(s)
    s = s.masked_fill(~visible, float("-inf"))
    m = s.amax(-1, keepdim=True).clamp_min(-1e300)                       # (a row with nothing visible: o = 0)
    x = s - m
    if defect == "log2e_bf16":                                           # exp2(x * log2e) with log2e rounded to bf16
        x = x * (bf16_of(LOG2E) / LOG2E)
    p = torch.exp(x)
    den = p.sum(-1, keepdim=True)
    if defect == "p_bf16":
        p = rne_bf16(p)
    elif defect == "p_fp16":
        p = p.to(torch.float16).to(F64)
    if defect == "den_bf16":
        den = rne_bf16(den)
    return (p @ v) / den.clamp_min(1e-300)


def _pad(o, D):
    if o.shape[-1] == D:
        return o
    return torch.cat([o, o.new_zeros(*o.shape[:-1], D - o.shape[-1])], -1)


# ------------------------------------------------------------------ prefill
def prefill_exact(q, k, v, lens, scale, causal, starts=None, real=None, dev="cpu", defect=None):
    """varlen prefill: q [T, Hq, D], k / v [T, Hkv, D] (bf16); segment s = rows of lens[s]; causal on absolute rows of the
    segment; starts[s]: rows before it are keys only (their output rows are 0 here and not compared).  real: head width
    the scale belongs to - the reference runs at q[..., :real] and pads its output with exact zeros.
    -> bf16 [T, Hq, D]"""
    T, Hq, D = q.shape
    Hkv = k.shape[1]
    G = Hq // Hkv
    w = real or D
    out = torch.zeros(T, Hq, D, dtype=F64)
    off = 0
    for si, n in enumerate(lens):
        s0 = starts[si] if starts is not None else 0
        qs = q[off + s0:off + n, :, :w].to(dev, F64).permute(1, 0, 2)
        ks = k[off:off + n, :, :w].to(dev, F64).permute(1, 0, 2).repeat_interleave(G, 0)
        vs = v[off:off + n, :, :w].to(dev, F64).permute(1, 0, 2).repeat_interleave(G, 0)
        vis = None
        if causal:
            vis = torch.arange(n, device=dev)[None, :] <= torch.arange(s0, n, device=dev)[:, None]
        for h0 in range(0, Hq, 4):                                       # heads in chunks: [4, n, n] float64 at most
            o = _attend(qs[h0:h0 + 4], ks[h0:h0 + 4], vs[h0:h0 + 4], scale, vis, defect)
            out[off + s0:off + n, h0:h0 + 4] = _pad(o, D).permute(1, 0, 2).cpu()
        off += n
    return rne_bf16(out).to(BF)


def query_rows(lens, starts=None):
    """-> (bool [T] rows that are queries, segments as (row0, row1) of the compacted query rows)"""
    rows, segs, c = [], [], 0
    for si, n in enumerate(lens):
        s0 = starts[si] if starts is not None else 0
        rows += [False] * s0 + [True] * (n - s0)
        segs.append((c, c + n - s0))
        c += n - s0
    return torch.tensor(rows), segs


# ------------------------------------------------------------------ paged KV pools
def pages_of(n):
    return (n + PAGE - 1) // PAGE


def build_pools(ks, vs, seed, identity=False, fill=float("nan")):
    """ks / vs: per sequence [n, Hkv, D] bf16 -> (block table int32 [B, max_pages], kpool [P, Hkv, D/8, 64, 8],
    vpool [P, Hkv, D, 64 slots], max_pages).  Unwritten slots hold `fill` (NaN: a kernel that reads one poisons its row).
    identity: row b owns pages [b * max_pages, (b + 1) * max_pages) (the block table is then that identity); otherwise the
    pages are a seeded shuffle of a pool with 3 spare pages."""
    B, Hkv, D = len(ks), ks[0].shape[1], ks[0].shape[2]
    max_pages = max(pages_of(k.shape[0]) for k in ks) + 1
    n_pages = B * max_pages if identity else sum(pages_of(k.shape[0]) for k in ks) + 3
    perm = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed)).tolist()
    bt = torch.zeros(B, max_pages, dtype=torch.int32)
    kpool = torch.full((n_pages, Hkv, D // 8, PAGE, 8), fill, dtype=BF)
    vpool = torch.full((n_pages, Hkv, D, PAGE), fill, dtype=BF)
    for b, (k, v) in enumerate(zip(ks, vs)):
        n = k.shape[0]
        for p in range(max_pages):
            bt[b, p] = b * max_pages + p if identity else (perm.pop() if p < pages_of(n) else 0)
        for p in range(pages_of(n)):
            page, m = int(bt[b, p]), min(PAGE, n - p * PAGE)
            kpool[page, :, :, :m, :] = k[p * PAGE:p * PAGE + m].permute(1, 0, 2).reshape(Hkv, m, D // 8, 8).permute(0, 2, 1, 3)
            vpool[page][:, :, VSLOT[:m]] = v[p * PAGE:p * PAGE + m].permute(1, 2, 0)
    return bt, kpool, vpool, max_pages


# ------------------------------------------------------------------ decode
def decode_exact(q, ks, vs, scale, real=None, dev="cpu", defect=None):
    """one query row per sequence: q [B, Hq * D], ks / vs per sequence [n, Hkv, D] -> bf16 [B, Hq * D]"""
    B = q.shape[0]
    Hkv, D = ks[0].shape[1], ks[0].shape[2]
    Hq = q.shape[1] // D
    w = real or D
    rows = []
    for b in range(B):
        qq = q[b].view(Hq, 1, D)[..., :w].to(dev, F64)
        kk = ks[b][..., :w].to(dev, F64).permute(1, 0, 2).repeat_interleave(Hq // Hkv, 0)
        vv = vs[b][..., :w].to(dev, F64).permute(1, 0, 2).repeat_interleave(Hq // Hkv, 0)
        rows.append(_pad(_attend(qq, kk, vv, scale, None, defect), D).reshape(Hq * D).cpu())
    return rne_bf16(torch.stack(rows)).to(BF)


def dequant8(x):
    """x [n, Hkv, D] bf16 -> the exact values scale * n + bias of oracle/quant.py's mx.quantize(bits = 8, group_size = 64)
    (what vlm_kv_quantize_tokens stores, bit for bit), float64"""
    from oracle import quant as Q

    wq, sc, bi = Q.quantize_nd(x, 64, 8)
    n = Q.unpack(wq.reshape(-1, wq.shape[-1]), 8).reshape(*x.shape).to(F64)
    g = n.reshape(*x.shape[:-1], -1, 64)
    return (g * sc.to(F64)[..., None] + bi.to(F64)[..., None]).reshape(x.shape)


def decode_q8_exact(q, ks, vs, scale, dev="cpu", defect=None):
    """8-bit decode (quantized_scaled_dot_product_attention at L == 1) over the exactly dequantised keys / values, with the
    typed graph's rounding points: bf16(scale), q * scale -> bf16, scores -> bf16 -> bf16 [B, Hq * D]"""
    B = q.shape[0]
    Hkv, D = ks[0].shape[1], ks[0].shape[2]
    Hq = q.shape[1] // D
    s = bf16_of(scale)
    if defect == "scale_2m8":
        s = s * (1 + 2.0 ** -8)
    inner = None if defect in ("scale_2m8", "logits_bf16", "scale_bf16") else defect
    rows = []
    for b in range(B):
        qs = rne_bf16(q[b].view(Hq, 1, D).to(dev, F64) * s)
        kk = dequant8(ks[b]).to(dev).permute(1, 0, 2).repeat_interleave(Hq // Hkv, 0)
        vv = dequant8(vs[b]).to(dev).permute(1, 0, 2).repeat_interleave(Hq // Hkv, 0)
        rows.append(_attend(qs, kk, vv, 1.0, None, inner, round_logits=True).reshape(Hq * D).cpu())
    return rne_bf16(torch.stack(rows)).to(BF)


def oproj_exact(att, wo, h=None, dev="cpu"):
    """o_proj fused behind the attention: att (the exactly rounded attention, bf16 [M, K]) @ wo.T in float64, rounded once;
    + h as the reference's second typed op (rounded again)"""
    y = rne_bf16(att.to(dev, F64) @ wo.to(dev, F64).T).cpu()
    if h is not None:
        y = rne_bf16(y + h.to(F64))
    return y.to(BF)


def decode_inputs(lens, Hq, Hkv, D=128, seed=0, real=None, kscale=1.0, outlier=False):
    """seeded q [B, Hq * D] and per-sequence k / v [n, Hkv, D]; real < D: columns real.. are exact zeros"""
    q = rnd(len(lens), Hq, D, seed=seed)
    ks = [rnd(n, Hkv, D, seed=seed + 100 + b, scale=kscale) for b, n in enumerate(lens)]
    vs = [rnd(n, Hkv, D, seed=seed + 200 + b, scale=kscale) for b, n in enumerate(lens)]
    if outlier:
        for k in ks:
            k[:, :, 5] += 3.0                                           # an outlier channel: lopsided 8-bit groups
    if real is not None and real < D:
        q[..., real:] = 0
        for t in ks + vs:
            t[..., real:] = 0
    return q.reshape(len(lens), Hq * D), ks, vs


def prefill_inputs(lens, Hq, Hkv, D, seed=0, real=None):
    T = sum(lens)
    q, k, v = rnd(T, Hq, D, seed=seed), rnd(T, Hkv, D, seed=seed + 1), rnd(T, Hkv, D, seed=seed + 2)
    if real is not None and real < D:
        for t in (q, k, v):
            t[..., real:] = 0
    return q, k, v


# ------------------------------------------------------------------ shape tables (the GPU sweeps and the CPU bar test share them)
DECODE_LENS = [1, 63, 64, 65, 2047, 4100]
# every G = Hq / Hkv instance of the bf16 decode kernels; Hq <= 16 so the o_proj prologue form (K = Hq * 128 <= 2048) runs too
DECODE_CASES = [dict(G=G, Hq=2 * G, Hkv=2, lens=DECODE_LENS) for G in range(1, 9)]
# the 8-bit kernel: B * Hkv < 128 -> the 64-key form; B * Hkv >= 128 (with nsplit <= 16) -> the half-page form
Q8_CASES = [dict(G=G, Hq=2 * G, Hkv=2, lens=DECODE_LENS, nsplit=8, form="64-key") for G in range(1, 9)] + [
    dict(G=4, Hq=32, Hkv=8, lens=[1, 63, 64, 65, 2047, 130, 700, 33, 4100, 64, 65, 1, 200, 999, 128, 257], nsplit=8,
         form="half-page"),                                             # 16 rows x 8 kv heads = 128 pairs
    dict(G=7, Hq=28, Hkv=4, lens=[1, 63, 64, 65, 2047, 130, 700, 33] * 4, nsplit=16, form="half-page"),   # 32 x 4
    dict(G=1, Hq=8, Hkv=8, lens=[65, 2047, 1, 300] * 3 + [64, 63], nsplit=4, form="64-key"),              # 14 x 8 = 112 pairs
]

PREFILL_SHORT = [1, 63, 64, 65, 127, 128, 129]
PREFILL_CASES = []
for _D in (64, 80, 128):
    for _causal in (False, True):
        for _G in (1, 4, 6, 7, 8):
            _lens = list(PREFILL_SHORT)
            # one prompt near 2k tokens per (D, causal): it straddles the 128-row block and 64-key tile 16 times over
            if _G == {(64, False): 1, (64, True): 4, (80, False): 1, (80, True): 6, (128, False): 8, (128, True): 7}[(_D, _causal)]:
                _lens = [2049, 65, 1]
            PREFILL_CASES.append(dict(D=_D, causal=_causal, G=_G, Hq=_G, Hkv=1, lens=_lens))
QSTART_CASES = [
    dict(D=128, causal=True, G=4, Hq=8, Hkv=2, lens=[300, 129, 65], starts=[257, 1, 64]),
    dict(D=128, causal=True, G=8, Hq=8, Hkv=1, lens=[700, 64], starts=[699, 0]),
    dict(D=128, causal=True, G=1, Hq=4, Hkv=4, lens=[130, 190], starts=[1, 127]),
    dict(D=64, causal=True, G=7, Hq=7, Hkv=1, lens=[300, 129], starts=[200, 128]),
    dict(D=80, causal=False, G=4, Hq=4, Hkv=1, lens=[200, 576], starts=[100, 575]),
]
# padded heads: the model runs a narrower head inside a wider kernel (zero pad columns, scale = real ** -0.5)
PAD_PREFILL_CASES = [
    dict(D=80, real=72, causal=False, G=1, Hq=4, Hkv=4, lens=[576, 129, 1]),       # SigLIP (Idefics2's tower) in the D = 80 kernel
    dict(D=128, real=96, causal=True, G=1, Hq=4, Hkv=4, lens=[300, 64, 129]),     # Phi-3.5 in the D = 128 engine
    dict(D=128, real=64, causal=True, G=1, Hq=4, Hkv=4, lens=[300, 64, 129]),     # nanoLLaVA's Qwen1.5-0.5B
]
PAD_DECODE_CASES = [dict(real=96, G=1, Hq=4, Hkv=4, lens=DECODE_LENS), dict(real=64, G=1, Hq=4, Hkv=4, lens=DECODE_LENS)]


def case_id(c):
    return "-".join(f"{k}{v if not isinstance(v, list) else len(v)}" for k, v in c.items() if k not in ("lens", "starts"))
