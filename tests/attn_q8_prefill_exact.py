"""The exactly rounded result of a prompt chunk attending over the uniform 8-bit KV cache (vlm_attn_prefill_paged_q8) - the
L > 1 sibling of attn_exact.decode_q8_exact - with the shape table and the pool builders its GPU test and its CPU bar test
share.  Float64 attention over the exactly dequantised keys / values (attn_exact.dequant8) with the typed graph's rounding
points and no others: bf16(scale), q * scale -> bf16, scores -> bf16; probabilities and P . V exact; one rounding to bf16.
The kernel is held to the existing "q8" class of attn_exact.BARS.  Imports without a GPU."""
from __future__ import annotations

import torch

from tests import attn_exact as A

BF, F64 = A.BF, A.F64
D = 128
# (tokens cached before the chunk, chunk rows, Hq, Hkv, outlier channel k[:, :, 5] += 3)
CASES = [(0, 5, 4, 2, False), (37, 70, 12, 2, False), (63, 1, 12, 2, False), (64, 64, 32, 8, True), (200, 129, 12, 2, True),
         (1000, 300, 28, 4, False), (4100, 257, 12, 2, False)]
# one launch, three segments of different sequences and lengths (block-table rows out of order)
MULTI = dict(Hq=12, Hkv=2, segs=[(10, 70), (130, 5), (0, 129)], seg_seq=[2, 0, 1])


def case_id(c):
    return f"prefix{c[0]}-chunk{c[1]}-Hq{c[2]}-Hkv{c[3]}" + ("-outlier" if c[4] else "")


def inputs(prefix, chunk, Hq, Hkv, seed, outlier=False):
    """-> q [chunk, Hq, D] (the chunk's rotated queries), k / v [prefix + chunk, Hkv, D] (the whole sequence), bf16"""
    q = A.rnd(chunk, Hq, D, seed=seed)
    k = A.rnd(prefix + chunk, Hkv, D, seed=seed + 1, scale=0.8)
    v = A.rnd(prefix + chunk, Hkv, D, seed=seed + 2, scale=0.8)
    if outlier:
        k[:, :, 5] += 3.0
    return q, k, v


def visible(prefix, chunk, dev="cpu"):
    """row r of the chunk sits at position prefix + r and sees slots 0 .. prefix + r"""
    return torch.arange(prefix + chunk, device=dev)[None, :] <= (prefix + torch.arange(chunk, device=dev))[:, None]


def prefill_q8_exact(q, k, v, prefix, scale, dev="cpu", defect=None):
    """q [L, Hq, D], k / v [prefix + L, Hkv, D] -> bf16 [L, Hq, D]"""
    L, Hq, _ = q.shape
    G = Hq // k.shape[1]
    s = A.bf16_of(scale)
    if defect == "scale_2m8":
        s = s * (1 + 2.0 ** -8)
    inner = None if defect in ("scale_2m8", "logits_bf16", "scale_bf16") else defect
    qs = A.rne_bf16(q.to(dev, F64).permute(1, 0, 2) * s)
    kk = A.dequant8(k).to(dev).permute(1, 0, 2).repeat_interleave(G, 0)
    vv = A.dequant8(v).to(dev).permute(1, 0, 2).repeat_interleave(G, 0)
    vis = visible(prefix, L, dev)
    out = torch.zeros(L, Hq, D, dtype=F64)
    for h0 in range(0, Hq, 4):                                           # heads in chunks: [4, L, S] float64 at most
        o = A._attend(qs[h0:h0 + 4], kk[h0:h0 + 4], vv[h0:h0 + 4], 1.0, vis, inner, round_logits=True)
        out[:, h0:h0 + 4] = o.permute(1, 0, 2).cpu()
    return A.rne_bf16(out).to(BF)


def oracle_typed(q, k, v, scale):
    """the oracle's typed graph (oracle/quant.py quantized_sdpa, causal) on the same inputs, bf16 [L, Hq, D]"""
    from oracle import quant as Q

    qk = Q.quantize_nd(k.permute(1, 0, 2)[None], 64, 8)
    qv = Q.quantize_nd(v.permute(1, 0, 2)[None], 64, 8)
    return Q.quantized_sdpa(q.permute(1, 0, 2)[None], qk, qv, scale, causal=True)[0].permute(1, 0, 2)


def nan_q8_pools(kpool, dev="cuda"):
    """8-bit pools for a bf16 pool of kpool's size in which NOTHING is written yet: 0xff bytes, NaN | NaN (scale | bias) words"""
    n = kpool.numel()
    return (torch.full((n,), 0xff, dtype=torch.uint8, device=dev), torch.full((n,), 0xff, dtype=torch.uint8, device=dev),
            torch.full((n // 64,), 0x7fc07fc0, dtype=torch.int32, device=dev),
            torch.full((n // 64,), 0x7fc07fc0, dtype=torch.int32, device=dev))
