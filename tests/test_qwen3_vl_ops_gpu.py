"""The three operator forms the Qwen3-VL family adds, on the GPU against the torch restatement (tests/qwen3_vl_ref.py):
QK-norm + interleaved M-RoPE + paged KV write (vlm_mrope_kvwrite_scaled with a negative mrope_sec0), the tanh-GELU GEMM
epilogue (VLM_EPI_GELU_TANH) and the DeepStack row add (vlm_scatter_image_rows with a negative row count)."""
import hashlib

import pytest
import torch

from oracle import ops as O
from tests import qwen3_vl_ref as R
from tests.attn_exact import VSLOT
from tests.helpers import bf16_close

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
D = 128
SECTION = [24, 20, 20]
EPS = 1e-6


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def _norm_weights(seed):
    """drawn around 1, not equal to 1"""
    g = torch.Generator().manual_seed(seed)
    qw, kw = ((1 + 0.2 * torch.randn(D, generator=g)).to(BF) for _ in range(2))
    assert not bool((qw == 1).all()) and not bool((kw == 1).all())
    return qw, kw


def _pools(n_pages, Hkv, fill):
    """pools pre-filled with a sentinel pattern: what the kernel does not write must still be there"""
    g = torch.Generator().manual_seed(fill)
    kpool = torch.randn(n_pages, Hkv, D // 8, 64, 8, generator=g).to(BF)
    vpool = torch.randn(n_pages, Hkv, D, 64, generator=g).to(BF)
    return kpool, vpool


def _check_pools(out, kpool0, vpool0, kpool, vpool, kv_seq, kv_slot, bt, Hq, Hkv):
    """page contents == the rows the kernel left in the qkv buffer (k) / the untouched v rows, bit for bit, in the layouts the
    attention kernels read; every other pool entry still holds its sentinel"""
    T = out.shape[0]
    o = out.view(T, Hq + 2 * Hkv, D).cpu()
    kp = kpool.cpu().permute(0, 1, 3, 2, 4).reshape(kpool.shape[0], Hkv, 64, D)            # [page, Hkv, token, D]
    vp = vpool.cpu()[..., VSLOT].permute(0, 1, 3, 2)                                         # [page, Hkv, D, slot] -> [page, Hkv, token, D]
    k0 = kpool0.permute(0, 1, 3, 2, 4).reshape(kpool.shape[0], Hkv, 64, D).clone()
    v0 = vpool0[..., VSLOT].permute(0, 1, 3, 2).clone()
    for t in range(T):
        s, slot = int(kv_seq[t]), int(kv_slot[t])
        page, within = int(bt[s, slot // 64]), slot % 64
        assert torch.equal(kp[page, :, within], o[t, Hq:Hq + Hkv]), t
        assert torch.equal(vp[page, :, within], o[t, Hq + Hkv:]), t
        k0[page, :, within] = kp[page, :, within]
        v0[page, :, within] = vp[page, :, within]
    assert torch.equal(kp, k0) and torch.equal(vp, v0)


def _run(vops, qkv, Hq, Hkv, pos3, qw, kw, kv_seq, kv_slot, bt, n_pages, theta=5e6, fill=7):
    inv = O.mrope_inv_freq(D, theta)
    tab = vops.qknorm_table(inv.cuda(), EPS, qw.cuda(), kw.cuda())
    assert tab.dtype == torch.float32 and tab.numel() == D // 2 + 1 + 2 * D
    kpool0, vpool0 = _pools(n_pages, Hkv, fill)
    kpool, vpool = kpool0.cuda(), vpool0.cuda()
    i32 = lambda a: None if a is None else torch.as_tensor(a).to(torch.int32).cuda()   # noqa: E731
    out = vops.mrope_qknorm_kvwrite_(qkv.cuda().clone(), Hq, Hkv, D, i32(pos3[0]), i32(pos3[1]), i32(pos3[2]), tab, SECTION,
                                     kv_seq=i32(kv_seq), kv_slot=i32(kv_slot), block_table=i32(bt), kpool=kpool, vpool=vpool)
    ref = R.qknorm_rope(qkv, (Hq, Hkv, D), pos3, inv, SECTION, qw, kw, EPS)
    return out, ref, (kpool0, vpool0, kpool, vpool)


def _compare(out, ref, qkv, Hq, Hkv, what):
    """the bar of test_mrope_kvwrite_prefill_and_pages (tests/test_ops_gpu.py): 1.01 bf16 ulps + 2e-3 of the rms; v untouched"""
    T = out.shape[0]
    o, r = out.view(T, Hq + 2 * Hkv, D), ref.view(T, Hq + 2 * Hkv, D)
    for name, sl in (("q", slice(0, Hq)), ("k", slice(Hq, Hq + Hkv))):
        ok, rep = bf16_close(o[:, sl], r[:, sl], ulps=1.01, atol_rms=2e-3)
        print(f"qknorm rope {what} {name}: {rep}")
        assert ok, (what, name, rep)
    assert torch.equal(o[:, Hq + Hkv:].cpu(), qkv.view(T, Hq + 2 * Hkv, D)[:, Hq + Hkv:])


@pytest.mark.parametrize("Hq,Hkv", [(4, 2), (16, 8)])
def test_qknorm_mrope_kvwrite_prefill(Hq, Hkv):
    """T = 37 tokens over two sequences, DISTINCT t / h / w positions: every frequency of the interleaved selector - the h / w
    lanes below 60, the boundary at 60 and the frequencies 61 .. 63 that fall back to t - rotates by its own angle"""
    from mlx_vlm_amd import ops as vops

    T = 37
    qkv = rnd(T, (Hq + 2 * Hkv) * D, seed=19 + Hq)
    g = torch.Generator().manual_seed(20)
    pos3 = torch.stack([torch.randint(0, 1000, (T,), generator=g), torch.randint(1000, 2000, (T,), generator=g),
                        torch.randint(2000, 3000, (T,), generator=g)])
    qw, kw = _norm_weights(21)
    kv_seq = torch.cat([torch.zeros(25), torch.ones(12)]).to(torch.int32)          # tokens [0, 25) -> seq 0 slots 50 .. 74 (a page edge)
    kv_slot = torch.cat([torch.arange(25) + 50, torch.arange(12)]).to(torch.int32)
    bt = torch.tensor([[3, 1, 0, 0], [6, 0, 0, 0]], dtype=torch.int32)
    out, ref, pools = _run(vops, qkv, Hq, Hkv, pos3, qw, kw, kv_seq, kv_slot, bt, n_pages=8)
    _compare(out, ref, qkv, Hq, Hkv, f"prefill {Hq}:{Hkv}")
    _check_pools(out, *pools, kv_seq, kv_slot, bt, Hq, Hkv)
    # not vacuous, three ways: the chunked selector, equal positions and unit norm weights each give something else
    inv = O.mrope_inv_freq(D, 5e6)
    far = lambda other: float((other.float() - ref.float()).abs().max()) > 0.1      # noqa: E731
    assert far(R.qknorm_rope(qkv, (Hq, Hkv, D), pos3, inv, SECTION, qw, kw, EPS, interleaved=False))
    assert far(R.qknorm_rope(qkv, (Hq, Hkv, D), pos3[:1].expand(3, T), inv, SECTION, qw, kw, EPS))
    assert far(R.qknorm_rope(qkv, (Hq, Hkv, D), pos3, inv, SECTION, torch.ones(D, dtype=BF), torch.ones(D, dtype=BF), EPS))
    # the frequencies behind the section boundary take the t position: moving h and w alone leaves columns 60 .. 63 (+ 64) as they are
    moved = torch.stack([pos3[0], pos3[1] + 17, pos3[2] + 29])
    out2, _, _ = _run(vops, qkv, Hq, Hkv, moved, qw, kw, kv_seq, kv_slot, bt, n_pages=8)
    a, b = out.view(T, -1, D)[:, :Hq + Hkv].cpu(), out2.view(T, -1, D)[:, :Hq + Hkv].cpu()
    t_cols = [f for f in range(64) if not ((f % 3 == 1 or f % 3 == 2) and f < 60)]
    assert t_cols[-4:] == [60, 61, 62, 63]
    cols = torch.tensor(t_cols + [f + 64 for f in t_cols])
    assert torch.equal(a[..., cols], b[..., cols]) and not torch.equal(a, b)


@pytest.mark.parametrize("Hq,Hkv", [(4, 2), (16, 8)])
@pytest.mark.parametrize("B", [1, 3, 16])
def test_qknorm_mrope_kvwrite_decode_rows(B, Hq, Hkv):
    """B decode rows - the three positions equal, row b = block-table row b - at slots around a page edge, through a
    non-identity block table, positions up to about 1000: only the norm is new against the chunked form there"""
    from mlx_vlm_amd import ops as vops

    qkv = rnd(B, (Hq + 2 * Hkv) * D, seed=40 + B + Hq)
    slots = torch.tensor([[63, 64, 70][b % 3] for b in range(B)], dtype=torch.int32)
    pos = torch.tensor([(997 - 61 * b) % 1000 for b in range(B)])
    qw, kw = _norm_weights(41)
    perm = torch.randperm(2 * B, generator=torch.Generator().manual_seed(B)) + 1          # page 0 is nobody's
    bt = perm.reshape(B, 2).to(torch.int32)
    out, ref, pools = _run(vops, qkv, Hq, Hkv, pos[None].expand(3, B), qw, kw, None, slots, bt, n_pages=2 * B + 1)
    _compare(out, ref, qkv, Hq, Hkv, f"decode B={B} {Hq}:{Hkv}")
    _check_pools(out, *pools, torch.arange(B), slots, bt, Hq, Hkv)
    # equal positions: the interleaved and the chunked selector give the same rotation (compute_mrope_frequencies' 2-D branch)
    inv = O.mrope_inv_freq(D, 5e6)
    assert torch.equal(ref, R.qknorm_rope(qkv, (Hq, Hkv, D), pos[None].expand(3, B), inv, SECTION, qw, kw, EPS, interleaved=False))


def test_qknorm_form_refuses_what_it_is_not_built_for():
    from mlx_vlm_amd import _lib, ops as vops

    qkv = rnd(2, 6 * 64, seed=1).cuda()
    pos = torch.zeros(2, dtype=torch.int32).cuda()
    tab = torch.zeros(32 + 1 + 128, dtype=torch.float32).cuda()
    with pytest.raises(_lib.VlmHipError, match="unsupported shape"):       # head_dim 64
        vops.mrope_qknorm_kvwrite_(qkv, 2, 2, 64, pos, pos, pos, tab, [12, 10, 10])
    with pytest.raises(ValueError):
        vops.mrope_qknorm_kvwrite_(rnd(2, 4 * D).cuda(), 2, 1, D, pos, pos, pos, tab, SECTION)


# The chunked form (every family before this one) on fixed seeded inputs: the SHA-256 of what the PARENT commit's library wrote
# (q / k rows in place, both pools), recorded on an MI355X.  The QK-norm form is a kernel of its own; this pins that the launch
# behind a non-negative mrope_sec0 still writes the parent's bits.
CHUNKED_FORM_DIGEST = {
    "plain": "9afdee3a7b0e5fd21aca23d2d5c6852d6635f1e813457f4080f386f1af584c23",
    "scaled": "95a29eb8a6ae2a167f789ce2a21078c9b94b018850575c0cd719572071d527b9",
}


def _chunked_form_bytes(scale):
    from mlx_vlm_amd import ops as vops

    T, Hq, Hkv = 150, 4, 2
    qkv = rnd(T, (Hq + 2 * Hkv) * D, seed=19)
    pos = torch.randint(0, 3000, (3, T), generator=torch.Generator().manual_seed(20)).int().cuda()
    kv_seq = torch.cat([torch.zeros(100), torch.ones(50)]).to(torch.int32).cuda()
    kv_slot = torch.cat([torch.arange(100) + 5, torch.arange(50)]).to(torch.int32).cuda()
    bt = torch.tensor([[3, 1, 0, 0], [6, 0, 0, 0]], dtype=torch.int32).cuda()
    kpool = torch.zeros(8, Hkv, D // 8, 64, 8, dtype=BF, device="cuda")
    vpool = torch.zeros(8, Hkv, D, 64, dtype=BF, device="cuda")
    out = vops.mrope_kvwrite_(qkv.cuda().clone(), Hq, Hkv, D, pos[0], pos[1], pos[2], O.mrope_inv_freq(D, 1e6).cuda(), 16, 24, kv_seq,
                              kv_slot, bt, kpool, vpool, qk_scale=scale)
    return b"".join(t.cpu().contiguous().view(torch.int16).numpy().tobytes() for t in (out, kpool, vpool))


@pytest.mark.parametrize("form", ["plain", "scaled"])
def test_chunked_form_writes_the_parents_bits(form):
    digest = hashlib.sha256(_chunked_form_bytes(None if form == "plain" else 1.1875)).hexdigest()
    print(f"chunked form {form}: sha256 {digest}")
    assert digest == CHUNKED_FORM_DIGEST[form]


# ---------------------------------------------------------------- tanh-GELU epilogue
def _gelu_case(M, N, K):
    a, w, b = rnd(M, K, seed=3 + M), rnd(N, K, seed=4 + N, scale=0.08), rnd(N, seed=5, scale=0.5)
    return a, w, b, R.gelu_tanh(O.linear(a, w, b))


@pytest.mark.parametrize("M,N,K", [(5, 64, 64), (200, 512, 256), (1024, 4096, 1024)])
def test_gemm_bias_gelu_tanh(M, N, K):
    """VLM_EPI_BIAS | VLM_EPI_GELU_TANH against oracle linear + bias followed by the restatement's typed tanh-GELU, at the
    bar the issue gives the fast-GELU epilogue: 2 bf16 ulps + 2e-2 of the rms"""
    from mlx_vlm_amd import ops as vops

    a, w, b, ref = _gelu_case(M, N, K)
    out = vops.gemm(a.cuda(), w.cuda(), bias=b.cuda(), epilogue=vops.EPI_BIAS | vops.EPI_GELU_TANH)
    ok, rep = bf16_close(out, ref, ulps=2, atol_rms=2e-2)
    print(f"GEMM BIAS|GELU_TANH {M}x{N}x{K}: {rep}")
    assert ok, rep
    # it is the tanh form: the fast form x * sigmoid(1.702 x) of the same linear output is an order of magnitude further away
    rel = lambda r: float((out.float().cpu() - r.float()).pow(2).mean().sqrt() / r.float().pow(2).mean().sqrt())   # noqa: E731
    assert rel(O.gelu_fast(O.linear(a, w, b))) > 10 * rel(ref)
    plain = vops.gemm(a.cuda(), w.cuda(), bias=b.cuda(), epilogue=vops.EPI_BIAS)
    assert not torch.equal(out, plain)


def test_gemm_gelu_tanh_every_tile_staging_and_split_form():
    """every kernel form that takes VLM_EPI_GELU_FAST takes the tanh form: register and LDS-DMA staging and the 256 x 256 kernel
    in its variants are bit-identical to each other (as they are for the other epilogues); split-K (forced x4) and the forced
    small tiles agree with the oracle at the bar above"""
    from mlx_vlm_amd import ops as vops

    a, w, b, ref = _gelu_case(1024, 4096, 1024)
    a, w, b = a.cuda(), w.cuda(), b.cuda()
    epi = vops.EPI_BIAS | vops.EPI_GELU_TANH
    outs = {}
    try:
        for mode in (1, 2, 3, 4, 6, 7, 10, 8, 9, 101, 102, 103, 141):
            vops.gemm_set_staging(mode)
            outs[mode] = vops.gemm(a, w, bias=b, epilogue=epi)
    finally:
        vops.gemm_set_staging(0)
    for mode in (2, 3, 4, 6, 7, 10, 8):
        assert torch.equal(outs[mode], outs[1]), mode
    for mode, out in outs.items():
        ok, rep = bf16_close(out, ref, ulps=2, atol_rms=2e-2)
        assert ok, (mode, rep)
    # a long-K shape that takes split-K on its own (few tiles, K >= 2048)
    a2, w2, b2, ref2 = _gelu_case(130, 264, 2048)
    out2 = vops.gemm(a2.cuda(), w2.cuda(), bias=b2.cuda(), epilogue=epi)
    ok, rep = bf16_close(out2, ref2, ulps=2, atol_rms=2e-2)
    assert ok, rep


def test_gelu_tanh_typed_graph_on_a_sweep():
    """every bf16 value in [-8, 8] through the epilogue (identity weight, zero bias: the linear output IS the input) against the
    typed graph.  tanh on the device is 1 - 2 / (1 + exp2(.)) on the transcendental units, within ~1e-7 of the CPU's tanh: the
    bf16 rounding of tanh - a step of 2^-9 or more above 0.25 - flips for about 1e-7 / 2^-9 = 5e-5 of the values, i.e. about
    one of the 17 k here, and such a flip may move T(1 + tanh) by one step.  So: the epilogue's bar for every value, and at
    least 99 % of them bit-equal; from |x| = 6 on tanh has saturated to +-1 in bf16 and nothing can flip."""
    from mlx_vlm_amd import ops as vops

    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16).view(BF)
    x = bits[torch.isfinite(bits.float()) & (bits.float().abs() <= 8)]
    n = (x.numel() + 63) // 64 * 64
    xs = torch.zeros(n, dtype=BF)
    xs[:x.numel()] = x
    a = xs.reshape(-1, 64)
    out = vops.gemm(a.cuda(), torch.eye(64, dtype=BF).cuda(), bias=torch.zeros(64, dtype=BF).cuda(),
                    epilogue=vops.EPI_BIAS | vops.EPI_GELU_TANH).cpu()
    ref = R.gelu_tanh(a)
    ok, rep = bf16_close(out, ref, ulps=2, atol_rms=2e-2, frac_exact=0.99)
    print(f"tanh-GELU sweep over {x.numel()} values: {rep}")
    assert ok, rep
    big = a.float().abs() >= 6
    assert torch.equal(out[big], ref[big])


# ---------------------------------------------------------------- DeepStack add
def test_deepstack_add_rows():
    """h[rows[i]] += e[i]: 7 rows of 256 columns, row 0 and the last row among them - torch.equal against the typed add"""
    from mlx_vlm_amd import ops as vops

    T, Dh = 23, 256
    h, e = rnd(T, Dh, seed=50), rnd(7, Dh, seed=51)
    rows = torch.tensor([0, 22, 5, 9, 10, 17, 3], dtype=torch.int32)
    ref = h.clone()
    ref[rows.long()] = O.add(h[rows.long()], e)
    hd = h.cuda().clone()
    out = vops.add_rows_(e.cuda(), rows.cuda(), hd)
    assert out is hd and torch.equal(hd.cpu(), ref)
    untouched = torch.tensor([i for i in range(T) if i not in rows.tolist()])
    assert torch.equal(hd.cpu()[untouched], h[untouched]) and not torch.equal(hd.cpu()[rows.long()], h[rows.long()])
    # a strided destination (rows of a wider buffer) and an empty list
    wide = torch.zeros(T, 2 * Dh, dtype=BF, device="cuda")
    wide[:, :Dh] = h.cuda()
    vops.add_rows_(e.cuda(), rows.cuda(), wide[:, :Dh])
    assert torch.equal(wide[:, :Dh].cpu(), ref) and not bool(wide[:, Dh:].any())
    vops.add_rows_(e.cuda()[:0], rows.cuda()[:0], hd)
    assert torch.equal(hd.cpu(), ref)
    # the scatter form of the same entry point still replaces
    vops.scatter_rows_(e.cuda(), rows.cuda(), hd)
    assert torch.equal(hd.cpu()[rows.long()], e)
