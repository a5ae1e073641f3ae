"""The kernels of the one-row decode step order their parameters for the kernel-argument preload (csrc/gemv_bf16.hip,
csrc/attn_decode.hip; build.py -amdgpu-kernarg-preload-count).  A reordered signature goes wrong when two arguments of
one type swap, and equal strides or aliased operands hide exactly that, so every case here runs on pairwise different
leading dimensions (ldx = K + 8, ldw = K + 16, ldy = N + 8, ldres = N + 24 wherever the entry point takes one) and on a
buffer of its own per operand, and is held two ways:

  * bit equality with the same op on contiguous operands - a stride does not enter the arithmetic;
  * the exactly rounded host result (float64, rounded once to bf16 at the reference's rounding points) with the bars of
    tests/test_op_noise_gpu.py: GEMV and norms <= 1e-4 rel-rms, decode attention <= 5e-4; the greedy tail bit for bit
    (tests/sampler_exact.py).

Smallest shapes that reach every form: K = 72 (9 chunks of 8 against 64 lanes), N = 10 (against 8 rows per workgroup),
M = 1, 2, 4, 8; split-K at K = 3592 (just past the row-wave limit) with N = 12 and 8; the qkv form at hidden 72 with 6 + 1
heads of 128; the page-split attention and the merging o_proj at 6 + 1 heads over 1, 64 and 65 tokens; the tail at V = 1000.
The GEMV entry point offers bias + residual with no prologue, and residual behind the norm prologue, at no row count
(VLM_ERR_ARG before anything is enqueued): those cases assert that the refusal does not depend on the strides either.
Weights (and x where no norm runs) lie on a coarse binary lattice, so their fp32 sums are exact in any order and a 1e-4
bar over ten outputs is not decided by one legitimate flip of a last bit."""
import pytest
import torch

from oracle import ops as O
from tests import attn_exact as A
from tests import sampler_exact as S

pytestmark = pytest.mark.gpu
BF, F64 = torch.bfloat16, torch.float64
NAN = float("nan")
K, N = 72, 10


@pytest.fixture(scope="module")
def vops():
    from mlx_vlm_amd import ops

    return ops


def lattice(*shape, seed, step, span):
    """multiples of `step` in [-span, span] (bf16-exact)"""
    g = torch.Generator().manual_seed(seed)
    n = int(span / step)
    return (torch.randint(-n, n + 1, shape, generator=g).to(torch.float32) * step).to(BF)


def rnd(*shape, seed, s=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * s).to(BF)


def pitched(t, ld):
    """the values of t [rows, n] as a view with leading dimension ld of a NaN-filled device buffer of its own"""
    buf = torch.full((t.shape[0], ld), NAN, dtype=t.dtype, device="cuda")
    buf[:, :t.shape[1]] = t.cuda()
    return buf[:, :t.shape[1]]


def bf(x64):
    return A.rne_bf16(x64).to(BF)


def rel_rms(a, b):
    a, b = a.detach().cpu().to(F64), b.detach().cpu().to(F64)
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


def held(name, got, exact, bar):
    d = rel_rms(got, exact)
    print(f"KERNARG-ORDER {name:70s} vs exact {d:.3e}   bar {bar:.0e}")
    assert bool(torch.isfinite(got.float()).all()), name
    assert d <= bar, (name, d, bar)


def rmsnorm_exact(x, w, eps=1e-6):
    xf = x.to(F64)
    inv = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return bf(bf(xf * inv).to(F64) * w.to(F64))


# ------------------------------------------------------------------ row-wave and split-K GEMV
EPIS = ["none", "bias", "residual", "bias+residual", "swiglu"]


def gemv_exact(xe, W, b, r, epi):
    acc = xe.to(F64) @ W.to(F64).T
    if epi == "swiglu":
        return O.swiglu(bf(acc[:, 0::2]), bf(acc[:, 1::2]))
    if "bias" in epi:
        acc = acc + b.to(F64)
    if "residual" in epi:
        return bf(bf(acc).to(F64) + r.to(F64))
    return bf(acc)


def run_gemv(vops, x, W, b, r, nw, epi, k, n, pitch):
    code = {"none": 0, "bias": vops.EPI_BIAS, "residual": vops.EPI_RESIDUAL, "bias+residual": vops.EPI_BIAS | vops.EPI_RESIDUAL,
            "swiglu": vops.EPI_SWIGLU}[epi]
    n_out = n // 2 if epi == "swiglu" else n
    M = x.shape[0]
    ldx, ldw, ldy, ldres = (k + 8, k + 16, n + 8, n + 24) if pitch else (k, k, n_out, n)
    y = vops.gemv(pitched(x, ldx), pitched(W, ldw), bias=b.clone().cuda() if "bias" in epi else None,
                  res=pitched(r, ldres) if "residual" in epi else None, norm_w=nw.clone().cuda() if nw is not None else None,
                  out=pitched(torch.full((M, n_out), NAN, dtype=BF), ldy), eps=1e-6, epilogue=code)
    return y.cpu()


@pytest.mark.parametrize("M", [1, 2, 4, 8])
@pytest.mark.parametrize("pro", ["none", "rmsnorm"])
def test_rowwave_forms_on_distinct_strides(vops, pro, M):
    from mlx_vlm_amd._lib import VlmHipError

    W, b, r = lattice(N, K, seed=1, step=1 / 32, span=0.5), lattice(N, seed=2, step=1 / 16, span=1), lattice(M, N, seed=3, step=1 / 8, span=2)
    if pro == "rmsnorm":
        x, nw = rnd(M, K, seed=4 + M), (1 + 0.1 * torch.randn(K, generator=torch.Generator().manual_seed(5))).to(BF)
        xe = rmsnorm_exact(x, nw)
    else:
        x, nw = lattice(M, K, seed=4 + M, step=1 / 8, span=4), None
        xe = x
    ran = []
    for epi in EPIS:
        try:
            ref = run_gemv(vops, x, W, b, r, nw, epi, K, N, pitch=False)
        except VlmHipError as e:
            # not a form of the library at this (prologue, row count): refused before anything is enqueued, and refused alike
            with pytest.raises(VlmHipError):
                run_gemv(vops, x, W, b, r, nw, epi, K, N, pitch=True)
            print(f"KERNARG-ORDER row-wave {pro} M={M} {epi}: not offered ({e})")
            continue
        got = run_gemv(vops, x, W, b, r, nw, epi, K, N, pitch=True)
        assert torch.equal(got, ref), (pro, M, epi)
        held(f"row-wave GEMV, prologue {pro}, M = {M}, epilogue {epi}", got, gemv_exact(xe, W, b, r, epi), 1e-4)
        ran.append(epi)
    # the forms the one-row step is made of must be among them
    assert {"none", "bias", "swiglu"} <= set(ran) and (pro == "rmsnorm" or "residual" in ran), ran


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("n", [12, 8])
def test_splitk_residual_on_distinct_strides(vops, n, M):
    k = 3592
    x, W = lattice(M, k, seed=10 + M, step=1 / 8, span=4), lattice(n, k, seed=11 + n, step=1 / 32, span=0.5)
    r = lattice(M, n, seed=12, step=1 / 8, span=2)
    ref = run_gemv(vops, x, W, None, r, None, "residual", k, n, pitch=False)
    got = run_gemv(vops, x, W, None, r, None, "residual", k, n, pitch=True)
    assert torch.equal(got, ref)
    held(f"split-K GEMV + residual, K = {k}, N = {n}, M = {M}", got, gemv_exact(x, W, None, r, "residual"), 1e-4)


# ------------------------------------------------------------------ qkv: RMSNorm + GEMV + bias + M-RoPE + paged KV write
HQ, HKV, D = 6, 1, 128


@pytest.mark.parametrize("M", [1, 2])
def test_qkv_rope_kvwrite_on_distinct_positions_and_slots(vops, M):
    hidden, n = K, (HQ + 2 * HKV) * D
    h, nw = rnd(M, hidden, seed=20 + M), (1 + 0.1 * torch.randn(hidden, generator=torch.Generator().manual_seed(21))).to(BF)
    W, b = lattice(n, hidden, seed=22, step=1 / 32, span=0.5), lattice(n, seed=23, step=1 / 16, span=1)
    pos = torch.tensor([37, 1000][:M], dtype=torch.int32)
    slot = torch.tensor([70, 3][:M], dtype=torch.int32)
    inv = O.mrope_inv_freq(D, 1e6)
    max_pages = 4

    def run(ldq):
        kpool = torch.zeros(M * max_pages, HKV, D // 8, 64, 8, dtype=BF, device="cuda")
        vpool = torch.zeros(M * max_pages, HKV, D, 64, dtype=BF, device="cuda")
        out = pitched(torch.full((M, n), NAN, dtype=BF), ldq)
        vops.gemv_qkv_rope_kvwrite(h.cuda(), nw.cuda(), W.cuda(), b.cuda(), HQ, HKV, D, pos.cuda(), slot.cuda(), inv.cuda(), None,
                                   kpool, vpool, out=out, max_pages=max_pages)
        return out.cpu()[:, :HQ * D], kpool.cpu(), vpool.cpu()

    q0, k0, v0 = run(n)
    q1, k1, v1 = run(n + 8)
    assert torch.equal(q1, q0) and torch.equal(k1, k0) and torch.equal(v1, v0)
    # exact: y = bf16(xn W^T + b); q / k heads rotated on (j, j + D/2) by pos * inv_freq[j]; v as it is
    y = bf(rmsnorm_exact(h, nw).to(F64) @ W.to(F64).T + b.to(F64)).to(F64).view(M, HQ + 2 * HKV, D)
    ang = pos.to(F64)[:, None] * inv.to(F64)[None, :]
    cs, sn = torch.cos(ang)[:, None, :], torch.sin(ang)[:, None, :]
    lo, hi = y[:, :HQ + HKV, :D // 2], y[:, :HQ + HKV, D // 2:]
    rot = bf(torch.cat([lo * cs - hi * sn, hi * cs + lo * sn], -1))
    kp = k1.permute(0, 1, 3, 2, 4).reshape(M * max_pages, HKV, 64, D)
    vp = v1[..., A.VSLOT].permute(0, 1, 3, 2)
    for m in range(M):
        page, within = m * max_pages + int(slot[m]) // 64, int(slot[m]) % 64
        got = torch.cat([q1[m], kp[page, :, within].reshape(-1), vp[page, :, within].reshape(-1)])
        exact = torch.cat([rot[m].reshape(-1), bf(y[m, HQ + HKV:]).reshape(-1)])
        held(f"qkv + M-RoPE + KV write, row {m} of {M} (pos {int(pos[m])}, slot {int(slot[m])})", got, exact, 1e-4)
    # one token per row went into the pools, nothing else
    assert int((k1 != 0).sum()) <= M * HKV * D and int((v1 != 0).sum()) <= M * HKV * D


# ------------------------------------------------------------------ page-split attention + the o_proj that merges it
@pytest.mark.parametrize("add", [0, 1])
@pytest.mark.parametrize("ctx", [1, 64, 65])
def test_pagesplit_attention_and_merging_oproj(vops, ctx, add):
    S_, sc, hd = 16, D ** -0.5, HQ * D
    q, k, v = rnd(1, hd, seed=30 + ctx), rnd(ctx, HKV, D, seed=31 + ctx), rnd(ctx, HKV, D, seed=32 + ctx)
    bt, kpool, vpool, max_pages = A.build_pools([k], [v], seed=ctx, identity=True)      # unwritten slots hold NaN
    exact = A.decode_exact(q, [k], [v], sc)
    kd, vd = kpool.cuda(), vpool.cuda()
    kv_len = torch.tensor([ctx - add], dtype=torch.int32).cuda()
    Wo, res = lattice(N, hd, seed=33, step=1 / 32, span=0.5), lattice(1, N, seed=34, step=1 / 8, span=2)
    exact_o = bf(bf(exact.to(F64) @ Wo.to(F64).T).to(F64) + res.to(F64))
    outs = []
    for qd in (q.cuda(), pitched(q, hd + 8)):
        row = []
        for table in (None, bt.cuda()):      # identity layout (the step's form) and through a block table
            row.append(vops.attn_decode_paged_split(qd, kd, vd, table, kv_len, add, HQ, HKV, D, sc, S_, max_pages=max_pages).cpu())
            po, pml = vops.attn_decode_paged_split(qd, kd, vd, table, kv_len, add, HQ, HKV, D, sc, S_, max_pages=max_pages, merge=False)
            for ldh in (N, N + 8):
                row.append(vops.gemv_attn_out_bf16_(po, pml, Wo.cuda(), pitched(res, ldh), HQ, D).cpu())
        outs.append(row)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    for i, what in enumerate(["identity pages", "block table"]):
        held(f"page-split attention, last arriver merges, {what}, ctx {ctx} (+{add})", outs[1][3 * i], exact, 5e-4)
        assert torch.equal(outs[1][3 * i + 1], outs[1][3 * i + 2])
        held(f"partials merged in the o_proj prologue + residual, {what}, ctx {ctx} (+{add})", outs[1][3 * i + 2], exact_o, 5e-4)


# ------------------------------------------------------------------ greedy tail
@pytest.mark.parametrize("B", [1, 2])
def test_greedy_tail_on_distinct_pitches(vops, B):
    V, Dm = 1000, 64
    head = S.batch_rows(V, B)
    embed = torch.randn(V, Dm, generator=torch.Generator().manual_seed(V + B)).to(BF).cuda()
    got = []
    for ld, ldh in ((V, Dm), (V + 8, Dm + 8)):
        ctx = torch.arange(10, 10 + B, dtype=torch.int32, device="cuda")
        pos = torch.arange(20, 20 + B, dtype=torch.int32, device="cuda")
        step = torch.zeros(1, dtype=torch.int32, device="cuda")
        tok = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        hid = pitched(torch.zeros(B, Dm, dtype=BF), ldh)
        lp = vops.sample_greedy_advance(pitched(head.x, ld), tok, ctx, pos, step, embed, hid)
        torch.cuda.synchronize()
        S.check_head(f"greedy tail ld {ld} ldh {ldh}", head, lp, tok)
        assert torch.equal(hid, embed[head.tok.cuda()])
        assert ctx.tolist() == list(range(11, 11 + B)) and pos.tolist() == list(range(21, 21 + B)) and int(step[0]) == 1
        got.append((lp.cpu(), tok.cpu(), hid.cpu()))
    assert all(torch.equal(a, b) for a, b in zip(*got))
