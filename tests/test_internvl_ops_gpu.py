"""GPU parity, operator level, of what the InternVL family adds to the library: the layer-scale GEMM epilogue
(VLM_EPI_BIAS | VLM_EPI_RESIDUAL | VLM_EPI_LAYERSCALE) in every tile, staging and split form, and the encoder-layer loop that
runs it (vlm_encoder_forward with the bit in act_epilogue).

Reference: tests/internvl_ref.py::layerscale_epilogue, the typed graph of the reference's encoder layer (x + ls * Linear(.): fp32
accumulate, then one rounding each after the bias, the multiply and the add), itself pinned to the reference's files bit for bit
by tests/test_internvl_cpu.py.  Bar of the random-operand tests: the one tests/test_ops_gpu.py::test_gemm_epilogues holds the
`bias_res` epilogue to - bf16_close(ulps=3) (3 * 2^-7 |ref| + 2e-3 rms(ref) per element).  The lattice tests are bit-exact.

Which form the dispatcher picks (csrc/gemm_bf16.hip::launch_epi / gemm_dispatch), (M rows, N columns, K):
    (200, 256, 128)    16 tiles, K < 2048                    -> 64 x 64 tiles, LDS-DMA staging, 4-stage K loop
    (77, 192, 320)     ragged M (77 = 64 + 13), N = 3 x 64   -> 64 x 64, rows and a whole tile column clamped
    (1025, 1024, 1024) the wo GEMM of one 448-px tile: 272 tiles of 64 x 64 (>= 256: no split-K, < 200 wider tiles) -> 64 x 64
    (130, 1024, 4096)  the fc2 shape at few rows: 48 tiles, K >= 2048 -> split-K x 8: 64 x 64 partial tiles + the reduce kernel, which carries the epilogue
    (300, 264, 2048)   25 tiles -> split-K x 8 at exactly 4 K tiles per split, N = 264 = 4 x 64 + 8: a ragged last tile column
    (24, 256, 512)     <= 32 rows -> the 32 x 64 tile
    (50, 128, 1024)    <= 64 rows, K >= 1024 -> the skinny split-K (32 .. 64 rows: 64 x 64 partial tiles)
    (20, 256, 2048)    <= 32 rows, K >= 2048 -> split-K over 32 x 64 partial tiles
    (129, 136, 72)     K % 64 != 0 -> global -> VGPR -> LDS staging (64 x 64)
and, forced through vlm_gemm_set_staging (the tower's shapes at 2 .. 13 tiles take these by themselves: 64 x 128 at 2050 rows,
128 x 128 at 4100, the 256 x 256 / 256 x 192 phased kernel at 13325 - too large for a quick test, so they are forced on small ones):
    102 / 103          64 x 128 and 128 x 128 tiles          1    register staging on a K % 64 == 0 shape
    143                split-K x 4 forced (64 x 64 partial tiles + the reduce kernel)
    3 / 6 / 7          the 256-wide phased kernel: automatic width, 256 x 192, 256 x 256
    4                  its two-phase variant                 10   its persistent tile loop (own chunked epilogue)
"""
import numpy as np
import pytest
import torch

from oracle import ops as O
from tests import internvl_ref as R
from tests.helpers import bf16_close

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

AUTO = [(200, 256, 128), (77, 192, 320), (1025, 1024, 1024), (130, 1024, 4096), (300, 264, 2048), (24, 256, 512), (50, 128, 1024),
        (20, 256, 2048), (129, 136, 72)]
FORCED = [((300, 264, 2048), 102), ((300, 264, 2048), 103), ((300, 264, 2048), 1), ((300, 264, 2048), 143), ((300, 520, 192), 3),
          ((300, 520, 192), 6), ((513, 264, 320), 7), ((300, 520, 192), 4), ((777, 520, 192), 10)]
CASES = [(s, 0) for s in AUTO] + FORCED


@pytest.fixture(scope="module")
def vops():
    from mlx_vlm_amd import ops

    return ops


def _operands(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(BF)   # noqa: E731
    a, w = rn(M, K), rn(N, K, sc=1.4 / K ** 0.5)
    b, r = rn(N, sc=0.5), rn(M, N)
    ls = (0.05 + 0.45 * torch.rand(N, generator=g)).to(BF)
    return a, w, b, ls, r


def _run(vops, mode, a, w, bias2, res, out=None, epi=None):
    epi = vops.EPI_BIAS | vops.EPI_RESIDUAL | vops.EPI_LAYERSCALE if epi is None else epi
    try:
        vops.gemm_set_staging(mode)
        return vops.gemm(a, w, bias=bias2, res=res, out=out, epilogue=epi)
    finally:
        vops.gemm_set_staging(0)


@pytest.mark.parametrize("shape,mode", CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}-m{m}" for s, m in CASES])
def test_layerscale_epilogue_every_form(vops, shape, mode):
    """(1) against the typed restatement at the bias_res bar; (2) with ls == 1 bit-identical to the existing BIAS | RESIDUAL
    epilogue of the same form (x * 1.0 is exact); (3) in place (res is C), as the encoder loop calls it"""
    M, N, K = shape
    a, w, b, ls, r = _operands(M, N, K, seed=M + N + K)
    ref = R.layerscale_epilogue(a, w, b, ls, r)
    ad, wd, rd = a.cuda(), w.cuda(), r.cuda()
    b2 = vops.bias_scale(b, ls).cuda()
    out = _run(vops, mode, ad, wd, b2, rd)
    ok, rep = bf16_close(out, ref, ulps=3)
    assert ok, (shape, mode, rep)
    assert not bf16_close(out, O.add(r, O.linear(a, w, b)), ulps=3)[0]                  # the scale is not a no-op here
    ones = _run(vops, mode, ad, wd, vops.bias_scale(b, torch.ones(N)).cuda(), rd)
    plain = _run(vops, mode, ad, wd, b.cuda(), rd, epi=vops.EPI_BIAS | vops.EPI_RESIDUAL)
    assert torch.equal(ones, plain), int((ones != plain).sum())
    x = rd.clone()
    got = _run(vops, mode, ad, wd, b2, x, out=x)
    assert got.data_ptr() == x.data_ptr() and torch.equal(x, out)


LATTICE = [((200, 256, 128), 0), ((130, 1024, 4096), 0), ((300, 264, 2048), 0), ((24, 256, 512), 0), ((129, 136, 72), 0),
           ((300, 264, 2048), 102), ((300, 264, 2048), 103), ((300, 520, 192), 6), ((513, 264, 320), 7), ((300, 520, 192), 4),
           ((777, 520, 192), 10)]


@pytest.mark.parametrize("shape,mode", LATTICE, ids=[f"{s[0]}x{s[1]}x{s[2]}-m{m}" for s, m in LATTICE])
def test_layerscale_epilogue_lattice_is_bit_exact(vops, shape, mode):
    """operands on which every partial sum is an exact integer (tests/internvl_ref.py::lattice_operands, shown exact on the CPU
    by tests/test_internvl_cpu.py): the summation order drops out and the result must equal the restatement BIT FOR BIT - a
    wrong column of bias or ls, a scale taken from the bias row, or a result rounded once instead of per step cannot pass.  Every column has its own
    (bias, ls) pair and ls has four values, so a shifted or clamped column index shows."""
    M, N, K = shape
    a, w, b, ls, r = R.lattice_operands(M, N, K, seed=K + N)
    ref = R.layerscale_epilogue(a, w, b, ls, r)
    out = _run(vops, mode, a.cuda(), w.cuda(), vops.bias_scale(b, ls).cuda(), r.cuda()).cpu()
    assert torch.equal(out, ref), (int((out != ref).sum()), np.argwhere((out != ref).numpy())[:4].tolist())
    if K >= 2048:      # |acc| passes 256 often enough: rounding once at the end instead of before the residual add changes bits
        y32 = a.float() @ w.float().T + b.float()
        assert not torch.equal((r.float() + y32 * ls.float()).to(BF), ref)


def test_layerscale_flag_is_refused_outside_its_combination(vops):
    from mlx_vlm_amd._lib import VlmHipError

    a, w, b, ls, r = (t.cuda() for t in _operands(64, 64, 64, seed=1))
    b2 = vops.bias_scale(b, ls).cuda()
    for epi in (vops.EPI_LAYERSCALE, vops.EPI_BIAS | vops.EPI_LAYERSCALE, vops.EPI_RESIDUAL | vops.EPI_LAYERSCALE,
                vops.EPI_BIAS | vops.EPI_RESIDUAL | vops.EPI_LAYERSCALE | vops.EPI_GELU_ERF):
        with pytest.raises(VlmHipError):
            vops.gemm(a, w, bias=b2, res=r, epilogue=epi)


# ------------------------------------------------------------------ the encoder loop
def _tower(vops, act_bits):
    cfg = R.tiny_cfg("qwen2")
    W = {k: v.to(BF) for k, v in R.random_weights(cfg, seed=1234, dtype=torch.float32, tower_only=True).items()}
    w = {}
    for i in range(cfg.vision.num_hidden_layers):
        p = f"vision_model.encoder.layers.{i}."
        g = lambda n: W[p + n].cuda().contiguous()   # noqa: E731
        ls_on = bool(act_bits & vops.EPI_LAYERSCALE)
        w.update({f"{i}.ln1w": g("norm1.weight"), f"{i}.ln1b": g("norm1.bias"), f"{i}.ln2w": g("norm2.weight"), f"{i}.ln2b": g("norm2.bias"),
                  f"{i}.wqkv": g("attn.qkv.weight"), f"{i}.bqkv": g("attn.qkv.bias"), f"{i}.wo": g("attn.proj.weight"),
                  f"{i}.bo": vops.bias_scale(g("attn.proj.bias"), g("ls1")) if ls_on else g("attn.proj.bias"),
                  f"{i}.w1": g("mlp.fc1.weight"), f"{i}.b1": g("mlp.fc1.bias"), f"{i}.w2": g("mlp.fc2.weight"),
                  f"{i}.b2": vops.bias_scale(g("mlp.fc2.bias"), g("ls2")) if ls_on else g("mlp.fc2.bias")})
    return cfg, W, w


def _manual_loop(vops, w, x, n_layers, H, hd, eps, act_bits, cu, nqb, scale):
    """the layer loop out of single operator calls: what vlm_encoder_forward enqueues, launch by launch"""
    x = x.clone()
    HD = H * hd
    res_epi = vops.EPI_BIAS | vops.EPI_RESIDUAL | (act_bits & vops.EPI_LAYERSCALE)
    for i in range(n_layers):
        xn = vops.layernorm(x, w[f"{i}.ln1w"], w[f"{i}.ln1b"], eps=eps)
        qkv = vops.gemm(xn, w[f"{i}.wqkv"], bias=w[f"{i}.bqkv"], epilogue=vops.EPI_BIAS)
        att = vops.attn_prefill(qkv[:, :HD], qkv[:, HD:2 * HD], qkv[:, 2 * HD:], cu, nqb, H, H, hd, scale, False, uniform_segments=True)
        vops.gemm(att, w[f"{i}.wo"], bias=w[f"{i}.bo"], res=x, out=x, epilogue=res_epi)
        xn = vops.layernorm(x, w[f"{i}.ln2w"], w[f"{i}.ln2b"], eps=eps)
        h = vops.gemm(xn, w[f"{i}.w1"], bias=w[f"{i}.b1"], epilogue=vops.EPI_BIAS | (act_bits & ~vops.EPI_LAYERSCALE))
        vops.gemm(h, w[f"{i}.w2"], bias=w[f"{i}.b2"], res=x, out=x, epilogue=res_epi)
    return x


@pytest.mark.parametrize("act", ["tanh", "erf"])
def test_encoder_forward_with_layer_scale(vops, act):
    """vlm_encoder_forward with the bit set, tiny tower, 3 tiles of 17 tokens, against the restatement (2e-2 relative rms, the
    towers' bar in tests/test_vlm_family_llava_bunny_gpu.py) and, bit for bit, against the same launches made one by one"""
    bits = {"tanh": vops.EPI_GELU_TANH, "erf": vops.EPI_GELU_ERF}[act] | vops.EPI_LAYERSCALE
    cfg, W, w = _tower(vops, bits)
    v = cfg.vision
    g = torch.Generator().manual_seed(7)
    x0 = torch.randn(3, 17, v.hidden_size, generator=g).to(BF)
    ref = R.vision_tower(W, cfg, None, embeddings=x0, act=act)
    cu = torch.tensor([0, 17, 34, 51], dtype=torch.int32).cuda()
    enc = vops.EncoderLayers(w, v.num_hidden_layers)
    x = x0.reshape(51, -1).cuda().contiguous()
    out = enc.forward_(x.clone(), v.num_attention_heads, 64, v.layer_norm_eps, bits, cu, 3, 64 ** -0.5)
    rel = float((out.float().cpu() - ref.reshape(51, -1).float()).pow(2).mean().sqrt() / ref.float().pow(2).mean().sqrt())
    assert rel < 2e-2, rel
    no_ls = R.vision_tower({k: (torch.ones_like(t) if k.endswith((".ls1", ".ls2")) else t) for k, t in W.items()}, cfg, None, embeddings=x0, act=act)
    assert float((out.float().cpu() - no_ls.reshape(51, -1).float()).pow(2).mean().sqrt() / ref.float().pow(2).mean().sqrt()) > 0.1
    manual = _manual_loop(vops, w, x, v.num_hidden_layers, v.num_attention_heads, 64, v.layer_norm_eps, bits, cu, 3, 64 ** -0.5)
    assert torch.equal(out, manual)


@pytest.mark.parametrize("act_name", ["EPI_GELU_FAST", "EPI_GELU_ERF"])
def test_encoder_forward_without_the_bit_is_unchanged(vops, act_name):
    """bit clear: the loop is the launch sequence it was - BIAS | RESIDUAL behind wo and w2, bo / b2 plain [E] rows - bit for bit"""
    bits = getattr(vops, act_name)
    cfg, W, w = _tower(vops, bits)
    v = cfg.vision
    g = torch.Generator().manual_seed(8)
    x = torch.randn(51, v.hidden_size, generator=g).to(BF).cuda()
    cu = torch.tensor([0, 17, 34, 51], dtype=torch.int32).cuda()
    out = vops.EncoderLayers(w, v.num_hidden_layers).forward_(x.clone(), v.num_attention_heads, 64, v.layer_norm_eps, bits, cu, 3, 64 ** -0.5)
    manual = _manual_loop(vops, w, x, v.num_hidden_layers, v.num_attention_heads, 64, v.layer_norm_eps, bits, cu, 3, 64 ** -0.5)
    assert torch.equal(out, manual)
    W1 = {k: (torch.ones_like(t) if k.endswith((".ls1", ".ls2")) else t) for k, t in W.items()}
    ref = R.vision_tower(W1, cfg, None, embeddings=x.cpu().reshape(3, 17, -1), act="erf") if act_name == "EPI_GELU_ERF" else None
    if ref is not None:
        rel = float((out.float().cpu() - ref.reshape(51, -1).float()).pow(2).mean().sqrt() / ref.float().pow(2).mean().sqrt())
        assert rel < 2e-2, rel
