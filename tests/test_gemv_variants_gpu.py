"""The launch-shape bits of VLM_TUNE_GEMV_VARIANT (include/vlm_hip.h) change how the one-row GEMVs are cut into
workgroups, never what they compute: a row's sum is the lane partials over its chunks followed by one wavefront
reduction, whichever rows share the wave.  So every bit is held to the BYTES of variant 0:

    4   gate/up (RMSNorm prologue + SwiGLU) at 2 rows per wave     (acts at N >= 8192, K <= 1536)
    8   the head form (RMSNorm prologue, no epilogue) likewise
    16  the o_proj that merges the page-split attention at 4 rows per wave  (Hq * D <= 1536)
    32  non-storing waves of the RMSNorm prologue read x / norm_w through a zero-extent buffer resource

Shapes: K = 512 / 1536 / 3584 (one, three, seven 16-byte chunks per lane), N = 16 / 24 (a single workgroup, a partly
filled one), 8200 (just above the 8192 switch to 4 rows per wave) and 8198 (the rows do not fill the last wave).
Variant 0 itself is pinned once to the oracle with the bars of tests/test_ops_gpu.py.

The variant is process-wide and travels through vlm_llm_set_tuning, so the module builds the tiny model for its
handle and puts the defaults back when it is done."""
import pytest
import torch

from oracle import ops as O
from oracle import qwen2_vl as oq
from tests.helpers import bf16_close, build_product_model

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
BITS = [4, 8, 16, 32, 4 | 8 | 16 | 32]
NS = [16, 24, 8200, 8198]


@pytest.fixture(scope="module")
def variant():
    """set(bits): the process-wide variant (the engine's default bit 0 stays on, as in a decode step)"""
    cfg = oq.tiny_cfg()
    W = oq.random_weights(cfg, seed=1234, dtype=BF, std=0.05, embed_std=0.2)
    lm = build_product_model(cfg, W, kv_pool_tokens=1024, max_seqs=2).language_model
    base = lm.TUNING_DEFAULTS["gemv_variant"] & 3
    yield lambda bits: lm.apply_tuning(gemv_variant=base | bits)
    lm.apply_tuning()


def _rnd(*shape, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(*shape, generator=g, device="cuda") * scale).to(BF)


_norm_inputs = {}


def _norm_case(K, N):
    """one input set per shape, shared by every test that reads it"""
    if (K, N) not in _norm_inputs:
        _norm_inputs[(K, N)] = (_rnd(1, K, seed=10 + K), (1 + 0.1 * _rnd(K, seed=11 + K).float()).to(BF),
                                _rnd(N, K, seed=12 + N, scale=0.05))
    return _norm_inputs[(K, N)]


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", [512, 1536, 3584])
def test_norm_prologue_forms_give_the_bytes_of_variant_0(vops, variant, K, N):
    h, nw, w = _norm_case(K, N)
    variant(0)
    ref_glu = vops.gemv(h, w, norm_w=nw, eps=1e-6, epilogue=vops.EPI_SWIGLU)
    ref_head = vops.gemv(h, w, norm_w=nw, eps=1e-6)
    assert bool(torch.isfinite(ref_glu.float()).all()) and bool(torch.isfinite(ref_head.float()).all())
    for bits in BITS:
        variant(bits)
        # (NaN-filled outputs: a row the launch does not write cannot pass)
        glu = vops.gemv(h, w, norm_w=nw, eps=1e-6, epilogue=vops.EPI_SWIGLU, out=torch.full_like(ref_glu, float("nan")))
        head = vops.gemv(h, w, norm_w=nw, eps=1e-6, out=torch.full_like(ref_head, float("nan")))
        assert torch.equal(glu, ref_glu), (bits, "swiglu")
        assert torch.equal(head, ref_head), (bits, "head")


def _partials(Hq, D, live, seed):
    """16 split slots of which the first `live` hold a page: (m in the log2 domain, l) and fp32 O rows; a dead slot carries
    m = -inf, l = 0 and NaN where its O would be, as the partial-only attention launch leaves it"""
    S = 16
    g = torch.Generator(device="cuda").manual_seed(seed)
    po = torch.randn(1, Hq, S, D, generator=g, device="cuda")
    ml = torch.empty(1, Hq, S, 2, device="cuda")
    ml[..., 0] = torch.randn(1, Hq, S, generator=g, device="cuda") * 3
    ml[..., 1] = torch.rand(1, Hq, S, generator=g, device="cuda") * 50 + 1
    po *= ml[..., 1:2]                                          # O_s is the un-normalised sum: of the order of l_s
    po[:, :, live:] = float("nan")
    ml[:, :, live:, 0] = float("-inf")
    ml[:, :, live:, 1] = 0
    return po, ml


def _merge_ref(po, ml, live):
    """x[h, d] = sum_s 2^(m_s - M) O_s[d] / sum_s 2^(m_s - M) l_s over the live splits, in fp64 -> bf16"""
    m, l, o = ml[0, :, :live, 0].double(), ml[0, :, :live, 1].double(), po[0, :, :live].double()
    f = torch.exp2(m - m.max(dim=1, keepdim=True).values)
    x = (f[..., None] * o).sum(1) / (f * l).sum(1, keepdim=True)
    return x.reshape(1, -1).to(BF)


@pytest.mark.parametrize("live", [1, 9, 16])
@pytest.mark.parametrize("HqD", [(4, 128), (12, 128)])
def test_attn_merge_oproj_forms_give_the_bytes_of_variant_0(vops, variant, HqD, live):
    Hq, D = HqD
    po, ml = _partials(Hq, D, live, seed=70 + live)
    for N in NS + [1538]:          # (below the 8192 switch bit 16 is the one that acts: 1538 leaves its last wave 2 of 4 rows)
        wo, h = _rnd(N, Hq * D, seed=64 + N, scale=0.03), _rnd(1, N, seed=65)
        variant(0)
        ref = vops.gemv_attn_out_bf16_(po, ml, wo, h.clone(), Hq, D)
        assert bool(torch.isfinite(ref.float()).all())
        assert not torch.equal(ref, h)
        for bits in BITS:
            variant(bits)
            assert torch.equal(vops.gemv_attn_out_bf16_(po, ml, wo, h.clone(), Hq, D), ref), (bits, N)


def test_variant_0_is_the_oracles(vops, variant):
    """the reference of the comparisons above, pinned once: the bars of tests/test_ops_gpu.py (3 ulps for the norm prologue
    + SwiGLU and for the head; 3 ulps + 2 % of the output rms behind the merge of the attention partials)"""
    variant(0)
    h, nw, w = _norm_case(1536, 8200)
    xn = O.rms_norm(h.cpu(), nw.cpu(), 1e-6)
    ok, rep = bf16_close(vops.gemv(h, w, norm_w=nw, eps=1e-6, epilogue=vops.EPI_SWIGLU),
                         O.swiglu(O.linear(xn, w.cpu()[0::2]), O.linear(xn, w.cpu()[1::2])), ulps=3)
    assert ok, rep
    ok, rep = bf16_close(vops.gemv(h, w, norm_w=nw, eps=1e-6), O.linear(xn, w.cpu()), ulps=3)
    assert ok, rep
    Hq, D, N, live = 12, 128, 8198, 9
    po, ml = _partials(Hq, D, live, seed=70 + live)
    wo, hh = _rnd(N, Hq * D, seed=64 + N, scale=0.03), _rnd(1, N, seed=65)
    ref = (O.linear(_merge_ref(po, ml, live).cpu(), wo.cpu()).float() + hh.cpu().float()).to(BF)
    ok, rep = bf16_close(vops.gemv_attn_out_bf16_(po, ml, wo, hh.clone(), Hq, D), ref, ulps=3, atol_rms=2e-2)
    assert ok, rep


@pytest.fixture(scope="module")
def vops():
    from mlx_vlm_amd import ops

    return ops
