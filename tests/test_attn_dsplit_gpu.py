"""Bits 8 / 9 (256 / 512) of VLM_TUNE_GEMV_VARIANT (include/vlm_hip.h): the partial-only page-split decode attention
(vlm_attn_decode_paged_split with out == NULL) splits the eight 16-row output tiles of a page over DZ = 2 / 4 workgroups
(grid z).  Every z computes the scores and the softmax statistics as the single workgroup does and keeps its own tiles,
so the partials are the same BYTES: DZ = 2 and 4 are held to DZ = 1 in the same library (DZ = 1 is held to the exact
result by tests/test_attn_exact_gpu.py and tests/test_ops_gpu.py).

G in {1, 6, 7} query heads per kv head (Hkv = 2), B in {1, 2} rows, contexts 1, 63, 64, 65, 700 and 1100 at S = 16
splits (1100 = 18 pages: splits 0 and 1 walk two pages) and 2100 at S = 32, identity layout and a permuted block table.
  * part_ml equal everywhere (z = 0 alone stores it; every split, live or dead, has its pair);
  * part_o equal on every split whose m is finite - a dead split's O bytes are unspecified by contract (the buffers start
    as NaN).  A context of n keys has min(S, ceil(n / 64)) live splits - split s owns pages s, s + S, ... - and the test
    asserts that count for every row and head, so the exclusion cannot hide a live split;
  * with out != NULL (the merging form) the launch is today's: equal output with the bits set."""
import pytest
import torch

from oracle import qwen2_vl as oq
from tests.helpers import build_product_model

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
HKV, D = 2, 128
CASES = [(16, n) for n in (1, 63, 64, 65, 700, 1100)] + [(32, 2100)]
MAX_PAGES = 34                                       # 2100 keys = 33 pages


@pytest.fixture(scope="module")
def dsplit():
    """set(dz): the process-wide switch (travels through vlm_llm_set_tuning: the module builds a tiny model for its handle)"""
    cfg = oq.tiny_cfg()
    W = oq.random_weights(cfg, seed=1234, dtype=BF, std=0.05, embed_std=0.2)
    lm = build_product_model(cfg, W, kv_pool_tokens=1024, max_seqs=2).language_model
    base = lm.TUNING_DEFAULTS["gemv_variant"] & ~(256 | 512)
    yield lambda dz: lm.apply_tuning(gemv_variant=base | {1: 0, 2: 256, 4: 512}[dz])
    lm.apply_tuning()


@pytest.fixture(scope="module")
def pools():
    g = torch.Generator(device="cuda").manual_seed(5)
    n_pages = 2 * MAX_PAGES
    kpool = (torch.randn(n_pages, HKV, D // 8, 64, 8, generator=g, device="cuda") * 0.5).to(BF)
    vpool = (torch.randn(n_pages, HKV, D, 64, generator=g, device="cuda") * 0.5).to(BF)
    perm = torch.randperm(n_pages, generator=torch.Generator().manual_seed(6)).to(torch.int32)
    return kpool, vpool, perm.reshape(2, MAX_PAGES).cuda()


@pytest.mark.parametrize("layout", ["identity", "paged"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("G", [1, 6, 7])
def test_output_tiles_over_grid_z_give_the_bytes_of_one_workgroup(dsplit, pools, G, B, layout):
    from mlx_vlm_amd import ops

    kpool, vpool, table = pools
    Hq = G * HKV
    bt = table[:B].contiguous() if layout == "paged" else None
    g = torch.Generator(device="cuda").manual_seed(7 + G)
    q = torch.randn(B, Hq * D, generator=g, device="cuda").to(BF)
    for S, ctx in CASES:
        lens = [ctx, max(1, ctx - 37)][:B]                            # (row 1: another page count wherever 37 keys cross a page)
        kv_len = torch.tensor([n - 1 for n in lens], dtype=torch.int32, device="cuda")   # the step adds its own key

        def run(dz):
            dsplit(dz)
            return ops.attn_decode_paged_split(q, kpool, vpool, bt, kv_len, 1, Hq, HKV, D, D ** -0.5, S, merge=False,
                                               max_pages=MAX_PAGES)

        po1, ml1 = run(1)
        live = torch.isfinite(ml1[..., 0])                            # [B, Hq, S]
        for b, n in enumerate(lens):
            want = min(S, (n + 63) // 64)
            assert live[b].sum(dim=1).tolist() == [want] * Hq, (S, ctx, b)
            assert bool(live[b, :, :want].all())
        assert bool(torch.isfinite(po1[live]).all())
        for dz in (2, 4):
            po, ml = run(dz)
            assert torch.equal(ml.view(torch.int32), ml1.view(torch.int32)), (S, ctx, dz)
            assert torch.equal(po[live].view(torch.int32), po1[live].view(torch.int32)), (S, ctx, dz)


@pytest.mark.parametrize("layout", ["identity", "paged"])
def test_the_merging_form_keeps_its_grid(dsplit, pools, layout):
    from mlx_vlm_amd import ops

    kpool, vpool, table = pools
    G, B, S = 6, 2, 16
    Hq = G * HKV
    bt = table[:B].contiguous() if layout == "paged" else None
    q = torch.randn(B, Hq * D, generator=torch.Generator(device="cuda").manual_seed(9), device="cuda").to(BF)
    kv_len = torch.tensor([699, 64], dtype=torch.int32, device="cuda")
    outs = []
    for dz in (1, 2, 4):
        dsplit(dz)
        outs.append(ops.attn_decode_paged_split(q, kpool, vpool, bt, kv_len, 1, Hq, HKV, D, D ** -0.5, S, max_pages=MAX_PAGES))
    assert bool(torch.isfinite(outs[0].float()).all())
    assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0])
