"""Bit 12 of VLM_TUNE_GEMV_VARIANT and bits 6 .. 10 of vlm_decode_args.flags (include/vlm_hip.h): a one-row step runs its
page-split attention and the o_proj that merges it over EXACTLY as many splits as its context has pages.  The attention
launch writes the (m, l) pairs of a head at a pitch rounded up to even, the o_proj prologue is compiled for the count: S slots,
no clamped address, the pairs of a head as 16-byte loads.  Every split owns at most one page - as under 16 splits - and the
merge adds the live splits in the same order: the partials of the live slots and the residual stream carry the BYTES of the
16-slot form with bits 11 and 12 off.

Operators (Hq 12, Hkv 2, D 128, N = K = 1536, one row; identity and paged layouts): ctx + 1 on both sides of every page
boundary that changes the count's parity, the class or the form (1, 2 | 63, 64 | 65 ... 1023, 1024).  An odd count can only
have run the exact form: the class forms refuse a pitch that is not the split count (VLM_ERR_SHAPE).  One count more than the
context has pages - the step of a lookahead run enqueued across a page boundary - finds a slot with m = -inf and drops it.
At 1025 tokens no count can be named (17 pages): 16 splits, the first walks two pages, the bit changes nothing.

Engine: generate_step on the tiny two-layer Qwen2-VL at lookahead 8 across ctx + 1 = 512 -> 513 (counts 8 -> 9, an even and
an odd pitch) and 1024 -> 1025 (16 -> not named) yields the tokens and `torch.equal` log-probs of the run with the bit off."""
import numpy as np
import pytest
import torch

from oracle import qwen2_vl as oq
from tests.helpers import build_product_model

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
HKV, G, D, MAX_PAGES = 2, 6, 128, 17
HQ = HKV * G
LENS = [1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 576, 577, 640, 641, 768, 769, 1023, 1024]          # ctx + 1
EXACT, CLASSES = 4096, 2048


@pytest.fixture(scope="module")
def tiny():
    cfg = oq.tiny_cfg()
    cfg.text.tie_word_embeddings = False
    W = oq.random_weights(cfg, seed=1234, dtype=BF, std=0.05, embed_std=0.2)
    for k in list(W):
        if k.endswith("o_proj.weight") or k.endswith("down_proj.weight"):
            W[k] = (W[k].float() * 0.5).to(BF)
    W = oq.peak_head(W, cfg, gamma=4.0, stride=389, n_cycle=1000)
    model = build_product_model(cfg, W, kv_pool_tokens=4096, max_seqs=4)
    yield model
    model.language_model.apply_tuning()


def _variant(lm, on):
    base = lm.TUNING_DEFAULTS["gemv_variant"] & ~(CLASSES | EXACT)
    lm.apply_tuning(gemv_variant=base | on)


@pytest.fixture(scope="module")
def pools():
    g = torch.Generator(device="cuda").manual_seed(5)
    kpool = (torch.randn(MAX_PAGES, HKV, D // 8, 64, 8, generator=g, device="cuda") * 0.5).to(BF)
    vpool = (torch.randn(MAX_PAGES, HKV, D, 64, generator=g, device="cuda") * 0.5).to(BF)
    table = torch.randperm(MAX_PAGES, generator=torch.Generator().manual_seed(6)).to(torch.int32).reshape(1, MAX_PAGES).cuda()
    q = torch.randn(1, HQ * D, generator=g, device="cuda").to(BF)
    wo = (torch.randn(HQ * D, HQ * D, generator=g, device="cuda") * 0.03).to(BF)
    h = torch.randn(1, HQ * D, generator=g, device="cuda").to(BF)
    return kpool, vpool, table, q, wo, h


def _run(pools, layout, n, S, pitch=None):
    """partial-only attention over S splits at ctx + 1 = n, then the o_proj that merges them -> (part_o, part_ml, h)"""
    from mlx_vlm_amd import ops

    kpool, vpool, table, q, wo, h = pools
    bt = table if layout == "paged" else None
    kv_len = torch.tensor([n - 1], dtype=torch.int32, device="cuda")            # the step adds its own key
    po, ml = ops.attn_decode_paged_split(q, kpool, vpool, bt, kv_len, 1, HQ, HKV, D, D ** -0.5, S, merge=False, max_pages=MAX_PAGES,
                                         ml_pitch=pitch)
    return po, ml, ops.gemv_attn_out_bf16_(po, ml, wo, h.clone(), HQ, D)


@pytest.fixture(scope="module")
def refs(tiny, pools):
    """the 16-slot form with bits 11 and 12 off, once for every case"""
    lm = tiny.language_model
    try:
        _variant(lm, 0)
        out = {(layout, n): _run(pools, layout, n, 16) for layout in ("identity", "paged") for n in LENS + [1025]}
    finally:
        lm.apply_tuning()
    for (layout, n), (po, ml, y) in out.items():
        assert int(torch.isfinite(ml[0, 0, :, 0]).sum().item()) == min(16, (n + 63) // 64)
        assert bool(torch.isfinite(y.float()).all()) and not torch.equal(y, pools[5])
    return out


@pytest.mark.parametrize("layout", ["identity", "paged"])
def test_the_exact_count_gives_the_bytes_of_16_splits(tiny, pools, refs, layout):
    lm = tiny.language_model
    try:
        _variant(lm, CLASSES | EXACT)
        for n in LENS:
            po16, ml16, y16 = refs[layout, n]
            live = (n + 63) // 64
            for S in (live, live + 1):                # the count of the context; the count of a context one page longer
                if S > 16:
                    continue
                po, ml, y = _run(pools, layout, n, S, pitch=(S + 1) & ~1)
                assert ml.shape[2] == (S + 1) & ~1
                assert torch.equal(ml[0, :, :live], ml16[0, :, :live]), (n, S)
                assert torch.equal(po[0, :, :live], po16[0, :, :live]), (n, S)
                assert bool(torch.isinf(ml[0, :, live:S, 0]).all()), (n, S)
                assert torch.equal(y, y16), (n, S)
    finally:
        lm.apply_tuning()


@pytest.mark.parametrize("layout", ["identity", "paged"])
def test_at_1025_tokens_the_path_is_the_one_of_the_bit_off(tiny, pools, refs, layout):
    lm = tiny.language_model
    po16, ml16, y16 = refs[layout, 1025]
    try:
        _variant(lm, CLASSES | EXACT)
        po, ml, y = _run(pools, layout, 1025, 16)
        assert torch.equal(ml, ml16) and torch.equal(po, po16) and torch.equal(y, y16)
    finally:
        lm.apply_tuning()


def _generate(model, n_prompt, n=20):
    from mlx_vlm_amd.generate import generate_step

    ids = np.random.default_rng(21).integers(3, 1000, (1, n_prompt))
    out = [(t, lp.float().cpu()) for t, lp in generate_step(ids, model, None, None, max_tokens=n, temperature=0.0, lookahead=8)]
    assert len(out) == n
    return [t for t, _ in out], torch.stack([lp for _, lp in out])


def _counts_of(lm, run):
    """the split counts (flags bits 6 .. 10) of the steps `run` enqueues"""
    from mlx_vlm_amd import _lib

    seen, args_of = [], lm.decode_state(1).args.__func__

    def spy(st, *a, flags=0, **kw):
        seen.append((int(flags) & _lib.DECODE_NSPLITS_MASK) >> _lib.DECODE_NSPLITS_SHIFT)
        return args_of(st, *a, flags=flags, **kw)

    cls = type(lm.decode_state(1))
    cls.args = spy
    try:
        out = run()
    finally:
        cls.args = args_of
    return out, seen


@pytest.mark.parametrize("n_prompt", [500, 1012], ids=["512-513", "1024-1025"])
def test_generate_step_across_a_page_boundary_equals_the_run_with_the_bit_off(tiny, n_prompt):
    from mlx_vlm_amd import _lib

    lm = tiny.language_model
    n, n_layers = 20, 2
    try:
        _variant(lm, CLASSES)
        (toks0, lps0), seen = _counts_of(lm, lambda: _generate(tiny, n_prompt, n))
        assert set(seen) == {0}
        assert len(set(toks0)) == len(toks0)                       # (the peaked head walks a permutation: no accidental agreement)
        _variant(lm, CLASSES | EXACT)
        (toks, lps), seen = _counts_of(lm, lambda: _generate(tiny, n_prompt, n))
        # one step per call at ctx = n_prompt .. n_prompt + n - 2: the pages of ctx + 1, nothing beyond 1024 tokens
        pages = [(c + 1 + 63) // 64 for c in range(n_prompt, n_prompt + n - 1)]
        assert seen == [p if p <= 16 else 0 for p in pages], seen
        assert len(set(seen)) == 2
        assert toks == toks0 and torch.equal(lps, lps0)
        assert int(_lib.lib().vlm_llm_decode_launches(lm._handle)) == 5 * n_layers + 3
    finally:
        lm.apply_tuning()
