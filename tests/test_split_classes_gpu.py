"""Bit 11 of VLM_TUNE_GEMV_VARIANT and bits 4, 5 of vlm_decode_args.flags (include/vlm_hip.h): a one-row step at a short context
runs its page-split attention and the o_proj that merges it over 4 / 8 / 12 splits instead of 16, and the o_proj prologue
reads only that many (m, l, O) slots.  While 64 S >= ctx + 1 every split owns at most one page - as under 16 splits - and the
merge adds the live splits in the same order (the dead ones are exact zeros): the residual stream carries the BYTES of S = 16.

Operators: attention + o_proj of one row, G = 6 query heads per kv head, identity and paged layouts, at ctx + 1 on both sides of
every class boundary (1, 64 | 65, 256 | 257, 512 | 513, 768 | 769, 1024) - every class that holds the context against S = 16
with the bit off (the 16-slot prologue the parent ran).

Engine: generate_step on the tiny two-layer Qwen2-VL from a 250-token prompt for 20 tokens at lookahead 8 (the steps cross
ctx + 1 = 256, i.e. the class changes with steps of both classes in flight) yields the tokens and `torch.equal` log-probs of
the run with the bit off, in the same number of launches per step; under a window (max_kv_size) and with a temperature the
steps keep 16 splits, and stay equal as well."""
import numpy as np
import pytest
import torch

from oracle import qwen2_vl as oq
from tests.helpers import build_product_model

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
HKV, G, D, MAX_PAGES = 2, 6, 128, 16
HQ = HKV * G
LENS = [1, 64, 65, 256, 257, 512, 513, 768, 769, 1024]          # ctx + 1


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
    base = lm.TUNING_DEFAULTS["gemv_variant"] & ~2048
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


@pytest.mark.parametrize("layout", ["identity", "paged"])
def test_every_class_that_holds_the_context_gives_the_bytes_of_16_splits(tiny, pools, layout):
    from mlx_vlm_amd import ops

    lm = tiny.language_model
    kpool, vpool, table, q, wo, h = pools
    bt = table if layout == "paged" else None

    def run(n, S):
        kv_len = torch.tensor([n - 1], dtype=torch.int32, device="cuda")            # the step adds its own key
        po, ml = ops.attn_decode_paged_split(q, kpool, vpool, bt, kv_len, 1, HQ, HKV, D, D ** -0.5, S, merge=False, max_pages=MAX_PAGES)
        assert int(torch.isfinite(ml[0, 0, :, 0]).sum().item()) == min(S, (n + 63) // 64)
        return ops.gemv_attn_out_bf16_(po, ml, wo, h.clone(), HQ, D)

    try:
        for n in LENS:
            _variant(lm, 0)
            ref = run(n, 16)
            assert bool(torch.isfinite(ref.float()).all()) and not torch.equal(ref, h)
            _variant(lm, 2048)
            classes = [S for S in (4, 8, 12, 16) if 64 * S >= n]
            assert classes
            for S in classes:
                assert torch.equal(run(n, S), ref), (n, S)
    finally:
        lm.apply_tuning()


def _generate(model, n_prompt=250, n=20, temperature=0.0, **kw):
    from mlx_vlm_amd.generate import generate_step

    ids = np.random.default_rng(21).integers(3, 1000, (1, n_prompt))
    out = [(t, lp.float().cpu()) for t, lp in generate_step(ids, model, None, None, max_tokens=n, temperature=temperature, lookahead=8, **kw)]
    assert len(out) == n
    return [t for t, _ in out], torch.stack([lp for _, lp in out])


def _classes_of(lm, run):
    """the split classes (flags bits 4, 5) of the steps `run` enqueues"""
    from mlx_vlm_amd import _lib

    seen, args_of = [], lm.decode_state(1).args.__func__

    def spy(st, *a, flags=0, **kw):
        seen.append((int(flags) & _lib.DECODE_SPLITS_MASK) >> _lib.DECODE_SPLITS_SHIFT)
        return args_of(st, *a, flags=flags, **kw)

    cls = type(lm.decode_state(1))
    cls.args = spy
    try:
        out = run()
    finally:
        cls.args = args_of
    return out, seen


def test_generate_step_across_256_tokens_equals_the_run_with_the_bit_off(tiny):
    from mlx_vlm_amd import _lib

    lm = tiny.language_model
    n_layers = 2
    try:
        _variant(lm, 0)
        (toks0, lps0), seen = _classes_of(lm, lambda: _generate(tiny))
        assert set(seen) == {0}
        assert int(_lib.lib().vlm_llm_decode_launches(lm._handle)) == 5 * n_layers + 3
        assert len(set(toks0)) == len(toks0)                       # (the peaked head walks a permutation: no accidental agreement)
        _variant(lm, 2048)
        (toks, lps), seen = _classes_of(lm, lambda: _generate(tiny))
        # steps at ctx = 250 .. 268: ctx + 1 <= 256 takes 4 splits, the rest 8
        assert seen == [1] * 6 + [2] * 13, seen
        assert toks == toks0 and torch.equal(lps, lps0)
        assert int(_lib.lib().vlm_llm_decode_launches(lm._handle)) == 5 * n_layers + 3
    finally:
        lm.apply_tuning()


@pytest.mark.parametrize("kw", [dict(max_kv_size=300), dict(temperature=0.8, top_p=0.9, seed=7)], ids=["window", "sampled"])
def test_window_and_sampled_steps_keep_16_splits(tiny, kw):
    lm = tiny.language_model
    try:
        _variant(lm, 0)
        ref = _generate(tiny, **kw)
        _variant(lm, 2048)
        (toks, lps), seen = _classes_of(lm, lambda: _generate(tiny, **kw))
        assert set(seen) == {0}, seen
        assert toks == ref[0] and torch.equal(lps, ref[1])
    finally:
        lm.apply_tuning()
