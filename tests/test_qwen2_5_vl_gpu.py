"""The Qwen2.5-VL family on the GPU: the biased SwiGLU GEMM epilogue, the tower in its Qwen2.5 block form (window order on the
device, both attention routes) against the torch restatement (tests/qwen2_5_vl_ref.py, itself pinned to the reference and to
transformers by tests/test_qwen2_5_vl_cpu.py), and the family end to end: load() of a checkpoint directory, generate_step,
MLX 4-bit, BatchGenerator, a warm prefix-cache admission, and an old-form Qwen2-VL handle next to a new-form one."""
import os

import numpy as np
import pytest
import torch

from oracle import ops as O
from oracle import qwen2_vl as oq
from tests import qwen2_5_vl_ref as R
from tests.helpers import bf16_close, build_product_model, synth_request
from tests.test_engine_gpu import _tie_aware_equal

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
HERE = os.path.dirname(os.path.abspath(__file__))
GRIDS = [(1, 12, 20), (1, 8, 8), (1, 2, 2)]          # windows 64 64 32 32 32 16 | 64 (an exact multiple: padding windows) | 4
ROUTES = {"one_tile": "1", "general": "0"}


def _rel_rms_err(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30))


@pytest.fixture(scope="module")
def tiny():
    cfg = R.tiny_cfg()
    W = R.random_weights(cfg, seed=1234, dtype=BF, std=0.05, embed_std=0.2)
    return cfg, W, R.build_product_model(cfg, W, kv_pool_tokens=8192, max_seqs=16)


@pytest.fixture(scope="module")
def tower_ref(tiny):
    """the restatement's features for GRIDS, computed once"""
    cfg, W, _ = tiny
    _, pix, thw = R.synth_request(cfg, GRIDS, seed=3)
    return pix, thw, R.vision_tower(W, cfg, torch.from_numpy(pix).to(BF), thw)


# ---------------------------------------------------------------- GEMM epilogue
@pytest.mark.parametrize("M,N2,K", [(308, 384, 160), (77, 6912, 1280), (2048, 6912, 1280)])
def test_gemm_bias_swiglu(M, N2, K):
    """VLM_EPI_BIAS | VLM_EPI_SWIGLU on interleaved (gate, up) rows and biases vs swiglu(linear(x, wg, bg), linear(x, wu, bu)):
    3 bf16 ulps, the bar test_gemv_w4_norm_prologue_swiglu_and_head gives the same expression.  The first two shapes run the
    128-tile kernels (csrc/gemm_bf16.hip); 2048 rows are 8 x 27 = 216 tiles of 256 x 256, past the 120 from which the dispatcher
    takes the phased kernel of csrc/gemm256_bf16.hip (images from about 470 x 470 pixels up)"""
    from mlx_vlm_amd import ops

    I = N2 // 2
    g = torch.Generator().manual_seed(M + K)
    x = torch.randn(M, K, generator=g).to(BF)
    wg, wu = (torch.randn(I, K, generator=g) * 0.05).to(BF), (torch.randn(I, K, generator=g) * 0.05).to(BF)
    bg, bu = (torch.randn(I, generator=g) * 0.5).to(BF), (torch.randn(I, generator=g) * 0.5).to(BF)
    ref = O.swiglu(O.linear(x, wg, bg), O.linear(x, wu, bu))
    wgu = torch.stack([wg, wu], dim=1).reshape(N2, K).contiguous().cuda()
    bgu = torch.stack([bg, bu], dim=1).reshape(N2).contiguous().cuda()
    out = ops.gemm(x.cuda(), wgu, bias=bgu, epilogue=ops.EPI_BIAS | ops.EPI_SWIGLU)
    assert out.shape == (M, I)
    ok, rep = bf16_close(out, ref, ulps=3)
    print(f"GEMM BIAS|SWIGLU {M}x{N2}x{K}: {rep}")
    assert ok, rep
    if M >= 2048:
        # both kernel families by name on this shape: staging mode 3 = the 256 x 256 kernel whenever legal, 2 = never
        try:
            for mode in (3, 2):
                ops.gemm_set_staging(mode)
                ok, rep = bf16_close(ops.gemm(x.cuda(), wgu, bias=bgu, epilogue=ops.EPI_BIAS | ops.EPI_SWIGLU), ref, ulps=3)
                assert ok, (mode, rep)
        finally:
            ops.gemm_set_staging(0)
    # the bias is really added (before the activation): without it the result is far away
    assert _rel_rms_err(ops.gemm(x.cuda(), wgu, epilogue=ops.EPI_SWIGLU), ref) > 0.1


# ---------------------------------------------------------------- tower
@pytest.mark.parametrize("route", list(ROUTES))
def test_tower_vs_restatement(tiny, tower_ref, route, monkeypatch):
    """three images in one call, window blocks on the one-tile kernel and on the general kernel: relative rms < 2e-2, the bar of
    test_vision_tower_vs_oracle for two blocks + merger"""
    cfg, W, model = tiny
    pix, thw, ref = tower_ref
    monkeypatch.setenv("VLM_VIT_WINDOW_ATTN", ROUTES[route])
    assert model.vision_tower.one_tile(64) == (route == "one_tile")
    out = model.vision_tower(torch.from_numpy(pix), thw)
    assert out.shape == ref.shape == (sum(t * h * w for t, h, w in GRIDS) // 4, cfg.vision.out_hidden_size)
    e = _rel_rms_err(out, ref)
    print(f"tower {route}: rel-rms {e:.4f}")
    assert e < 2e-2, e
    # every image separately gives the rows it has in the joint call (the window order never crosses images)
    r0 = 0
    for g in GRIDS:
        n = g[0] * g[1] * g[2]
        single = model.vision_tower(torch.from_numpy(pix[r0:r0 + n]), np.array([g]))
        assert _rel_rms_err(single, ref[r0 // 4:(r0 + n) // 4]) < 2e-2, g
        r0 += n


def test_tower_routes_agree_and_permutation_matters(tiny, tower_ref, monkeypatch):
    cfg, W, model = tiny
    pix, thw, ref = tower_ref
    outs = {}
    for route, v in ROUTES.items():
        monkeypatch.setenv("VLM_VIT_WINDOW_ATTN", v)
        outs[route] = model.vision_tower(torch.from_numpy(pix), thw).float().cpu()
    assert _rel_rms_err(outs["one_tile"], outs["general"]) < 1e-2
    # not vacuous: the features in window order (no reverse gather) are far from the reference
    from mlx_vlm_amd.models.qwen2_5_vl.vision import host_tables

    wi = host_tables(thw, 112, 2, 14)["window_index"]
    assert _rel_rms_err(outs["general"][torch.from_numpy(wi)], ref) > 0.3


@pytest.mark.parametrize("case", ["one_image", "three_images"])
def test_fp32_weight_model_vs_hf_golden(case):
    """HF fp32 features vs the HIP bf16 path on the same fp32 checkpoint: < 3e-2"""
    G = np.load(os.path.join(HERE, "golden", "qwen2_5_vl_tiny_hf.npz"))
    cfg = R.tiny_cfg()
    W32 = R.random_weights(cfg, seed=1234, dtype=torch.float32, std=0.05, embed_std=0.2)
    model = R.build_product_model(cfg, W32, kv_pool_tokens=2048, max_seqs=4)
    grids = [tuple(g) for g in G[case + ".grids"].tolist()]
    _, pix, thw = R.synth_request(cfg, grids, seed=len(grids))
    e = _rel_rms_err(model.vision_tower(torch.from_numpy(pix), thw), torch.from_numpy(G[case + ".hf_image_features"]))
    assert e < 3e-2, e


def test_tower_at_real_widths(monkeypatch):
    """1280 / 16 heads / 3420 / out 2048 at two blocks (block 0 windowed, block 1 full): the only place the 3420 -> 3456 padding
    runs on the device"""
    cfg = R.real_width_cfg()
    W = R.random_weights(cfg, seed=77, dtype=BF, std=0.02, tower_only=True)
    from mlx_vlm_amd.models.qwen2_5_vl import VisionConfig, VisionModel

    vm = VisionModel(VisionConfig.from_dict(R.model_config_dict(cfg)["vision_config"]))
    vm.load_weights({k[len("vision_tower."):]: v for k, v in W.items()})
    assert vm.mlp_hidden == 3456
    _, pix, thw = R.synth_request(cfg, GRIDS, seed=5)
    ref = R.vision_tower(W, cfg, torch.from_numpy(pix).to(BF), thw)
    for route, v in ROUTES.items():
        monkeypatch.setenv("VLM_VIT_WINDOW_ATTN", v)
        out = vm(torch.from_numpy(pix), thw)
        e = _rel_rms_err(out, ref)
        print(f"real widths {route}: rel-rms {e:.4f}")
        assert out.shape == (308 // 4, 2048) and e < 2e-2, (route, e)


# ---------------------------------------------------------------- end to end
def _quantized(seed):
    from oracle import quant as Q

    cfg = R.tiny_cfg()
    W = R.random_weights(cfg, seed=seed, dtype=BF, std=0.05, embed_std=0.2)
    ck, ow = Q.quantize_checkpoint(W, predicate=lambda p, v: p.startswith("language_model."))
    return cfg, {k: (v.view(torch.uint32) if v.dtype == torch.int32 else v) for k, v in ck.items()}, ow


@pytest.mark.parametrize("w4", [False, True])
def test_load_checkpoint_directory_and_generate(tmp_path, w4):
    """config.json with "model_type": "qwen2_5_vl" + safetensors under the HF names + a tokenizer -> load() -> 12 greedy tokens
    of generate_step against the restatement (tie-aware, 3e-2; first-step log-probs at 2 ulps + 3e-2 rms); w4: the language
    model in MLX 4-bit, the tower left bf16"""
    from mlx_vlm_amd import load
    from mlx_vlm_amd.generate import generate_step

    if w4:
        cfg, ck, ow = _quantized(4321)
        R.write_checkpoint(tmp_path, cfg, ck, quantization={"group_size": 64, "bits": 4})
    else:
        cfg = R.tiny_cfg()
        ow = ck = R.random_weights(cfg, seed=4321, dtype=BF, std=0.05, embed_std=0.2)
        R.write_checkpoint(tmp_path, cfg, ck)
    model, processor = load(str(tmp_path), kv_pool_tokens=4096, max_seqs=4)
    assert type(model).__module__.endswith("qwen2_5_vl.qwen2_5_vl") and model.language_model.quantized == w4
    assert type(processor).__name__ == "Qwen2_5_VLProcessor"
    ids, pix, thw = R.synth_request(cfg, [(1, 12, 20), (1, 8, 8)], n_text=11, seed=46)
    n_new = 12
    ref_toks, ref_logits = R.generate_greedy(ow, cfg, ids, torch.from_numpy(pix).to(BF), thw, max_tokens=n_new, return_logits=True)
    toks, lps = [], []
    for t, lp in generate_step(ids, model, torch.from_numpy(pix), None, max_tokens=n_new, temperature=0.0, image_grid_thw=thw):
        toks.append(t)
        lps.append(lp.float().cpu())
    assert len(toks) == n_new
    ok, n, margin = _tie_aware_equal(toks, ref_toks, ref_logits, tol=3e-2)
    assert ok, (toks, ref_toks, n, margin)
    ok, rep = bf16_close(lps[0], O.logprobs_from_logits(ref_logits[0][None])[0], ulps=2, atol_rms=3e-2)
    assert ok, rep
    if not w4:
        # the user API over the processor: image -> smart resize -> patches -> placeholder expansion -> same family path
        from mlx_vlm_amd import generate

        img = np.random.default_rng(3).integers(0, 256, (100, 150, 3), dtype=np.uint8)
        words = " ".join(f"t{int(i)}" for i in np.random.default_rng(4).integers(3, 1000, 9))
        out = generate(model, processor, f"<|vision_start|> <|image_pad|> <|vision_end|> {words}", image=img, max_tokens=6,
                       temperature=0.0)
        assert out.prompt_tokens == 2 + 9 + (112 // 14) * (140 // 14) // 4 and out.generation_tokens >= 1


def test_generate_step_options_of_the_shared_language_model(tiny):
    """prompt_cache, kv_bits=8 and max_kv_size live in the shared language model: they run for this family and stay close to the
    plain run's first log-probs"""
    from mlx_vlm_amd.generate import generate_step

    cfg, W, model = tiny
    ids, pix, thw = R.synth_request(cfg, [(1, 8, 8)], n_text=9, seed=21)
    run = lambda **kw: [(t, lp.float().cpu()) for t, lp in generate_step(ids, model, torch.from_numpy(pix), None, max_tokens=5,   # noqa: E731
                                                                        temperature=0.0, image_grid_thw=thw, **kw)]
    plain = run()
    cache = model.language_model.make_cache()
    cached = run(prompt_cache=cache)
    assert [t for t, _ in cached] == [t for t, _ in plain] and cache[0].offset >= ids.shape[1]
    cache[0]._seq.release()
    q8 = run(kv_bits=8)
    ok, rep = bf16_close(q8[0][1], plain[0][1], ulps=2, atol_rms=3e-2)
    assert ok and len(q8) == 5, rep
    win = run(max_kv_size=64)
    assert len(win) == 5 and win[0][0] == plain[0][0]


def test_batch_generator_equals_single_requests(tiny):
    """three requests of different sizes - an exact-multiple grid, a ragged one, text only - through the BatchGenerator: every
    request's tokens are the ones it produces alone, under the end-to-end test's tie-aware rule (_tie_aware_equal, 3e-2 of the
    restatement's logit rms): while the single run follows the restatement its logits are the judge of a divergence between the
    batch run and the single run; the single run and the batch run are each held to the restatement by the same rule"""
    from mlx_vlm_amd.batch import BatchGenerator
    from tests.test_engine_gpu import _insert_all, _single_runs

    cfg, W, model = tiny
    reqs = [R.synth_request(cfg, [(1, 8, 8)], n_text=7, seed=61), R.synth_request(cfg, [(1, 12, 20)], n_text=10, seed=62),
            R.synth_request(cfg, [], n_text=15, seed=63)]
    max_tokens = [7, 5, 8]
    singles = _single_runs(model, reqs, max_tokens)
    gen = BatchGenerator(model, None, max_tokens=8, completion_batch_size=4, prefill_batch_size=2)
    uids = _insert_all(gen, reqs, max_tokens)
    got = {u: [] for u in uids}
    while gen.has_work:
        _, out = gen.next()
        for r in out:
            got[r.uid].append((r.token, r.token_logprob))
    gen.close()
    for (ids, pix, thw), m, u, single in zip(reqs, max_tokens, uids, singles):
        ref_toks, ref_logits = R.generate_greedy(W, cfg, ids, torch.from_numpy(pix).to(BF) if pix is not None else None, thw,
                                                 max_tokens=m, return_logits=True)
        batch, alone = [t for t, _ in got[u]], [t for t, _ in single]
        assert len(batch) == len(alone) == m
        for name, toks in (("single", alone), ("batch", batch)):
            ok, n, margin = _tie_aware_equal(toks, ref_toks, ref_logits, tol=3e-2)
            assert ok, (name, u, toks, ref_toks, n, margin)
        # batch against single: the restatement's logits describe a step as long as the single run has followed its tokens up to
        # that step (the first step at which it leaves them included)
        valid = next((i for i, (a, b) in enumerate(zip(alone, ref_toks)) if a != b), m - 1) + 1
        ok, n, margin = _tie_aware_equal(batch[:valid], alone[:valid], ref_logits, tol=3e-2)
        assert ok, (u, batch, alone, n, margin)


def test_warm_prefix_cache_admission(tiny):
    """BatchGenerator(apc_manager=) accepts the family (it shares the language-model class): a request whose first 128 tokens
    and image equal an earlier one's is admitted warm - the tower is not called - and decodes what it decodes cold"""
    from mlx_vlm_amd.apc import APCManager
    from mlx_vlm_amd.batch import BatchGenerator
    from tests.test_apc_gpu import CountingTower

    cfg, W, model = tiny
    a_ids, pix, thw = R.synth_request(cfg, [(1, 8, 8)], n_text=140, seed=31)
    a_ids = a_ids.reshape(-1)
    b_ids = np.concatenate([a_ids[:128], np.random.default_rng(5).integers(3, 1000, 21)])
    kw = dict(pixel_values=torch.from_numpy(pix), image_grid_thw=thw)
    tower = model.vision_tower
    model.vision_tower = counting = CountingTower(tower)

    def run(gen, ids):
        (u,) = gen.insert([ids], 6, prompt_kwargs=[kw])
        toks = []
        while gen.has_work:
            _, out = gen.next()
            toks += [r.token for r in out if r.uid == u]
        return toks

    try:
        mgr = APCManager(num_blocks=8)
        gen = BatchGenerator(model, None, max_tokens=6, completion_batch_size=4, apc_manager=mgr)
        run(gen, a_ids)
        calls = counting.calls
        warm = run(gen, b_ids)
        snap = mgr.stats_snapshot()
        assert snap["lookups_hit"] == 1 and snap["matched_tokens"] == 128 and counting.calls == calls
        gen.close()
        mgr.close()
        plain = BatchGenerator(model, None, max_tokens=6, completion_batch_size=4)
        cold = run(plain, b_ids)
        plain.close()
        assert counting.calls == calls + 1
    finally:
        model.vision_tower = tower
    ref_toks, ref_logits = R.generate_greedy(W, cfg, b_ids[None], torch.from_numpy(pix).to(BF), thw, max_tokens=6, return_logits=True)
    for toks in (warm, cold):
        ok, n, margin = _tie_aware_equal(toks, ref_toks, ref_logits, tol=3e-2)
        assert ok and len(toks) == 6, (toks, ref_toks, n, margin)


def test_old_form_handle_is_untouched_by_a_new_form_one(tiny, tower_ref):
    """a Qwen2-VL tower (first form of vlm_vit_forward) gives bit-identical features for test_vision_tower_vs_oracle's inputs before
    and after a Qwen2.5 tower has run in the same process"""
    cfg2 = oq.tiny_cfg()
    W2 = oq.random_weights(cfg2, seed=1234, dtype=BF, std=0.05, embed_std=0.2)
    old = build_product_model(cfg2, W2, kv_pool_tokens=2048, max_seqs=4)
    _, pix2, thw2 = synth_request(cfg2, [(56, 84), (112, 56)], seed=3)
    before = old.vision_tower(torch.from_numpy(pix2), thw2).clone()
    assert _rel_rms_err(before, oq.vision_tower(W2, cfg2, torch.from_numpy(pix2).to(BF), thw2)) < 2e-2
    _, _, model = tiny
    pix, thw, ref = tower_ref
    assert _rel_rms_err(model.vision_tower(torch.from_numpy(pix), thw), ref) < 2e-2
    after = old.vision_tower(torch.from_numpy(pix2), thw2)
    assert torch.equal(before, after)
