"""The Qwen3-VL family on the GPU against the torch restatement (tests/qwen3_vl_ref.py, itself pinned bit for bit to the reference
and at 1e-4 to transformers by tests/test_qwen3_vl_cpu.py): the tower in its Qwen3 block form with its DeepStack taps, and the
family end to end on the tiny model (4 decoder layers, 2 taps) - prefill with DeepStack, greedy and teacher-forced decode on
the two-launch qkv step, captured against eager steps, the batch generator with a wide step, chunked prefill across an image's
rows, the shared language model's options, MLX 4-bit weights, load() of a checkpoint directory."""
import numpy as np
import pytest
import torch

from oracle import ops as O
from tests import qwen3_vl_ref as R
from tests.helpers import bf16_close
from tests.test_engine_gpu import _insert_all, _tie_aware_equal

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
GRIDS = [(1, 4, 6), (1, 8, 8), (1, 2, 2)]


def _rel_rms_err(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30))


def _pix(pix):
    return torch.from_numpy(pix) if pix is not None else None


@pytest.fixture(scope="module")
def tiny():
    cfg = R.tiny_cfg()
    W = R.random_weights(cfg, seed=1234, dtype=BF, std=0.05, embed_std=0.2)
    return cfg, W, R.build_product_model(cfg, W, kv_pool_tokens=8192, max_seqs=48)


@pytest.fixture(scope="module")
def image_prompt(tiny):
    """one prompt over two images with the restatement's prefill logits, 8 greedy tokens and their logits - computed once"""
    cfg, W, _ = tiny
    ids, pix, thw = R.synth_request(cfg, [(1, 8, 8), (1, 4, 6)], n_text=13, seed=11)
    logits, f = R.prefill_logits(W, cfg, ids, _pix(pix).to(BF), thw, return_features=True)
    toks, step_logits = R.generate_greedy(W, cfg, ids, _pix(pix).to(BF), thw, max_tokens=8, return_logits=True)
    return ids, pix, thw, logits, f, toks, step_logits


# ---------------------------------------------------------------- tower
@pytest.mark.parametrize("grids", [[(1, 4, 6)], [(1, 8, 8)], GRIDS], ids=["g4x6", "g8x8", "three"])
def test_tower_and_taps_vs_restatement(tiny, grids):
    """main output and every DeepStack tap: relative rms < 2e-2, the bar of the Qwen2.5-VL tower test for blocks + merger"""
    cfg, W, model = tiny
    _, pix, thw = R.synth_request(cfg, grids, seed=3)
    ref, ref_taps = R.vision_tower(W, cfg, _pix(pix).to(BF), thw)
    out, taps = model.vision_tower(_pix(pix), thw)
    n = sum(t * h * w for t, h, w in grids) // 4
    assert out.shape == ref.shape == (n, cfg.vision.out_hidden_size) and len(taps) == len(ref_taps) == 2
    errs = [_rel_rms_err(out, ref)] + [_rel_rms_err(t, r) for t, r in zip(taps, ref_taps)]
    print(f"tower {grids}: rel-rms main {errs[0]:.4f} taps {errs[1]:.4f} {errs[2]:.4f}")
    assert max(errs) < 2e-2, errs
    # the taps are three different things: the main merger's output is none of them, and they are not each other
    assert _rel_rms_err(taps[0], ref) > 0.3 and _rel_rms_err(taps[0], ref_taps[1]) > 0.3
    if len(grids) > 1:
        # every image separately gives the rows it has in the joint call (position rows and attention never cross images)
        r0 = 0
        for g in grids:
            m = g[0] * g[1] * g[2]
            single, staps = model.vision_tower(_pix(pix[r0:r0 + m]), np.array([g]))
            assert _rel_rms_err(single, ref[r0 // 4:(r0 + m) // 4]) < 2e-2, g
            assert _rel_rms_err(staps[1], ref_taps[1][r0 // 4:(r0 + m) // 4]) < 2e-2, g
            r0 += m


def test_fp32_weight_model_vs_hf_golden():
    """HF fp32 features and taps vs the HIP bf16 path on the same fp32 checkpoint: < 3e-2"""
    import os

    H = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qwen3_vl_tiny_hf.npz"))
    cfg = R.tiny_cfg()
    W32 = R.random_weights(cfg, seed=1234, dtype=torch.float32, std=0.05, embed_std=0.2)
    model = R.build_product_model(cfg, W32, kv_pool_tokens=2048, max_seqs=4)
    for case in ("one_image", "three_images"):
        grids = [tuple(g) for g in H[case + ".grids"].tolist()]
        _, pix, thw = R.synth_request(cfg, grids, seed=len(grids))
        out, taps = model.vision_tower(_pix(pix), thw)
        assert _rel_rms_err(out, torch.from_numpy(H[case + ".hf_image_features"])) < 3e-2
        for j, t in enumerate(taps):
            assert _rel_rms_err(t, torch.from_numpy(H[case + f".hf_tap{j}"])) < 3e-2, (case, j)


# ---------------------------------------------------------------- end to end
def test_prefill_logits_and_greedy_vs_restatement(tiny, image_prompt):
    """every prompt row's logits (DeepStack behind the first two decoder layers) at 2e-2 rel-rms per row, then 8 greedy tokens
    under the tie-aware rule"""
    from mlx_vlm_amd.generate import generate_step

    cfg, W, model = tiny
    ids, pix, thw, ref_logits, ref_f, ref_toks, ref_steps = image_prompt
    lm = model.language_model
    f = model.get_input_embeddings(ids, _pix(pix), image_grid_thw=thw)
    assert f.deepstack_visual_embeds.shape == (2, int(ref_f.visual_pos_masks.sum()), cfg.text.hidden_size)
    assert np.array_equal(f.visual_pos_masks, ref_f.visual_pos_masks) and np.array_equal(np.asarray(f.position_ids), ref_f.position_ids)
    cache = lm.make_cache()
    out = lm(ids, f.inputs_embeds, cache=cache, position_ids=f.position_ids, visual_pos_masks=f.visual_pos_masks,
             deepstack_visual_embeds=f.deepstack_visual_embeds)
    cache[0]._seq.release()
    assert out.logits.shape == (1, ids.shape[1], cfg.text.vocab_size)
    worst = max(_rel_rms_err(out.logits[0, i], ref_logits[i]) for i in range(ids.shape[1]))
    print(f"prefill logits: worst row rel-rms {worst:.4f}")
    assert worst < 2e-2, worst
    # without the DeepStack inputs the same call is far away at the rows behind the image (the engine really adds them)
    cache = lm.make_cache()
    bare = lm(ids, f.inputs_embeds, cache=cache, position_ids=f.position_ids)
    cache[0]._seq.release()
    assert _rel_rms_err(bare.logits[0, -1], ref_logits[-1]) > 0.05
    toks = [t for t, _ in generate_step(ids, model, _pix(pix), None, max_tokens=8, temperature=0.0, image_grid_thw=thw)]
    ok, n, margin = _tie_aware_equal(toks, ref_toks, ref_steps, tol=3e-2)
    assert ok and len(toks) == 8, (toks, ref_toks, n, margin)


@pytest.mark.parametrize("grids", [[(1, 4, 6)], []], ids=["image", "text"])
def test_teacher_forced_decode_40_steps(tiny, grids):
    """40 forced tokens through the module call (vlm_llm_decode_forward: projection, then the QK-norm rotary launch, per layer):
    every step's logits at 2e-2 rel-rms against the restatement"""
    cfg, W, model = tiny
    lm = model.language_model
    ids, pix, thw = R.synth_request(cfg, grids, n_text=14, seed=44)
    forced = np.random.default_rng(45).integers(3, 1000, 40)
    ref = R.decode_teacher_forced(W, cfg, ids, _pix(pix).to(BF) if pix is not None else None, thw, forced)
    cache = lm.make_cache()
    out = model(ids, _pix(pix), cache=cache, logits_to_keep=1, **({"image_grid_thw": thw} if grids else {}))
    rows = [out.logits[0, -1].clone()]
    for y in forced:
        rows.append(lm(np.array([[int(y)]]), cache=cache).logits[0, -1].clone())
    cache[0]._seq.release()
    got = torch.stack(rows)
    worst = max(_rel_rms_err(got[i], ref[i]) for i in range(ref.shape[0]))
    print(f"teacher-forced {len(forced)} steps ({'image' if grids else 'text'}): worst row rel-rms {worst:.4f}")
    assert got.shape == ref.shape and worst < 2e-2, worst


@pytest.mark.parametrize("B", [1, 4])
def test_captured_step_equals_eager_step(tiny, B):
    """the captured decode step (hipGraph replay) and the eager step enqueue the same launches: tokens and every step's
    log-probs bit for bit"""
    from mlx_vlm_amd.generate import batch_generate_ids, generate_step

    cfg, W, model = tiny
    if B == 1:
        ids, pix, thw = R.synth_request(cfg, [(1, 4, 6)], n_text=9, seed=71)

        def run(use_graph):
            out = [(t, lp.clone()) for t, lp in generate_step(ids, model, _pix(pix), None, max_tokens=20, temperature=0.0,
                                                             image_grid_thw=thw, use_graph=use_graph)]
            return [t for t, _ in out], torch.stack([lp for _, lp in out])

        (ta, la), (tb, lb) = run(True), run(False)
        assert ta == tb and torch.equal(la, lb)
    else:
        reqs = [R.synth_request(cfg, [(1, 2, 2)] if i % 2 else [], n_text=6 + i, seed=80 + i) for i in range(B)]
        args = ([r[0].reshape(-1) for r in reqs], [_pix(r[1]) for r in reqs], [r[2] for r in reqs])
        a, _ = batch_generate_ids(model, *args, max_tokens=12, use_graph=True)
        b, _ = batch_generate_ids(model, *args, max_tokens=12, use_graph=False)
        assert a == b


def test_batch_generator_equals_single_requests(tiny):
    """5 mixed requests (three with images, two text only) through the BatchGenerator - their DeepStack rows concatenated into
    one prefill - against the same requests alone, under the rule of the 4-bit batch test: every compared step's log-prob
    within 2 ulps of the step's log-prob span, tokens equal up to the first tie, at least 80 % of all tokens equal"""
    from mlx_vlm_amd.batch import BatchGenerator
    from mlx_vlm_amd.generate import generate_step

    cfg, W, model = tiny
    reqs = [R.synth_request(cfg, [(1, 4, 6)], n_text=7, seed=61), R.synth_request(cfg, [], n_text=15, seed=62),
            R.synth_request(cfg, [(1, 8, 8), (1, 2, 2)], n_text=5, seed=63), R.synth_request(cfg, [], n_text=9, seed=64),
            R.synth_request(cfg, [(1, 2, 2)], n_text=11, seed=65)]
    max_tokens = [7, 5, 8, 6, 8]
    singles = []
    for (ids, pix, thw), m in zip(reqs, max_tokens):
        kw = dict(image_grid_thw=thw) if thw is not None else {}
        singles.append([(t, float(lp[t]), float(lp.float().abs().max())) for t, lp in
                        generate_step(ids, model, _pix(pix), None, max_tokens=m, **kw)])
    gen = BatchGenerator(model, None, max_tokens=8, completion_batch_size=8, prefill_batch_size=4)
    uids = _insert_all(gen, reqs, max_tokens)
    got = {u: [] for u in uids}
    while gen.has_work:
        _, out = gen.next()
        for r in out:
            got[r.uid].append((r.token, r.token_logprob))
    gen.close()
    n_equal = 0
    for u, single, m in zip(uids, singles, max_tokens):
        assert len(got[u]) == len(single) == m
        for i, ((ta, la), (tb, lb, span)) in enumerate(zip(got[u], single)):
            assert abs(la - lb) <= 2 * 2 ** -7 * span, (u, i, span, got[u], single)
            if ta != tb:
                break
            n_equal += 1
    assert n_equal >= 0.8 * sum(max_tokens), (n_equal, sum(max_tokens))
    # each single run is the restatement's, tie-aware (so the batch is held to it too, through the rule above)
    for (ids, pix, thw), m, single in zip(reqs[:3], max_tokens, singles):
        ref_toks, ref_logits = R.generate_greedy(W, cfg, ids, _pix(pix).to(BF) if pix is not None else None, thw, max_tokens=m,
                                                 return_logits=True)
        ok, n, margin = _tie_aware_equal([t for t, _, _ in single], ref_toks, ref_logits, tol=3e-2)
        assert ok, (ref_toks, single, n, margin)


def test_wide_step_of_17_rows_equals_single_rows(tiny):
    """17 sequences in one decode step - a WIDE step: the projection on the prefill GEMMs, then the QK-norm rotary launch over 17
    rows through the block table - against each sequence stepping alone: 2e-2 rel-rms per row"""
    cfg, W, model = tiny
    lm = model.language_model
    B = 17
    rng = np.random.default_rng(90)
    prompts = [rng.integers(3, 1000, 5 + (3 * i) % 11) for i in range(B)]
    feed = rng.integers(3, 1000, B)

    def prefilled(idx):
        caches = lm.make_cache_batch(len(idx))
        emb = torch.cat([lm.embed_tokens(prompts[i][None])[0] for i in idx])
        pos = np.concatenate([np.broadcast_to(np.arange(len(prompts[i]))[None], (3, len(prompts[i]))) for i in idx], axis=1)
        lm.prefill(emb, pos, caches, [len(prompts[i]) for i in idx], "last", reserve_extra=4)
        return caches

    lm._rope_deltas = None
    caches = prefilled(list(range(B)))
    wide = lm(feed.reshape(B, 1), cache=caches).logits[:, 0].clone()
    for c in caches:
        c[0]._seq.release()
    worst = 0.0
    for i in range(B):
        (c,) = prefilled([i])
        alone = lm(feed[i].reshape(1, 1), cache=c).logits[0, 0]
        c[0]._seq.release()
        worst = max(worst, _rel_rms_err(wide[i], alone))
    print(f"17-row wide step: worst row rel-rms vs single rows {worst:.4f}")
    assert worst < 2e-2, worst
    ref = R.decode_teacher_forced(W, cfg, prompts[3][None], None, None, [int(feed[3])])
    assert _rel_rms_err(wide[3], ref[1]) < 2e-2


@pytest.mark.parametrize("step", [7, 16])
def test_chunked_prefill_slices_the_deepstack_rows(tiny, image_prompt, step):
    """prefill_step_size small enough to cut an image's rows across chunks: the chunks' DeepStack embeds are cut with them
    (reference language.py:528-558), so the first token's log-probs are the one-shot run's (2 ulps + 3e-2 of the rms: the
    chunk path attends through other kernels) and the greedy tokens the restatement's"""
    from mlx_vlm_amd.generate import generate_step

    cfg, W, model = tiny
    ids, pix, thw, ref_logits, ref_f, ref_toks, ref_steps = image_prompt
    cols = np.nonzero(ref_f.visual_pos_masks[0])[0]
    assert any(cols[0] < b <= cols[-1] for b in range(step, ids.shape[1], step))          # a chunk border inside the image rows
    run = lambda **kw: [(t, lp.float().cpu()) for t, lp in generate_step(ids, model, _pix(pix), None, max_tokens=8,   # noqa: E731
                                                                        temperature=0.0, image_grid_thw=thw, **kw)]
    plain, chunked = run(), run(prefill_step_size=step)
    ok, rep = bf16_close(chunked[0][1], plain[0][1], ulps=2, atol_rms=3e-2)
    assert ok, rep
    ok, rep = bf16_close(chunked[0][1], O.logprobs_from_logits(ref_steps[0][None])[0], ulps=2, atol_rms=3e-2)
    assert ok, rep
    ok, n, margin = _tie_aware_equal([t for t, _ in chunked], ref_toks, ref_steps, tol=3e-2)
    assert ok, (chunked, ref_toks, n, margin)
    # the module call in two pieces, full-prompt mask and embeds handed to both (the call cuts them): last-row logits 3e-2 of the
    # one-shot restatement; the same two calls WITHOUT DeepStack are far away
    lm = model.language_model
    f = model.get_input_embeddings(ids, _pix(pix), image_grid_thw=thw)
    cut = int(cols[len(cols) // 2])

    def two_calls(**ds):
        cache = lm.make_cache()
        lm(ids[:, :cut], f.inputs_embeds[:, :cut], cache=cache, position_ids=f.position_ids, logits_to_keep=1, **ds)
        out = lm(ids[:, cut:], f.inputs_embeds[:, cut:], cache=cache, position_ids=f.position_ids, logits_to_keep=1, **ds)
        cache[0]._seq.release()
        return out.logits[0, -1]

    with_ds = two_calls(visual_pos_masks=f.visual_pos_masks, deepstack_visual_embeds=f.deepstack_visual_embeds)
    assert _rel_rms_err(with_ds, ref_logits[-1]) < 3e-2
    assert _rel_rms_err(two_calls(), ref_logits[-1]) > 0.05


def test_generate_step_options_of_the_shared_language_model(tiny):
    """prompt_cache, kv_bits=8 and max_kv_size live in the shared language model and only see slot / pos / pools: they run for
    this family and stay close to the plain run's first log-probs"""
    from mlx_vlm_amd.generate import generate_step

    cfg, W, model = tiny
    ids, pix, thw = R.synth_request(cfg, [(1, 8, 8)], n_text=9, seed=21)
    run = lambda **kw: [(t, lp.float().cpu()) for t, lp in generate_step(ids, model, _pix(pix), None, max_tokens=5,   # noqa: E731
                                                                        temperature=0.0, image_grid_thw=thw, **kw)]
    plain = run()
    cache = model.language_model.make_cache()
    cached = run(prompt_cache=cache)
    assert [t for t, _ in cached] == [t for t, _ in plain] and cache[0].offset >= ids.shape[1]
    cache[0]._seq.release()
    q8 = run(kv_bits=8, quantized_kv_start=0)
    ok, rep = bf16_close(q8[0][1], plain[0][1], ulps=2, atol_rms=3e-2)
    assert ok and len(q8) == 5, rep
    ok, rep = bf16_close(q8[1][1], plain[1][1], ulps=2, atol_rms=8e-2)          # a step that attended over the 8-bit pools
    assert ok, rep
    win = run(max_kv_size=64)
    assert len(win) == 5 and win[0][0] == plain[0][0]
    # a sampled run inside the captured step (the row-independent sampler tail) and top-p: runs, deterministic under a seed
    s1 = [t for t, _ in generate_step(ids, model, _pix(pix), None, max_tokens=5, temperature=0.8, top_p=0.9, seed=5, image_grid_thw=thw)]
    s2 = [t for t, _ in generate_step(ids, model, _pix(pix), None, max_tokens=5, temperature=0.8, top_p=0.9, seed=5, image_grid_thw=thw)]
    assert s1 == s2 and len(s1) == 5


def _quantized(seed):
    from oracle import quant as Q

    cfg = R.tiny_cfg()
    W = R.random_weights(cfg, seed=seed, dtype=BF, std=0.05, embed_std=0.2)
    ck, ow = Q.quantize_checkpoint(W, predicate=lambda p, v: p.startswith("language_model."))
    return cfg, {k: (v.view(torch.uint32) if v.dtype == torch.int32 else v) for k, v in ck.items()}, ow


def test_quantized_4bit_teacher_forced_decode_vs_restatement():
    """the language model in MLX 4-bit (embedding, every Linear, the tied head; the q / k norms stay bf16), the tower bf16: every
    teacher-forced step's logits against the restatement on the SAME quantized weights at the 4-bit bar of
    test_quantized_4bit_teacher_forced_decode_vs_oracle: 2e-2 rel-rms per row, 4 ulps + 8e-2 of the rms element-wise"""
    cfg, ck, ow = _quantized(1234)
    model = R.build_product_model(cfg, ck, kv_pool_tokens=4096, max_seqs=4)
    lm = model.language_model
    assert lm.quantized
    ids, pix, thw = R.synth_request(cfg, [(1, 4, 6)], n_text=14, seed=44)
    forced = np.random.default_rng(45).integers(3, 1000, 30)
    ref = R.decode_teacher_forced(ow, cfg, ids, _pix(pix).to(BF), thw, forced)
    cache = lm.make_cache()
    out = model(ids, _pix(pix), cache=cache, image_grid_thw=thw, logits_to_keep=1)
    rows = [out.logits[0, -1].clone()]
    for y in forced:
        rows.append(lm(np.array([[int(y)]]), cache=cache).logits[0, -1].clone())
    cache[0]._seq.release()
    got = torch.stack(rows)
    worst = max(_rel_rms_err(got[i], ref[i]) for i in range(ref.shape[0]))
    print(f"4-bit teacher-forced: worst row rel-rms {worst:.4f}")
    assert worst < 2e-2, worst
    ok, rep = bf16_close(got, ref, ulps=4, atol_rms=8e-2)
    assert ok, rep


def test_load_checkpoint_directory_and_generate(tmp_path):
    """config.json with "model_type": "qwen3_vl" + safetensors under the HF key names (model.visual.* / model.language_model.*,
    conv weight (O, C, T, H, W)) + a tokenizer -> load() -> greedy tokens of generate_step against the restatement; then the user
    API over the processor: image -> smart resize at patch 16 -> patches -> placeholder expansion -> generate()"""
    from mlx_vlm_amd import generate, load
    from mlx_vlm_amd.generate import generate_step

    cfg = R.tiny_cfg()
    W = R.random_weights(cfg, seed=4321, dtype=BF, std=0.05, embed_std=0.2)
    R.write_checkpoint(tmp_path, cfg, W)
    model, processor = load(str(tmp_path), kv_pool_tokens=4096, max_seqs=4)
    assert type(model).__module__.endswith("qwen3_vl.qwen3_vl") and not model.language_model.quantized
    assert type(processor).__name__ == "Qwen3VLProcessor" and processor.image_processor.patch_size == 16
    ids, pix, thw = R.synth_request(cfg, [(1, 4, 6), (1, 8, 8)], n_text=11, seed=46)
    n_new = 10
    ref_toks, ref_logits = R.generate_greedy(W, cfg, ids, _pix(pix).to(BF), thw, max_tokens=n_new, return_logits=True)
    toks, lps = [], []
    for t, lp in generate_step(ids, model, _pix(pix), None, max_tokens=n_new, temperature=0.0, image_grid_thw=thw):
        toks.append(t)
        lps.append(lp.float().cpu())
    ok, n, margin = _tie_aware_equal(toks, ref_toks, ref_logits, tol=3e-2)
    assert ok and len(toks) == n_new, (toks, ref_toks, n, margin)
    ok, rep = bf16_close(lps[0], O.logprobs_from_logits(ref_logits[0][None])[0], ulps=2, atol_rms=3e-2)
    assert ok, rep
    from PIL import Image

    img = Image.fromarray(np.random.default_rng(3).integers(0, 256, (70, 100, 3), dtype=np.uint8))
    words = " ".join(f"t{int(i)}" for i in np.random.default_rng(4).integers(3, 1000, 9))
    out = generate(model, processor, f"<|vision_start|> <|image_pad|> <|vision_end|> {words}", image=img, max_tokens=6, temperature=0.0)
    assert out.prompt_tokens == 2 + 9 + (64 // 16) * (96 // 16) // 4 and out.generation_tokens >= 1
    # a vision-cache hit runs on the cached features, without DeepStack (the reference's rule): it still generates
    from mlx_vlm_amd.vision_cache import VisionFeatureCache

    vc = VisionFeatureCache()
    a = generate(model, processor, f"<|vision_start|> <|image_pad|> <|vision_end|> {words}", image=img, max_tokens=4, temperature=0.0,
                 vision_cache=vc)
    b = generate(model, processor, f"<|vision_start|> <|image_pad|> <|vision_end|> {words}", image=img, max_tokens=4, temperature=0.0,
                 vision_cache=vc)
    assert a.generation_tokens >= 1 and b.generation_tokens >= 1


def test_old_form_handles_are_untouched_by_a_qwen3_one(tiny):
    """a Qwen2-VL model (first tower form, fused qkv launches, no mode key) gives bit-identical tokens and log-probs before and
    after a Qwen3-VL model has run in the same process"""
    from mlx_vlm_amd.generate import generate_step
    from oracle import qwen2_vl as oq
    from tests.helpers import build_product_model, synth_request

    cfg2 = oq.tiny_cfg()
    W2 = oq.random_weights(cfg2, seed=1234, dtype=BF, std=0.05, embed_std=0.2)
    old = build_product_model(cfg2, W2, kv_pool_tokens=2048, max_seqs=4)
    ids2, pix2, thw2 = synth_request(cfg2, [(56, 84)], n_text=9, seed=3)
    run = lambda: [(t, lp.clone()) for t, lp in generate_step(ids2, old, torch.from_numpy(pix2), None, max_tokens=6,   # noqa: E731
                                                             temperature=0.0, image_grid_thw=thw2)]
    before = run()
    cfg, W, model = tiny
    ids, pix, thw = R.synth_request(cfg, [(1, 4, 6)], n_text=7, seed=5)
    assert len(list(generate_step(ids, model, _pix(pix), None, max_tokens=4, image_grid_thw=thw))) == 4
    after = run()
    assert [t for t, _ in before] == [t for t, _ in after]
    assert all(torch.equal(a, b) for (_, a), (_, b) in zip(before, after))
