"""The InternVL3 / InternVL3.5 family on the GPU against the torch restatement (tests/internvl_ref.py, itself pinned bit for bit to
the reference and at 1e-4 to transformers by tests/test_internvl_cpu.py): the InternViT tower on the layer-scale encoder loop with
the pixel-shuffle connector, and the family end to end on the tiny models (2 decoder layers; the Qwen2 form with biases and
64-wide heads, the Qwen3 form with QK-norm and 128-wide heads) - prefill, teacher-forced and greedy decode, captured against eager
steps, the batch generator, the shared language model's options, MLX 4-bit weights, load() of a checkpoint directory.

Bars: tower / features 2e-2 relative rms (tests/test_vlm_family_llava_bunny_gpu.py, tests/test_vlm_family_idefics2_gpu.py); logits
2e-2 relative rms per row and bf16_close(ulps=4, atol_rms=8e-2) (tests/test_engine_gpu.py's tiny tests); greedy tokens tie-aware."""
import numpy as np
import pytest
import torch

from oracle import ops as O
from tests import internvl_ref as R
from tests.helpers import bf16_close
from tests.test_engine_gpu import _tie_aware_equal

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
FORMS = ["qwen2", "qwen3"]


def _rel_rms_err(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30))


def _pix(pix):
    return torch.from_numpy(pix) if pix is not None else None


@pytest.fixture(scope="module")
def tiny():
    """both forms on the same seed (so the same tower), built once"""
    out = {}
    for lm in FORMS:
        cfg = R.tiny_cfg(lm)
        W = R.random_weights(cfg, seed=1234, dtype=BF)
        out[lm] = (cfg, W, R.build_product_model(cfg, W, kv_pool_tokens=4096, max_seqs=16))
    return out


@pytest.fixture(scope="module")
def forced_refs(tiny):
    """per form: a 2-tile prompt with the restatement's teacher-forced logits over 40 steps - computed once, shared, not modified"""
    out = {}
    for lm in FORMS:
        cfg, W, _ = tiny[lm]
        ids, pix = R.synth_request(cfg, [2], n_text=14, seed=44)
        forced = np.random.default_rng(45).integers(3, 1000, 40)
        out[lm] = (ids, pix, forced, R.decode_teacher_forced(W, cfg, ids, _pix(pix), forced))
    return out


# ---------------------------------------------------------------- tower + connector
@pytest.mark.parametrize("tiles", [1, 3])
def test_tower_and_connector_vs_restatement(tiny, tiles):
    """VisionModel's last state (CLS row included) and the mlp1 features for 1 tile and for 3 (2 + thumbnail)"""
    cfg, W, model = tiny["qwen2"]
    _, pix = R.synth_request(cfg, [tiles], seed=3 + tiles)
    ref_last = R.vision_tower(W, cfg, _pix(pix).to(BF))
    last = model.vision_model(_pix(pix))
    assert last.shape == (tiles * 17, cfg.vision.hidden_size)
    e_last = _rel_rms_err(last, ref_last.reshape(tiles * 17, -1))
    ref_feats = R.connector(W, cfg, ref_last).reshape(tiles * 4, -1)
    feats = model.encode_image(_pix(pix))
    assert feats.shape == ref_feats.shape == (tiles * 4, cfg.text.hidden_size)
    e_feat = _rel_rms_err(feats, ref_feats)
    print(f"tower {tiles} tile(s): rel-rms last state {e_last:.4f}, features {e_feat:.4f}")
    assert e_last < 2e-2 and e_feat < 2e-2, (e_last, e_feat)
    assert _rel_rms_err(last.view(tiles, 17, -1)[:, 0], ref_last[:, 0]) < 2e-2                     # the CLS rows by themselves
    # the connector alone on the restatement's own tower output: gather table + LayerNorm(4E) + two GEMMs
    assert _rel_rms_err(model.connector(ref_last.reshape(tiles * 17, -1).cuda()), ref_feats) < 2e-2
    # without the layer scale the tower is far away (the bar sees the feature), and the 5-D form of the processor is taken
    W1 = {k: (torch.ones_like(v) if k.endswith((".ls1", ".ls2")) else v) for k, v in W.items()}
    assert _rel_rms_err(last, R.vision_tower(W1, cfg, _pix(pix).to(BF)).reshape(tiles * 17, -1)) > 0.1
    assert torch.equal(model.encode_image(_pix(pix)[None]), feats)
    if tiles > 1:            # tiles never see each other: a tile alone gives its rows of the joint call, bit for bit
        assert torch.equal(model.vision_model(_pix(pix[1:2])), last[17:34])


# ---------------------------------------------------------------- end to end
@pytest.mark.parametrize("lm", FORMS)
def test_prefill_and_teacher_forced_decode_40_steps(tiny, forced_refs, lm):
    """prefill of a 2-tile prompt through the module call, then 40 forced tokens: every row's logits against the restatement"""
    cfg, W, model = tiny[lm]
    ids, pix, forced, ref = forced_refs[lm]
    llm = model.language_model
    cache = llm.make_cache()
    out = model(ids, _pix(pix), cache=cache, logits_to_keep=1)
    rows = [out.logits[0, -1].clone()]
    for y in forced:
        rows.append(llm(np.array([[int(y)]]), cache=cache).logits[0, -1].clone())
    cache[0]._seq.release()
    got = torch.stack(rows)
    worst = max(_rel_rms_err(got[i], ref[i]) for i in range(ref.shape[0]))
    print(f"{lm}: prefill + {len(forced)} teacher-forced steps, worst row rel-rms {worst:.4f}")
    assert got.shape == ref.shape and worst < 2e-2, worst
    ok, rep = bf16_close(got, ref, ulps=4, atol_rms=8e-2)
    assert ok, rep


@pytest.mark.parametrize("lm", FORMS)
def test_every_prompt_row_and_positions(tiny, lm):
    cfg, W, model = tiny[lm]
    ids, pix = R.synth_request(cfg, [1, 2], n_text=9, seed=12)
    f = model.get_input_embeddings(ids, _pix(pix))
    ref_emb = R.get_input_embeddings(W, cfg, ids, _pix(pix))
    where = ids[0] == cfg.image_token_index
    assert int(where.sum()) == 12
    assert torch.equal(f.inputs_embeds[0, ~where].cpu(), ref_emb[0, ~where])                     # embedding rows: exact
    assert _rel_rms_err(f.inputs_embeds[0, where], ref_emb[0, where]) < 2e-2
    L = ids.shape[1]
    assert np.array_equal(np.asarray(f.position_ids), np.broadcast_to(np.arange(L), (3, 1, L))) and not np.asarray(f.rope_deltas).any()
    llm = model.language_model
    cache = llm.make_cache()
    out = llm(ids, f.inputs_embeds, cache=cache, position_ids=f.position_ids)
    cache[0]._seq.release()
    ref = R.language_model(W, cfg, ref_emb)[0]
    worst = max(_rel_rms_err(out.logits[0, i], ref[i]) for i in range(L))
    assert out.logits.shape == (1, L, cfg.text.vocab_size) and worst < 2e-2, worst


@pytest.mark.parametrize("lm", FORMS)
def test_generate_step_captured_equals_eager_and_the_restatement(tiny, lm):
    """generate_step on the captured graph: tokens and log-probs bit for bit the eager steps', tokens the restatement's (tie-aware)"""
    from mlx_vlm_amd.generate import generate_step

    cfg, W, model = tiny[lm]
    ids, pix = R.synth_request(cfg, [3], n_text=9, seed=71)

    def run(use_graph):
        out = [(t, lp.clone()) for t, lp in generate_step(ids, model, _pix(pix), None, max_tokens=16, temperature=0.0, use_graph=use_graph)]
        return [t for t, _ in out], torch.stack([lp for _, lp in out])

    (ta, la), (tb, lb) = run(True), run(False)
    assert ta == tb and torch.equal(la, lb) and len(ta) == 16
    ref_toks, ref_logits = R.generate_greedy(W, cfg, ids, _pix(pix), max_tokens=16, return_logits=True)
    ok, n, margin = _tie_aware_equal(ta, ref_toks, ref_logits, tol=3e-2)
    assert ok, (ta, ref_toks, n, margin)
    ok, rep = bf16_close(la[0], O.logprobs_from_logits(ref_logits[0][None])[0], ulps=2, atol_rms=3e-2)
    assert ok, rep


def test_batch_generator_equals_single_requests(tiny):
    """3 mixed requests (0, 1 and 2 images) through the BatchGenerator against the same requests alone, under the rule of the other
    families' batch tests: every compared step's log-prob within 2 ulps of the step's log-prob span, tokens equal up to the first
    tie, at least 80 % of all tokens equal"""
    from mlx_vlm_amd.batch import BatchGenerator
    from mlx_vlm_amd.generate import generate_step

    cfg, W, model = tiny["qwen2"]
    reqs = [R.synth_request(cfg, [], n_text=15, seed=62), R.synth_request(cfg, [3], n_text=7, seed=61),
            R.synth_request(cfg, [1, 2], n_text=5, seed=63)]
    max_tokens = [6, 8, 8]
    singles = [[(t, float(lp[t]), float(lp.float().abs().max())) for t, lp in generate_step(ids, model, _pix(pix), None, max_tokens=m)]
               for (ids, pix), m in zip(reqs, max_tokens)]
    gen = BatchGenerator(model, None, max_tokens=8, completion_batch_size=8, prefill_batch_size=4)
    kw = [dict(pixel_values=_pix(p)) if p is not None else {} for _, p in reqs]
    uids = gen.insert([r[0].reshape(-1) for r in reqs], list(max_tokens), prompt_kwargs=kw)
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
    for (ids, pix), m, single in zip(reqs, max_tokens, singles):
        ref_toks, ref_logits = R.generate_greedy(W, cfg, ids, _pix(pix), max_tokens=m, return_logits=True)
        ok, n, margin = _tie_aware_equal([t for t, _, _ in single], ref_toks, ref_logits, tol=3e-2)
        assert ok, (ref_toks, single, n, margin)
    from mlx_vlm_amd.apc import APCManager

    with pytest.raises(NotImplementedError, match="get_input_embeddings"):
        BatchGenerator(model, None, max_tokens=4, apc_manager=APCManager(num_blocks=8))


@pytest.mark.parametrize("lm", FORMS)
def test_generate_step_options_of_the_shared_language_model(tiny, lm):
    """prompt_cache, kv_bits=8, max_kv_size and chunked prefill live in the shared language model: they run for this family and stay
    close to the plain run; the kv_bits=8 run is held to the restatement over the quantized cache"""
    from mlx_vlm_amd.generate import generate_step

    cfg, W, model = tiny[lm]
    ids, pix = R.synth_request(cfg, [2], n_text=9, seed=21)
    run = lambda **kw: [(t, lp.float().cpu()) for t, lp in generate_step(ids, model, _pix(pix), None, max_tokens=5,   # noqa: E731
                                                                        temperature=0.0, **kw)]
    plain = run()
    cache = model.language_model.make_cache()
    cached = run(prompt_cache=cache)
    assert [t for t, _ in cached] == [t for t, _ in plain] and cache[0].offset >= ids.shape[1]
    cache[0]._seq.release()
    q8 = run(kv_bits=8, quantized_kv_start=0)
    ok, rep = bf16_close(q8[0][1], plain[0][1], ulps=2, atol_rms=3e-2)
    assert ok and len(q8) == 5, rep
    ref8 = R.decode_teacher_forced(W, cfg, ids, _pix(pix), [q8[0][0]], kv_bits=8)
    ok, rep = bf16_close(q8[1][1], O.logprobs_from_logits(ref8[1][None])[0], ulps=2, atol_rms=8e-2)      # a step over the 8-bit pools
    assert ok, rep
    win = run(max_kv_size=64)
    assert len(win) == 5 and win[0][0] == plain[0][0]
    chunked = run(prefill_step_size=7)
    ok, rep = bf16_close(chunked[0][1], plain[0][1], ulps=2, atol_rms=3e-2)
    assert ok, rep


def test_quantized_4bit_language_model_vs_restatement():
    """the language model in MLX 4-bit (embedding, every Linear, the head; q / k norms bf16), tower and mlp1 bf16: teacher-forced
    logits against the restatement on the SAME quantized weights at the 4-bit bar of the other families (2e-2 rel-rms per row,
    4 ulps + 8e-2 of the rms); then mlp1's Linears quantized too: dequantised once at load, features 2e-2 of the dequantised run"""
    from oracle import quant as Q

    cfg = R.tiny_cfg("qwen3")
    W = R.random_weights(cfg, seed=1234, dtype=BF)
    ck, ow = Q.quantize_checkpoint(W, predicate=lambda p, v: p.startswith("language_model."))
    ck = {k: (v.view(torch.uint32) if v.dtype == torch.int32 else v) for k, v in ck.items()}
    model = R.build_product_model(cfg, ck, kv_pool_tokens=2048, max_seqs=4)
    llm = model.language_model
    assert llm.quantized
    ids, pix = R.synth_request(cfg, [1], n_text=14, seed=44)
    forced = np.random.default_rng(45).integers(3, 1000, 24)
    ref = R.decode_teacher_forced(ow, cfg, ids, _pix(pix), forced)
    cache = llm.make_cache()
    out = model(ids, _pix(pix), cache=cache, logits_to_keep=1)
    rows = [out.logits[0, -1].clone()]
    for y in forced:
        rows.append(llm(np.array([[int(y)]]), cache=cache).logits[0, -1].clone())
    cache[0]._seq.release()
    got = torch.stack(rows)
    worst = max(_rel_rms_err(got[i], ref[i]) for i in range(ref.shape[0]))
    print(f"4-bit teacher-forced: worst row rel-rms {worst:.4f}")
    assert worst < 2e-2, worst
    ok, rep = bf16_close(got, ref, ulps=4, atol_rms=8e-2)
    assert ok, rep
    ck2, ow2 = Q.quantize_checkpoint(W, predicate=lambda p, v: p.startswith(("mlp1.1", "mlp1.3")))
    ck2 = {k: (v.view(torch.uint32) if v.dtype == torch.int32 else v) for k, v in ck2.items()}
    m2 = R.build_product_model(cfg, ck2, kv_pool_tokens=1024, max_seqs=2)
    dq = {k: (Q.dequantize(v.wq, v.scales, v.biases) if hasattr(v, "wq") else v) for k, v in ow2.items()}
    assert _rel_rms_err(m2.encode_image(_pix(pix)), R.image_features(dq, cfg, _pix(pix))) < 2e-2


def test_load_checkpoint_directory_and_generate(tmp_path):
    """config.json with "model_type": "internvl_chat" + safetensors under the checkpoint's names (conv weight (O, C, kH, kW)) + a
    tokenizer -> load() -> greedy tokens of generate_step against the restatement; then the user API over the processor: image ->
    dynamic tiling -> <img> <IMG_CONTEXT> x 4 x tiles </img> -> generate(), and a vision-cache hit"""
    from mlx_vlm_amd import generate, load
    from mlx_vlm_amd.generate import generate_step

    cfg = R.tiny_cfg("qwen2")
    W = R.random_weights(cfg, seed=4321, dtype=BF)
    R.write_checkpoint(tmp_path, cfg, W)
    model, processor = load(str(tmp_path), kv_pool_tokens=4096, max_seqs=4)
    assert type(model).__module__.endswith("internvl_chat.internvl_chat") and not model.language_model.quantized
    assert type(processor).__name__ == "InternVLChatProcessor" and processor.image_processor.size == 56 and processor.num_image_token == 4
    assert processor.image_processor.dynamic_max_num == 4 and processor.img_context_token_id == cfg.image_token_index
    ids, pix = R.synth_request(cfg, [2, 1], n_text=11, seed=46)
    n_new = 10
    ref_toks, ref_logits = R.generate_greedy(W, cfg, ids, _pix(pix), max_tokens=n_new, return_logits=True)
    toks = [t for t, _ in generate_step(ids, model, _pix(pix), None, max_tokens=n_new, temperature=0.0)]
    ok, n, margin = _tie_aware_equal(toks, ref_toks, ref_logits, tol=3e-2)
    assert ok and len(toks) == n_new, (toks, ref_toks, n, margin)
    from PIL import Image

    img = Image.fromarray(np.random.default_rng(3).integers(0, 256, (50, 100, 3), dtype=np.uint8))          # 2 : 1 -> 2 tiles + thumbnail
    word_ids = np.random.default_rng(4).integers(3, 1000, 9)
    words = " ".join(f"t{int(i)}" for i in word_ids)
    out = generate(model, processor, f"<image> {words}", image=img, max_tokens=6, temperature=0.0)
    assert out.prompt_tokens == 2 + 9 + 4 * 3 and out.generation_tokens >= 1
    # ... and those tokens are the restatement's on the processor's own pixel values
    pv = processor(text=f"<image> {words}", images=[img])
    assert pv["pixel_values"].shape == (3, 3, 56, 56)
    ref_toks, ref_logits = R.generate_greedy(W, cfg, pv["input_ids"], _pix(pv["pixel_values"]), max_tokens=6, return_logits=True)
    got = [int(w[1:]) for w in out.text.split() if w.startswith("t")]
    ok, n, margin = _tie_aware_equal(got, ref_toks[:len(got)], ref_logits, tol=3e-2)
    assert ok and len(got) >= 1, (got, ref_toks, n, margin)
    from mlx_vlm_amd.vision_cache import VisionFeatureCache

    vc = VisionFeatureCache()
    a = generate(model, processor, f"<image> {words}", image=img, max_tokens=4, temperature=0.0, vision_cache=vc)
    b = generate(model, processor, f"<image> {words}", image=img, max_tokens=4, temperature=0.0, vision_cache=vc)
    assert a.text == b.text and a.generation_tokens >= 1
