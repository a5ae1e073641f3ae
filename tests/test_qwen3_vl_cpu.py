"""Qwen3-VL on the host: the torch restatement (tests/qwen3_vl_ref.py) against vectors recorded from the REFERENCE'S files over
oracle/mlx_shim (tests/golden/make_golden_ref_qwen3_vl.py: bit-exact in bf16 and fp32, fallback rope mode) and from transformers
(make_golden_hf_qwen3_vl.py: fp32 at 1e-4), the product's host tables against the same goldens, and the family's host logic
(config, sanitize, placeholder expansion, the refusals, the C ABI's size).  CPU only; only the .npz files are read."""
import os
import re

import numpy as np
import pytest
import torch

from tests import qwen3_vl_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "qwen3_vl_tiny_ref.npz"))
H = np.load(os.path.join(HERE, "golden", "qwen3_vl_tiny_hf.npz"))
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
FEAT_ROWS, EMB_ROWS, LOGIT_ROWS = slice(None, None, 2), slice(None, None, 3), slice(None, None, 7)     # as the script sampled
CASES = ["one_image", "three_images", "text_only"]
IMAGE_CASES = ["one_image", "three_images"]
INTERP = ["g4x6", "g2x2", "g8x8", "g2x6x4", "three"]
BF = torch.bfloat16


def _weights(dt):
    W = R.random_weights(R.tiny_cfg(), seed=1234, dtype=torch.float32, std=0.05, embed_std=0.2)
    return {k: v.to(dt) for k, v in W.items()}


def _request(case):
    grids = [tuple(g) for g in G[case + ".grids"].tolist()]
    return R.synth_request(R.tiny_cfg(), grids, n_text=12 if grids else 19, seed=len(grids))


def _exact(name, got, ref):
    got = got.detach().to(torch.float32).numpy()
    assert np.array_equal(got, ref), (name, int((got != ref).sum()), float(np.abs(got - ref).max()))


def _host_model():
    from mlx_vlm_amd.models.qwen3_vl import Model, ModelConfig

    return Model(ModelConfig.from_dict(R.model_config_dict(R.tiny_cfg())), device="cpu", kv_pool_tokens=1024, max_seqs=2)


# ---------------------------------------------------------------- restatement vs the reference (shim goldens), bit for bit
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", CASES)
def test_restatement_is_the_reference_bit_for_bit(case, dt):
    """tower features, every DeepStack tap, merged embeddings, position ids, prefill logits (with DeepStack) and 8 greedy steps on
    the cache, in fp32 and bf16 - rope_mode="fallback" is the pure-MLX rope path the reference runs without Metal"""
    cfg, W = R.tiny_cfg(), _weights(DT[dt])
    ids, pix, thw = _request(case)
    pixt = torch.from_numpy(pix) if pix is not None else None
    p = f"{case}.{dt}."
    logits, f = R.prefill_logits(W, cfg, ids, pixt, thw, rope_mode="fallback", return_features=True)
    if pix is not None:
        _exact("image_features", f.image_features[FEAT_ROWS], G[p + "ref_image_features"])
        assert len(f.deepstack_visual_embeds) == 2
        for j, tap in enumerate(f.deepstack_visual_embeds):
            _exact(f"tap{j}", tap[FEAT_ROWS], G[p + f"ref_tap{j}"])
        assert np.array_equal(f.visual_pos_masks, G[case + ".ref_visual_pos_masks"])
    _exact("inputs_embeds", f.inputs_embeds[0][EMB_ROWS], G[p + "ref_inputs_embeds"])
    assert np.array_equal(np.asarray(f.position_ids), G[case + ".ref_position_ids"])
    assert np.array_equal(np.asarray(f.rope_deltas).reshape(-1), G[case + ".ref_rope_deltas"])
    _exact("prefill rows", logits[LOGIT_ROWS], G[p + "ref_prefill_logits"])
    _exact("prefill last", logits[-1], G[p + "ref_prefill_last"])
    toks, rows = R.generate_greedy(W, cfg, ids, pixt, thw, max_tokens=9, return_logits=True, rope_mode="fallback")
    assert toks[:8] == G[p + "ref_greedy"].tolist()
    _exact("decode logits", rows[1:9], G[p + "ref_decode_logits"])


def test_deepstack_and_fused_rope_are_visible():
    """not vacuous: without the DeepStack adds the prefill logits are far from the reference's, and the fused rope mode (what
    the engine runs) differs from the fallback mode by bf16 roundings only"""
    cfg, W = R.tiny_cfg(), _weights(BF)
    ids, pix, thw = _request("one_image")
    f = R.get_input_embeddings(W, cfg, ids, torch.from_numpy(pix), thw)
    ref = torch.from_numpy(G["one_image.bf16.ref_prefill_last"])
    rel = lambda a: float((a.float() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())   # noqa: E731
    no_ds = R.lm_head(W, cfg, R.qwen3_model(W, cfg, f.inputs_embeds, None, R._pos3(f.position_ids), "fallback"))[0, -1]
    assert rel(no_ds) > 0.05
    fused = R.prefill_logits(W, cfg, ids, torch.from_numpy(pix), thw, rope_mode="fused")[-1]
    assert 0 < rel(fused) < 2e-2
    # a cached-feature prompt runs without DeepStack (qwen3_vl.py:70-79)
    c = R.get_input_embeddings(W, cfg, ids, None, thw, cached_image_features=f.image_features)
    assert c.deepstack_visual_embeds is None and torch.equal(c.inputs_embeds, f.inputs_embeds)


def test_tower_additions_are_visible_at_the_gpu_tests_bar():
    """the GPU tower test holds features to 2e-2 relative rms: a tower without the position rows, or without the patch bias,
    is further from the restatement than that, so the bar sees either omission"""
    cfg, W = R.tiny_cfg(), _weights(BF)
    _, pix, thw = R.synth_request(cfg, [(1, 4, 6)], seed=3)
    ref, _ = R.vision_tower(W, cfg, torch.from_numpy(pix).to(BF), thw)
    rel = lambda a: float((a.float() - ref.float()).pow(2).mean().sqrt() / ref.float().pow(2).mean().sqrt())   # noqa: E731
    for key in ("vision_tower.pos_embed.weight", "vision_tower.patch_embed.proj.bias"):
        W0 = dict(W)
        W0[key] = torch.zeros_like(W[key])
        assert rel(R.vision_tower(W0, cfg, torch.from_numpy(pix).to(BF), thw)[0]) > 2e-2, key


# ---------------------------------------------------------------- restatement vs transformers
@pytest.mark.parametrize("case", IMAGE_CASES)
def test_restatement_matches_hf(case):
    """fp32 restatement vs Qwen3VLForConditionalGeneration: tower features, both taps, position ids, prompt logits at atol 1e-4"""
    cfg, W = R.tiny_cfg(), _weights(torch.float32)
    ids, pix, thw = _request(case)
    logits, f = R.prefill_logits(W, cfg, ids, torch.from_numpy(pix), thw, return_features=True)
    np.testing.assert_allclose(f.image_features.numpy(), H[case + ".hf_image_features"], rtol=0, atol=1e-4)
    for j, tap in enumerate(f.deepstack_visual_embeds):
        np.testing.assert_allclose(tap.numpy(), H[case + f".hf_tap{j}"], rtol=0, atol=1e-4)
    assert np.array_equal(np.asarray(f.position_ids), H[case + ".hf_position_ids"])
    assert np.array_equal(np.asarray(f.rope_deltas).reshape(-1), H[case + ".hf_rope_deltas"].reshape(-1))
    np.testing.assert_allclose(logits.numpy()[::3], H[case + ".hf_logits"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(logits.numpy()[-1], H[case + ".hf_logits_last"], rtol=0, atol=1e-4)


# ---------------------------------------------------------------- host tables vs the goldens
def test_interleaved_selector():
    sel = R.interleaved_position_selector([24, 20, 20], 64)
    assert np.array_equal(sel.numpy(), G["selector.interleaved"])
    assert np.array_equal(R.interleaved_position_selector([16, 24, 24], 64).numpy(), G["selector.interleaved_16_24_24"])
    assert np.array_equal(R.interleaved_position_selector([8, 4, 4], 16).numpy(), G["selector.interleaved_8_4_4_dim16"])
    # the rule the kernel evaluates (csrc/rope.hip): h where f % 3 == 1 and f < 3 sec1, w where f % 3 == 2 and f < 3 sec2, else t
    f = np.arange(64)
    rule = np.where((f % 3 == 1) & (f < 60), 1, np.where((f % 3 == 2) & (f < 60), 2, 0))
    assert np.array_equal(rule, G["selector.interleaved"])
    assert rule[60:].tolist() == [0, 0, 0, 0] and rule[57:60].tolist() == [0, 1, 2]        # 61 .. 63 fall back to t


@pytest.mark.parametrize("case", CASES)
def test_product_rope_index_equals_the_references(case):
    m = _host_model()
    ids, _, thw = _request(case)
    pos, deltas = m.language_model.get_rope_index(ids, thw)
    assert np.array_equal(np.asarray(pos), G[case + ".ref_position_ids"])
    assert np.array_equal(np.asarray(deltas).reshape(-1), G[case + ".ref_rope_deltas"])
    with pytest.raises(NotImplementedError, match="video"):
        m.language_model.get_rope_index(ids, None, np.array([[2, 4, 4]]))


def _dense(idx, wt, n_pos):
    """the four typed products of an identity table summed left to right, as fast_pos_embed_interpolate sums them"""
    out = None
    for k in range(4):
        e = np.zeros((idx.shape[1], n_pos), dtype=np.float32)
        e[np.arange(idx.shape[1]), idx[k]] = wt[k]
        out = e if out is None else (out + e).astype(np.float32)
    return out


@pytest.mark.parametrize("name", INTERP)
def test_interpolation_indices_and_weights(name):
    """the product's host tables and the restatement's, against the reference's own fast_pos_embed_interpolate run over an
    identity position table (each output row then shows its four corner indices and weights), rows in merge-unit order"""
    from mlx_vlm_amd.models.qwen3_vl.vision import pos_embed_tables

    grids = G[f"interp.{name}.grids"]
    ref = G[f"interp.{name}.dense"]
    idx, wt = pos_embed_tables(grids, 8, 2)
    assert idx.shape == wt.shape == (4, ref.shape[0]) and wt.dtype == np.float32
    assert np.array_equal(_dense(idx, wt, 64), ref)
    cfg = R.tiny_cfg()
    W = {"vision_tower.pos_embed.weight": torch.eye(64)}
    assert np.array_equal(R.fast_pos_embed_interpolate(W, cfg, grids).numpy(), ref)
    if name == "g8x8":                    # the table's own grid: every weight is exactly 0 or 1, every row is ONE table row
        assert set(np.unique(wt).tolist()) == {0.0, 1.0} and np.array_equal(ref.sum(1), np.ones(64, np.float32))
        order = np.arange(64).reshape(4, 2, 4, 2).transpose(0, 2, 1, 3).reshape(-1)
        assert np.array_equal(ref.argmax(1), order)
    if name == "g2x2":                    # the four corners of the table
        assert sorted(ref.argmax(1).tolist()) == [0, 7, 56, 63]


@pytest.mark.parametrize("name", INTERP)
def test_rot_pos_emb(name):
    from mlx_vlm_amd.models.qwen3_vl import VisionConfig, VisionModel

    vm = VisionModel(VisionConfig.from_dict(R.model_config_dict(R.tiny_cfg())["vision_config"]), device="cpu")
    np.testing.assert_allclose(vm.rot_pos_emb(G[f"interp.{name}.grids"]).numpy(), G[f"interp.{name}.rot_pos_emb"], rtol=0, atol=0)


def test_product_interpolation_rows_on_the_host():
    """VisionModel.fast_pos_embed_interpolate (torch ops on the tower's device - here the host) gives the restatement's rows"""
    from mlx_vlm_amd.models.qwen3_vl import VisionConfig, VisionModel

    cfg = R.tiny_cfg()
    W = R.random_weights(cfg, seed=3, dtype=BF, tower_only=True)
    vm = VisionModel(VisionConfig.from_dict(R.model_config_dict(cfg)["vision_config"]), device="cpu")
    vm._w["pos_embed.weight"] = W["vision_tower.pos_embed.weight"]
    grids = np.array([(1, 4, 6), (2, 6, 4), (1, 2, 2)])
    assert torch.equal(vm.fast_pos_embed_interpolate(grids), R.fast_pos_embed_interpolate(W, cfg, grids))


# ---------------------------------------------------------------- host logic of the family
def test_config_round_trip():
    from mlx_vlm_amd.models.qwen3_vl import ModelConfig, TextConfig, VisionConfig

    v = VisionConfig()
    assert (v.patch_size, v.num_position_embeddings, v.deepstack_visual_indexes) == (14, 2304, [])
    assert v.deepstack_visual_indexes is not VisionConfig().deepstack_visual_indexes
    d = R.model_config_dict(R.tiny_cfg())
    d["unknown_key"] = 1
    mc = ModelConfig.from_dict(d)
    t = mc.text_config
    assert mc.model_type == "qwen3_vl" and (mc.image_token_index, mc.video_token_index) == (2001, 2002)
    assert (t.head_dim, t.num_key_value_heads, t.hidden_size, t.attention_bias) == (128, 2, 256, False)
    assert t.rope_scaling["type"] == "default" and t.rope_scaling["mrope_section"] == [24, 20, 20] and t.rope_scaling["mrope_interleaved"]
    assert mc.vision_config.deepstack_visual_indexes == [0, 2] and mc.vision_config.num_position_embeddings == 64
    again = ModelConfig.from_dict(dict(mc.to_dict(), text_config=t.to_dict(), vision_config=mc.vision_config.to_dict()))
    assert again.text_config.to_dict() == t.to_dict() and again.vision_config.to_dict() == mc.vision_config.to_dict()
    assert TextConfig(**dict(d["text_config"], rope_scaling=None)).rope_scaling is None
    with pytest.raises(ValueError, match="rope_scaling"):
        ModelConfig.from_dict(dict(d, text_config=dict(d["text_config"], rope_scaling={"type": "mrope"})))


def test_sanitize_vs_reference():
    m = _host_model()
    keys = list(G["sanitize.hf_keys"])
    w = {k: (torch.from_numpy(G["sanitize.hf_conv"]) if k.endswith("patch_embed.proj.weight") else torch.zeros(3)) for k in keys}
    w["model.visual.blocks.0.attn.position_ids"] = torch.zeros(1)
    out = m.sanitize(w)
    vt = m.vision_tower.sanitize({k: v for k, v in out.items() if k.startswith("vision_tower.")})
    got = [k for k in out if not k.startswith("vision_tower.")] + list(vt)
    assert sorted(got) == sorted(G["sanitize.ref_keys"].tolist())
    assert np.array_equal(vt["vision_tower.patch_embed.proj.weight"].numpy(), G["sanitize.ref_conv"])
    # the inverse used by the checkpoint writers of the tests
    W = R.random_weights(R.tiny_cfg(), seed=1, tower_only=False)
    back = m.sanitize(R.to_hf_keys(W))
    assert sorted(back) == sorted(W)


def test_family_is_found_by_name_processor_and_placeholder_expansion(tmp_path):
    from mlx_vlm_amd import utils
    from mlx_vlm_amd.models.qwen2_vl import LanguageModel as Base

    arch, mt = utils.get_model_and_args({"model_type": "qwen3_vl"})
    assert mt == "qwen3_vl" and arch.Model.__module__.endswith("qwen3_vl.qwen3_vl")
    assert issubclass(arch.LanguageModel, Base) and arch.LanguageModel is not Base and arch.LanguageModel.DEEPSTACK
    cfg = R.tiny_cfg()
    R.write_checkpoint(tmp_path, cfg, {})
    proc = utils.load_processor(str(tmp_path), arch.ModelConfig.from_dict(R.model_config_dict(cfg)))
    ip = proc.image_processor
    assert type(proc).__name__ == "Qwen3VLProcessor" and (ip.patch_size, ip.merge_size, ip.image_mean, ip.image_std) == (16, 2, [0.5] * 3, [0.5] * 3)
    from PIL import Image

    img = Image.fromarray(np.random.default_rng(0).integers(0, 256, (70, 100, 3), dtype=np.uint8))
    out = proc(images=[img], text="<|vision_start|> <|image_pad|> <|vision_end|> t5 t6", return_mm_token_type_ids=True)
    gh, gw = (int(x) for x in out["image_grid_thw"][0, 1:])
    assert (gh * 16, gw * 16) == (64, 96) and out["pixel_values"].shape == (gh * gw, 3 * 2 * 16 * 16)
    ids = out["input_ids"][0].tolist()
    assert ids.count(cfg.image_token_id) == gh * gw // 4 and len(ids) == 4 + gh * gw // 4
    assert out["mm_token_type_ids"][0].count(1) == gh * gw // 4
    with pytest.raises(NotImplementedError, match="video"):
        proc(images=None, text="t5", videos=[object()])


def test_message_format_puts_the_images_first():
    """the reference's prompt_utils gives qwen3_vl LIST_WITH_IMAGE_FIRST (48)"""
    from mlx_vlm_amd import prompt_utils as pu

    msg = pu.get_message_json("qwen3_vl", "hi", num_images=2)
    assert msg == {"role": "user", "content": [{"type": "image"}, {"type": "image"}, {"type": "text", "text": "hi", "content": "hi"}]}
    with pytest.raises(NotImplementedError, match="video"):
        pu.get_message_json("qwen3_vl", "hi", video="clip.mp4")


def test_refusals(tmp_path):
    """what the README lists as unbuilt for this family raises NotImplementedError"""
    from mlx_vlm_amd import utils
    from mlx_vlm_amd.models.qwen3_vl import Model, ModelConfig

    with pytest.raises(NotImplementedError, match="qwen3_vl_moe"):
        utils.get_model_and_args({"model_type": "qwen3_vl_moe"})
    with pytest.raises(NotImplementedError, match="moe"):
        Model(ModelConfig.from_dict(dict(R.model_config_dict(R.tiny_cfg()), model_type="qwen3_vl_moe")), device="cpu")
    m = _host_model()
    ids, pix, thw = _request("one_image")
    with pytest.raises(NotImplementedError, match="video"):
        m.get_input_embeddings(ids, None, pixel_values_videos=torch.zeros(4, 1536), video_grid_thw=np.array([[2, 2, 2]]))
    with pytest.raises(NotImplementedError, match="Qwen2-VL"):
        utils.load_processor("/nonexistent", type("C", (), {"model_type": "qwen3_vl"})(), image_preprocess="device")
    from mlx_vlm_amd.convert import convert

    R.write_checkpoint(tmp_path, R.tiny_cfg(), {})
    with pytest.raises(NotImplementedError, match="qwen3_vl"):
        convert(str(tmp_path), str(tmp_path / "out"))
    from mlx_vlm_amd.apc import APCManager
    from mlx_vlm_amd.batch import BatchGenerator

    mgr = APCManager(num_blocks=2)
    try:
        with pytest.raises(NotImplementedError, match="DeepStack"):
            BatchGenerator(m, None, max_tokens=4, apc_manager=mgr)
    finally:
        mgr.close()


def test_tower_refuses_head_dim_72_and_pads_the_mlp():
    """the 8B / 32B towers (1152 / 16 heads = 72): refused at load, naming head_dim; 4304 is padded to 4352"""
    from mlx_vlm_amd.models.qwen3_vl import VisionConfig, VisionModel

    cfg = R.tiny_cfg(hidden_size=144, num_heads=2)
    W = R.random_weights(cfg, seed=1, tower_only=True)
    vm = VisionModel(VisionConfig.from_dict(R.model_config_dict(cfg)["vision_config"]), device="cpu")
    assert vm.head_dim == 72
    with pytest.raises(NotImplementedError, match="head_dim = 72"):
        vm.load_weights({k[len("vision_tower."):]: v for k, v in W.items()})
    big = VisionModel(VisionConfig(hidden_size=1152, num_heads=16, intermediate_size=4304, patch_size=16), device="cpu")
    assert (big.mlp_hidden, big.patch_k, big.num_grid_per_side) == (4352, 1536, 48)
    tiny = VisionModel(VisionConfig.from_dict(R.model_config_dict(R.tiny_cfg())["vision_config"]), device="cpu")
    assert (tiny.head_dim, tiny.mlp_hidden, tiny.deepstack_visual_indexes) == (64, 384, [0, 2])


def test_language_model_refuses_other_head_dims():
    from mlx_vlm_amd.models.qwen3_vl import Model, ModelConfig

    d = R.model_config_dict(R.tiny_cfg())
    d["text_config"] = dict(d["text_config"], head_dim=64, rope_scaling={"type": "default", "mrope_section": [12, 10, 10]})
    with pytest.raises(NotImplementedError, match="head_dim = 64"):
        Model(ModelConfig.from_dict(d), device="cpu")


def test_deepstack_window_slices_as_the_reference():
    """models/base.deepstack_window: mask and embeds of a prompt chunk (reference language.py:528-558)"""
    from mlx_vlm_amd.models.base import deepstack_window

    mask = np.zeros((1, 20), dtype=bool)
    mask[0, [2, 3, 4, 9, 10, 17]] = True
    emb = torch.arange(2 * 6 * 3, dtype=torch.float32).reshape(2, 6, 3)
    e, rows = deepstack_window(mask, emb, 0, 20)
    assert torch.equal(e, emb) and rows.tolist() == [2, 3, 4, 9, 10, 17]
    e, rows = deepstack_window(mask, emb, 4, 7)                     # columns 4 .. 10: the third, fourth and fifth visual rows
    assert torch.equal(e, emb[:, 2:5]) and rows.tolist() == [0, 5, 6]
    assert deepstack_window(mask, emb, 11, 6) is None and deepstack_window(mask, None, 0, 20) is None
    e, rows = deepstack_window(mask, [emb[0], emb[1]], 17, 3)
    assert torch.equal(e, emb[:, 5:6]) and rows.tolist() == [0]
    two = np.concatenate([mask, mask])
    e, rows = deepstack_window(two, torch.cat([emb, emb], 1), 0, 20)
    assert rows.tolist() == [2, 3, 4, 9, 10, 17, 22, 23, 24, 29, 30, 37]
    with pytest.raises(NotImplementedError):
        deepstack_window(two, torch.cat([emb, emb], 1), 4, 7)


def test_abi_still_60_names_version_8_and_struct_mirrors():
    root = os.path.dirname(HERE)
    hdr = open(os.path.join(root, "include", "vlm_hip.h")).read()
    assert len(set(re.findall(r"\b(vlm_[a-z0-9_]+)\s*\(", hdr))) == 60
    from mlx_vlm_amd import _lib

    assert len(_lib.SIGNATURES) == 60
    assert re.search(r"vlm_abi_version\(void\)\s*\{\s*return 8;", open(os.path.join(root, "mlx-vlm_amd", "csrc", "engine.hip")).read())
    # the appended fields sit at the END of their structs, in the header's order
    for cls, tail in ((_lib.LlmLayer, ["q_norm_w", "k_norm_w"]), (_lib.PrefillArgs, ["ds_embeds", "ds_rows", "n_ds", "n_ds_rows"]),
                      (_lib.VitBlock, ["tap_ln_w", "tap_ln_b", "tap_w0", "tap_b0", "tap_w2", "tap_b2"]), (_lib.VitGlobals, ["bpatch"]),
                      (_lib.VitArgs, ["pos_rows", "tap_out", "n_taps"])):
        names = [n for n, _ in cls._fields_]
        assert names[-len(tail):] == tail, (cls.__name__, names)
        struct = re.search(r"typedef struct (\w+) \{(.*?)\} \1;", hdr[hdr.index("typedef struct " + {
            "LlmLayer": "vlm_llm_layer", "PrefillArgs": "vlm_prefill_args", "VitBlock": "vlm_vit_block",
            "VitGlobals": "vlm_vit_globals", "VitArgs": "vlm_vit_args"}[cls.__name__]):], re.S).group(2)
        body = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
        order = [body.index(n) for n in tail]
        assert order == sorted(order) and all(body.index(n) > body.index(names[-len(tail) - 1]) for n in tail)
    assert (_lib.MODE_QWEN3, _lib.VIT_FORM_QWEN3) == (19, 4) and "#define VLM_MODE_QWEN3 19" in hdr and "#define VLM_VIT_FORM_QWEN3 4" in hdr
    assert "#define VLM_EPI_GELU_TANH 256" in hdr
