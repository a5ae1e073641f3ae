"""Qwen2.5-VL on the host: the window tables against the reference's own, the torch restatement (tests/qwen2_5_vl_ref.py) against
vectors recorded from the REFERENCE'S files over oracle/mlx_shim (tests/golden/make_golden_ref_qwen2_5_vl.py) and from
transformers (make_golden_hf_qwen2_5_vl.py), and the family's host logic (config, sanitize, the MLP zero padding, construction).
CPU only; only the .npz files are read."""
import os
import re

import numpy as np
import pytest
import torch

from tests import qwen2_5_vl_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "qwen2_5_vl_tiny_ref.npz"))
H = np.load(os.path.join(HERE, "golden", "qwen2_5_vl_tiny_hf.npz"))
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
FEAT_ROWS, EMB_ROWS, LOGIT_ROWS = slice(None, None, 2), slice(None, None, 3), slice(None, None, 7)     # as the script sampled
TABLES = ["g8x8", "g12x20", "g2x2", "g2x4x6", "g10x6", "two", "three"]
CASES = ["one_image", "three_images"]
BF = torch.bfloat16


def _weights(dt):
    W = R.random_weights(R.tiny_cfg(), seed=1234, dtype=torch.float32, std=0.05, embed_std=0.2)
    return {k: v.to(dt) for k, v in W.items()}


def _request(case):
    grids = G[case + ".grids"]
    return R.synth_request(R.tiny_cfg(), [tuple(g) for g in grids.tolist()], seed=len(grids))


def _close(name, got, ref, dt):
    got = got.detach().to(torch.float32).numpy()
    if dt == "f32":
        np.testing.assert_allclose(got, ref, rtol=2e-4, atol=2e-5, err_msg=name)
    else:
        assert np.array_equal(got, ref), (name, int((got != ref).sum()), float(np.abs(got - ref).max()))


# ---------------------------------------------------------------- host tables vs the reference
@pytest.mark.parametrize("name", TABLES)
def test_window_tables_equal_the_references(name):
    """window index, window table (zero-length windows dropped), full-image table, reverse index - of the product's host code
    and of the restatement - equal what the reference's get_window_index / __call__ computed"""
    from mlx_vlm_amd.models.qwen2_5_vl import vision as V

    grids = G[f"tables.{name}.grids"]
    wi, cu_raw = V.get_window_index(grids, 112, 2, 14)
    assert np.array_equal(wi, G[f"tables.{name}.window_index"])
    assert np.array_equal(np.asarray(cu_raw), G[f"tables.{name}.cu_window_raw"])          # padding windows included
    t = V.host_tables(grids, 112, 2, 14)
    assert np.array_equal(t["cu_window"], G[f"tables.{name}.cu_window"])
    assert (np.diff(t["cu_window"]) > 0).all()
    assert np.array_equal(t["cu_full"], G[f"tables.{name}.cu_full"])
    assert np.array_equal(t["reverse_index"], G[f"tables.{name}.reverse_index"])
    assert np.array_equal(t["window_index"][t["reverse_index"]], np.arange(len(wi)))
    # the restatement's own tables
    rwi, rcu = R.get_window_index(R.tiny_cfg(), grids)
    assert np.array_equal(rwi, wi) and np.array_equal(R.unique_first(rcu), G[f"tables.{name}.cu_window"])


def test_expected_window_lengths():
    from mlx_vlm_amd.models.qwen2_5_vl import vision as V

    assert np.diff(V.host_tables([(1, 12, 20)], 112, 2, 14)["cu_window"]).tolist() == [64, 64, 32, 32, 32, 16]
    assert np.diff(V.host_tables([(1, 2, 2)], 112, 2, 14)["cu_window"]).tolist() == [4]
    wi, cu_raw = V.get_window_index([(1, 8, 8)], 112, 2, 14)
    assert cu_raw == [0, 64, 64, 64, 64]                     # an exact multiple: three zero-length padding windows
    assert np.diff(V.host_tables([(1, 8, 8)], 112, 2, 14)["cu_window"]).tolist() == [64]


@pytest.mark.parametrize("name", TABLES)
def test_rotary_rows_in_window_order(name):
    """the product's rotary table is the reference's rot_pos_emb gathered by the window index (vision.py:354-358)"""
    from mlx_vlm_amd.models.qwen2_5_vl import VisionModel, VisionConfig
    from mlx_vlm_amd.models.qwen2_5_vl import vision as V

    grids = G[f"tables.{name}.grids"]
    vm = VisionModel(VisionConfig(depth=2, hidden_size=160, num_heads=2, intermediate_size=172, out_hidden_size=256,
                                  fullatt_block_indexes=[1]), device="cpu")
    plain = vm.rot_pos_emb(grids).numpy()
    np.testing.assert_allclose(plain[::5], G[f"tables.{name}.rot_pos_emb"], rtol=0, atol=0)
    t = V.host_tables(grids, 112, 2, 14)
    want = plain.reshape(-1, 4, plain.shape[1])[t["window_index"]].reshape(plain.shape)
    assert np.array_equal(vm.rot_pos_emb(grids, t["pos"]).numpy(), want)


# ---------------------------------------------------------------- restatement vs the reference (shim goldens)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", CASES)
def test_tower_and_embeddings_vs_reference(case, dt):
    """bf16: the patch contraction agrees to 1 bf16 ulp (Conv3d vs GEMM summation order), and from the reference's own patch
    embeddings on everything is bit-exact; fp32: rtol 2e-4, atol 2e-5"""
    cfg, W = R.tiny_cfg(), _weights(DT[dt])
    ids, pix, thw = _request(case)
    pixt = torch.from_numpy(pix).to(DT[dt])
    p = f"{case}.{dt}."
    start = None
    if dt == "bf16":
        own = R.patch_embed(W, cfg, pixt).to(torch.float32).numpy()
        ref = G[p + "ref_patch_embed"]
        assert np.abs(own - ref).max() <= 2.0 ** -7 * np.abs(ref).max() and (own != ref).mean() < 1e-3
        start = torch.from_numpy(ref).to(BF)
    feats = R.vision_tower(W, cfg, pixt, thw, patch_embeds=start)
    _close("image_features", feats[FEAT_ROWS], G[p + "ref_image_features"], dt)
    from oracle import qwen2_vl as oq

    emb = oq.merge_input_ids_with_image_features(cfg, feats, oq.embed_tokens(W, ids), ids)
    _close("inputs_embeds", emb[0][EMB_ROWS], G[p + "ref_inputs_embeds"], dt)
    pos, deltas = oq.get_rope_index(cfg, ids, thw)
    assert np.array_equal(np.asarray(pos), G[case + ".ref_position_ids"])
    assert np.array_equal(np.asarray(deltas).reshape(-1), G[case + ".ref_rope_deltas"])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", CASES)
def test_prefill_and_greedy_vs_reference(case, dt, monkeypatch):
    cfg, W = R.tiny_cfg(), _weights(DT[dt])
    ids, pix, thw = _request(case)
    pixt = torch.from_numpy(pix)
    p = f"{case}.{dt}."
    if dt == "bf16":      # continue from the reference's patch embeddings (see above)
        start = torch.from_numpy(G[p + "ref_patch_embed"]).to(BF)
        tower = R.vision_tower
        monkeypatch.setattr(R, "vision_tower", lambda W_, c_, px, g, **kw: tower(W_, c_, px, g, patch_embeds=start))
    # rope_mode="fallback": the pure-MLX rope path, which is what the reference runs over the shim
    logits = R.prefill_logits(W, cfg, ids, pixt, thw, rope_mode="fallback")
    _close("prefill rows", logits[LOGIT_ROWS], G[p + "ref_prefill_logits"], dt)
    _close("prefill last", logits[-1], G[p + "ref_prefill_last"], dt)
    toks, rows = R.generate_greedy(W, cfg, ids, pixt, thw, max_tokens=9, return_logits=True, rope_mode="fallback")
    assert toks[:8] == G[p + "ref_greedy"].tolist()
    _close("decode logits", rows[1:9], G[p + "ref_decode_logits"], dt)


# ---------------------------------------------------------------- restatement vs transformers
@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_hf(case):
    """fp32 restatement vs Qwen2_5_VLForConditionalGeneration: tower features, position ids, prompt logits at atol 1e-4"""
    cfg, W = R.tiny_cfg(), _weights(torch.float32)
    ids, pix, thw = _request(case)
    pixt = torch.from_numpy(pix)
    np.testing.assert_allclose(R.vision_tower(W, cfg, pixt, thw).numpy(), H[case + ".hf_image_features"], rtol=0, atol=1e-4)
    from oracle import qwen2_vl as oq

    pos, deltas = oq.get_rope_index(cfg, ids, thw)
    assert np.array_equal(np.asarray(pos), H[case + ".hf_position_ids"])
    assert np.array_equal(np.asarray(deltas).reshape(-1), H[case + ".hf_rope_deltas"].reshape(-1))
    logits = R.prefill_logits(W, cfg, ids, pixt, thw).numpy()
    np.testing.assert_allclose(logits[::3], H[case + ".hf_logits"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(logits[-1], H[case + ".hf_logits_last"], rtol=0, atol=1e-4)


# ---------------------------------------------------------------- host logic of the family
def test_config_parsing():
    from mlx_vlm_amd.models.qwen2_5_vl import ModelConfig, VisionConfig

    v = VisionConfig()
    assert (v.hidden_size, v.intermediate_size, v.window_size, v.patch_size, v.tokens_per_second) == (1280, 3420, 112, 14, 2)
    assert v.fullatt_block_indexes == [7, 15, 23, 31] and v.fullatt_block_indexes is not VisionConfig().fullatt_block_indexes
    d = R.model_config_dict(R.tiny_cfg())
    d.pop("tie_word_embeddings")
    d["unknown_key"] = 1
    mc = ModelConfig.from_dict(d)
    assert mc.model_type == "qwen2_5_vl" and mc.text_config.tie_word_embeddings is True
    assert mc.text_config.num_key_value_heads == 1 and mc.text_config.hidden_size == 256
    assert mc.vision_config.out_hidden_size == 256 and mc.vision_config.fullatt_block_indexes == [1]
    with pytest.raises(ValueError, match="rope_scaling"):
        ModelConfig.from_dict(dict(d, rope_scaling={"type": "mrope"}))


def test_family_is_found_by_name_and_processor_route():
    from mlx_vlm_amd import utils
    from mlx_vlm_amd.models.qwen2_5_vl.processing_qwen2_5_vl import Qwen2_5_VLProcessor

    arch, mt = utils.get_model_and_args({"model_type": "qwen2_5_vl"})
    assert mt == "qwen2_5_vl" and arch.Model.__module__.endswith("qwen2_5_vl.qwen2_5_vl")
    from mlx_vlm_amd.models.qwen2_vl import LanguageModel as Base

    assert arch.LanguageModel is Base                       # the shared language model: kv_bits, max_kv_size, prompt_cache live there

    class Tok:
        def __call__(self, text, **kw):
            return {"input_ids": [[7 if c == "I" else 3 for c in t.replace("<|image_pad|>", "I")] for t in text]}

        def convert_tokens_to_ids(self, t):
            return {"<|image_pad|>": 7, "<|video_pad|>": 8}[t]

    class IP:
        merge_size = 2

        def __call__(self, images):
            return {"pixel_values": np.zeros((16, 4), np.float32), "image_grid_thw": np.array([[1, 4, 4]])}

    out = Qwen2_5_VLProcessor(IP(), Tok())(images=[object()], text="a<|image_pad|>b", return_mm_token_type_ids=True)
    assert out["input_ids"].tolist() == [[3, 7, 7, 7, 7, 3]] and out["mm_token_type_ids"] == [[0, 1, 1, 1, 1, 0]]
    with pytest.raises(NotImplementedError, match="Qwen2-VL"):
        utils.load_processor("/nonexistent", type("C", (), {"model_type": "qwen2_5_vl"})(), image_preprocess="device")


def test_message_format_puts_the_images_first():
    """the reference's prompt_utils gives qwen2_5_vl LIST_WITH_IMAGE_FIRST (46), where qwen2_vl has the text item first"""
    from mlx_vlm_amd import prompt_utils as pu

    msg = pu.get_message_json("qwen2_5_vl", "hi", num_images=2)
    assert msg == {"role": "user", "content": [{"type": "image"}, {"type": "image"}, {"type": "text", "text": "hi", "content": "hi"}]}
    assert [c["type"] for c in pu.get_message_json("qwen2_vl", "hi", num_images=2)["content"]] == ["text", "image", "image"]
    assert pu.get_message_json("qwen2_5_vl", "hi", role="assistant", num_images=2)["content"] == [
        {"type": "text", "text": "hi", "content": "hi"}]


def test_sanitize_vs_reference():
    from mlx_vlm_amd.models.qwen2_5_vl import Model, ModelConfig

    m = Model(ModelConfig.from_dict(R.model_config_dict(R.tiny_cfg())), device="cpu", kv_pool_tokens=1024, max_seqs=2)
    keys = list(G["sanitize.hf_keys"])
    w = {k: (torch.from_numpy(G["sanitize.hf_conv"]) if k.endswith("patch_embed.proj.weight") else torch.zeros(3)) for k in keys}
    w["visual.blocks.0.attn.position_ids"] = torch.zeros(1)
    out = m.sanitize(w)
    vt = m.vision_tower.sanitize({k: v for k, v in out.items() if k.startswith("vision_tower.")})
    got = [k for k in out if not k.startswith("vision_tower.")] + list(vt)
    assert sorted(got) == sorted(G["sanitize.ref_keys"].tolist())
    assert np.array_equal(vt["vision_tower.patch_embed.proj.weight"].numpy(), G["sanitize.ref_conv"])
    # the transformers >= 4.5x layout
    out2 = m.sanitize({"model.visual.merger.ln_q.weight": torch.zeros(1), "model.language_model.norm.weight": torch.zeros(1)})
    assert sorted(out2) == ["language_model.model.norm.weight", "vision_tower.merger.ln_q.weight"]


@pytest.mark.parametrize("inter,padded", [(172, 192), (3420, 3456)])
def test_mlp_zero_padding(inter, padded):
    """gate / up rows and biases and down's columns padded to a multiple of 64, interleaved; the padded units are exactly zero
    and the padded MLP computes what the unpadded one does"""
    from mlx_vlm_amd.models.qwen2_5_vl.vision import pad_mlp
    from oracle import ops as O

    g = torch.Generator().manual_seed(inter)
    E = 160
    wg, wu = (torch.randn(inter, E, generator=g) * 0.05).to(BF), (torch.randn(inter, E, generator=g) * 0.05).to(BF)
    bg, bu = (torch.randn(inter, generator=g) * 0.05).to(BF), (torch.randn(inter, generator=g) * 0.05).to(BF)
    wd = (torch.randn(E, inter, generator=g) * 0.05).to(BF)
    wgu, bgu, wdp, ip = pad_mlp(wg, bg, wu, bu, wd)
    assert ip == padded and wgu.shape == (2 * padded, E) and bgu.shape == (2 * padded,) and wdp.shape == (E, padded)
    assert torch.equal(wgu[0:2 * inter:2], wg) and torch.equal(wgu[1:2 * inter:2], wu)
    assert torch.equal(bgu[0:2 * inter:2], bg) and torch.equal(bgu[1:2 * inter:2], bu) and torch.equal(wdp[:, :inter], wd)
    assert not wgu[2 * inter:].any() and not bgu[2 * inter:].any() and not wdp[:, inter:].any()
    x = (torch.randn(5, E, generator=g)).to(BF)
    act = O.swiglu(O.linear(x, wgu[0::2], bgu[0::2]), O.linear(x, wgu[1::2], bgu[1::2]))
    assert not act[:, inter:].any()                                          # silu(0) * 0
    assert torch.equal(act[:, :inter], O.swiglu(O.linear(x, wg, bg), O.linear(x, wu, bu)))
    assert torch.equal(O.linear(act, wdp), O.linear(act[:, :inter], wd))


def test_model_builds_on_the_host_and_refuses_other_head_dims():
    from mlx_vlm_amd.models.qwen2_5_vl import Model, ModelConfig

    cfg = R.tiny_cfg()
    m = Model(ModelConfig.from_dict(R.model_config_dict(cfg)), device="cpu", kv_pool_tokens=1024, max_seqs=2)
    vt = m.vision_tower
    assert (vt.head_dim, vt.mlp_hidden, vt.patch_k, vt.fullatt_block_indexes) == (80, 192, 1216, [1])
    real = Model(ModelConfig.from_dict(R.model_config_dict(R.real_width_cfg())), device="cpu", kv_pool_tokens=1024, max_seqs=2)
    assert (real.vision_tower.head_dim, real.vision_tower.mlp_hidden) == (80, 3456)
    bad = R.tiny_cfg(hidden_size=128)                                         # 2 heads of 64
    W = R.random_weights(bad, seed=1, tower_only=True)
    mb = Model(ModelConfig.from_dict(R.model_config_dict(bad)), device="cpu", kv_pool_tokens=1024, max_seqs=2)
    with pytest.raises(NotImplementedError, match="head_dim"):
        mb.vision_tower.load_weights({k[len("vision_tower."):]: v for k, v in W.items()})


def test_one_tile_knob(monkeypatch):
    """window blocks take the one-tile kernel only when every window fits it; VLM_VIT_WINDOW_ATTN forces either route"""
    from mlx_vlm_amd.models.qwen2_5_vl import VisionConfig, VisionModel
    from mlx_vlm_amd.models.qwen2_5_vl import vision as V

    vm = VisionModel(VisionConfig(depth=2, hidden_size=160, num_heads=2, intermediate_size=172, out_hidden_size=256,
                                  fullatt_block_indexes=[1]), device="cpu")
    monkeypatch.setenv("VLM_VIT_WINDOW_ATTN", "1")
    assert vm.one_tile(64) and not vm.one_tile(65)
    monkeypatch.setenv("VLM_VIT_WINDOW_ATTN", "0")
    assert not vm.one_tile(64)
    monkeypatch.delenv("VLM_VIT_WINDOW_ATTN")
    assert vm.one_tile(64) == V.ONE_TILE_DEFAULT
    # a 224-pixel window is 256 tokens: the general kernel, whatever the knob says
    assert int(np.diff(V.host_tables([(1, 16, 16)], 224, 2, 14)["cu_window"]).max()) == 256


def test_abi_still_60_names_version_8():
    root = os.path.dirname(HERE)
    hdr = open(os.path.join(root, "include", "vlm_hip.h")).read()
    assert len(set(re.findall(r"\b(vlm_[a-z0-9_]+)\s*\(", hdr))) == 60
    from mlx_vlm_amd import _lib

    assert len(_lib.SIGNATURES) == 60
