"""InternVL3 / 3.5 on the host: the torch restatement (tests/internvl_ref.py) against vectors recorded from the REFERENCE'S files
over oracle/mlx_shim (tests/golden/make_golden_ref_internvl.py: bit-exact in bf16 and fp32) and against transformers'
InternVLForConditionalGeneration (fp32 at 1e-4, run here), the processor against values recorded from the reference's
`dynamic_preprocess` / `build_transform`, and the family's host logic (pixel-shuffle table, CLS / position assembly, sanitize, the
refusals, the C ABI's size).  CPU only; of the reference only the recorded files are read."""
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle import ops as O
from tests import internvl_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "internvl_tiny_ref.npz"))
TILING = json.load(open(os.path.join(HERE, "golden", "internvl_tiling_ref.json")))
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
ROWS3, ROWS7 = slice(None, None, 3), slice(None, None, 7)          # as the script sampled
CASES = {"one_tile": [1], "three_tiles": [3], "text_only": []}
BF = torch.bfloat16


def _weights(lm, dt):
    return {k: v.to(dt) for k, v in R.random_weights(R.tiny_cfg(lm), seed=1234, dtype=torch.float32).items()}


def _request(cfg, case):
    tiles = CASES[case]
    return R.synth_request(cfg, tiles, n_text=12 if tiles else 19, seed=len(tiles) + sum(tiles))


def _exact(name, got, ref):
    got = got.detach().to(torch.float32).numpy()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.array_equal(got, ref), (name, int((got != ref).sum()), float(np.abs(got - ref).max()))


# ---------------------------------------------------------------- restatement vs the reference (shim goldens), bit for bit
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", ["one_tile", "three_tiles"])
def test_tower_and_connector_restatement_is_the_reference_bit_for_bit(case, dt):
    cfg, W = R.tiny_cfg("qwen2"), _weights("qwen2", DT[dt])
    ids, pix = _request(cfg, case)
    p = f"qwen2.{case}.{dt}."
    x = torch.from_numpy(pix).to(DT[dt])
    E = cfg.vision.hidden_size
    emb = R.vision_embeddings(W, cfg, x)
    _exact("embeddings", emb.reshape(-1, E)[ROWS3], G[p + "ref_vision_embeddings"])
    last = R.vision_tower(W, cfg, x)
    assert last.shape == (len(pix), 17, E)
    _exact("last state", last.reshape(-1, E)[ROWS3], G[p + "ref_vision_last"])
    feats = R.image_features(W, cfg, torch.from_numpy(pix))
    assert feats.shape == (len(pix) * 4, cfg.text.hidden_size)
    _exact("image features", feats, G[p + "ref_image_features"])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("lm", ["qwen2", "qwen3"])
def test_model_restatement_is_the_reference_bit_for_bit(lm, case, dt):
    """merged embeddings, prefill logits and 8 greedy steps on the cache, both language-model forms"""
    cfg, W = R.tiny_cfg(lm), _weights(lm, DT[dt])
    ids, pix = _request(cfg, case)
    pixt = torch.from_numpy(pix) if pix is not None else None
    p = f"{lm}.{case}.{dt}."
    emb = R.get_input_embeddings(W, cfg, ids, pixt)
    _exact("inputs_embeds", emb[0][ROWS3], G[p + "ref_inputs_embeds"])
    logits = R.language_model(W, cfg, emb)[0]
    _exact("prefill rows", logits[ROWS7], G[p + "ref_prefill_logits"])
    _exact("prefill last", logits[-1], G[p + "ref_prefill_last"])
    toks, rows = R.generate_greedy(W, cfg, ids, pixt, max_tokens=9, return_logits=True)
    assert toks[:8] == G[p + "ref_greedy"].tolist()
    _exact("decode logits", rows[1:9], G[p + "ref_decode_logits"])


def test_layer_scale_and_gelu_form_are_visible():
    """not vacuous: with ls = 1 (the feature absent) or the erf GELU in the MLP the tower is far from / measurably off the
    reference's vectors, and the GPU tests' 2e-2 bar sees a missing layer scale"""
    cfg, W = R.tiny_cfg("qwen2"), _weights("qwen2", BF)
    _, pix = _request(cfg, "one_tile")
    x = torch.from_numpy(pix).to(BF)
    ref = R.vision_tower(W, cfg, x).float()
    rel = lambda a: float((a.float() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())   # noqa: E731
    W1 = {k: (torch.ones_like(v) if k.endswith((".ls1", ".ls2")) else v) for k, v in W.items()}
    assert rel(R.vision_tower(W1, cfg, x)) > 0.1
    assert 0 < rel(R.vision_tower(W, cfg, x, act="erf")) < 2e-2
    assert 0 <= rel(R.vision_tower(W, cfg, x, conv=False)) < 1e-2                 # the GEMM form of the patch convolution


def test_layerscale_epilogue_restatement_and_lattice():
    """the three roundings of the epilogue are the encoder layer's (x + ls * Linear(.)), and on the lattice operands of the GPU test
    the fp32 restatement is EXACT: equal to the float64 accumulation and to any re-ordering of the K sum"""
    g = torch.Generator().manual_seed(3)
    a, w = (torch.randn(9, 64, generator=g) * 0.5).to(BF), (torch.randn(16, 64, generator=g) * 0.2).to(BF)
    b, ls, res = (torch.randn(16, generator=g) * 0.1).to(BF), (0.05 + 0.45 * torch.rand(16, generator=g)).to(BF), torch.randn(9, 16, generator=g).to(BF)
    want = O.add(res, R.mul(O.linear(a, w, b), ls))
    assert torch.equal(R.layerscale_epilogue(a, w, b, ls, res), want)
    assert not torch.equal(want, O.add(res, O.linear(a, (w.float() * ls.float()[:, None]).to(BF), R.mul(b, ls))))   # folding ls changes bits
    for (M, N, K) in ((37, 24, 4096), (130, 64, 320)):
        a, w, b, ls, res = R.lattice_operands(M, N, K, seed=K)
        r32, r64 = R.layerscale_epilogue(a, w, b, ls, res), R.layerscale_epilogue(a, w, b, ls, res, torch.float64)
        assert torch.equal(r32, r64)
        perm = torch.randperm(K, generator=g)
        halves = (a[:, perm[: K // 3]].float() @ w[:, perm[: K // 3]].float().T) + (a[:, perm[K // 3:]].float() @ w[:, perm[K // 3:]].float().T)
        y = (halves + b.float()).to(BF)
        assert torch.equal(O.add(res, R.mul(y, ls)), r32)
        assert float(r32.float().abs().max()) > 16 and len(torch.unique(r32)) > 20          # not a degenerate result
    ones = torch.ones_like(ls)
    assert torch.equal(R.layerscale_epilogue(a, w, b, ones, res), O.add(res, O.linear(a, w, b)))     # x * 1.0 is exact


# ---------------------------------------------------------------- restatement vs transformers
def _hf_model(cfg, W, act):
    tr = pytest.importorskip("transformers")
    if not hasattr(tr, "InternVLForConditionalGeneration"):
        pytest.skip("transformers without InternVL")
    t, v = cfg.text, cfg.vision
    vc = dict(hidden_size=v.hidden_size, num_hidden_layers=v.num_hidden_layers, num_attention_heads=v.num_attention_heads,
              intermediate_size=v.intermediate_size, image_size=[v.image_size] * 2, patch_size=[v.patch_size] * 2, attention_bias=True,
              use_qk_norm=False, hidden_act={"tanh": "gelu_pytorch_tanh", "erf": "gelu"}[act], norm_type="layer_norm",
              layer_norm_eps=v.layer_norm_eps, use_mean_pooling=True)
    tc = dict(model_type=t.model_type, hidden_size=t.hidden_size, num_hidden_layers=t.num_hidden_layers,
              intermediate_size=t.intermediate_size, num_attention_heads=t.num_attention_heads,
              num_key_value_heads=t.num_key_value_heads, vocab_size=t.vocab_size, rms_norm_eps=t.rms_norm_eps, rope_theta=t.rope_theta,
              tie_word_embeddings=False, attention_bias=t.attention_bias)
    if t.head_dim:
        tc["head_dim"] = t.head_dim
    hc = tr.InternVLConfig(vision_config=vc, text_config=tc, image_token_id=cfg.image_token_index, downsample_ratio=cfg.downsample_ratio,
                           projector_hidden_act="gelu", vision_feature_layer=-1, vision_feature_select_strategy="default",
                           tie_word_embeddings=False)
    hc._attn_implementation = "eager"
    model = tr.InternVLForConditionalGeneration(hc).eval().to(torch.float32)
    # the weight-name map: checkpoint (reference) name -> transformers name
    sd = {}
    for k, w in W.items():
        if k.startswith("vision_model.embeddings."):
            n = k.rsplit("embeddings.", 1)[1]
            n = {"class_embedding": "cls_token", "position_embedding": "position_embeddings",
                 "patch_embedding.weight": "patch_embeddings.projection.weight", "patch_embedding.bias": "patch_embeddings.projection.bias"}[n]
            sd["model.vision_tower.embeddings." + n] = w.permute(0, 3, 1, 2) if n.endswith("projection.weight") else w
        elif k.startswith("vision_model.encoder.layers."):
            i, n = k[len("vision_model.encoder.layers."):].split(".", 1)
            pre = f"model.vision_tower.encoder.layer.{i}."
            if n.startswith("attn.qkv."):
                for j, q in enumerate(("q_proj", "k_proj", "v_proj")):
                    sd[pre + f"attention.{q}." + n.rsplit(".", 1)[1]] = w.chunk(3, dim=0)[j]
            else:
                n = n.replace("attn.proj.", "attention.projection_layer.").replace("norm1.", "layernorm_before.")
                n = n.replace("norm2.", "layernorm_after.").replace("ls1", "lambda_1").replace("ls2", "lambda_2")
                sd[pre + n] = w
        elif k.startswith("mlp1."):
            i, n = k[len("mlp1."):].split(".")
            sd["model.multi_modal_projector." + {"0": "layer_norm", "1": "linear_1", "3": "linear_2"}[i] + "." + n] = w
        elif k.startswith("language_model.model."):
            sd["model.language_model." + k[len("language_model.model."):]] = w
        else:
            sd["lm_head.weight"] = w
    missing, unexpected = model.load_state_dict({k: v.contiguous() for k, v in sd.items()}, strict=False)
    assert not unexpected and all("rotary" in m or "inv_freq" in m for m in missing), (missing, unexpected)
    return model


@pytest.mark.parametrize("act", ["tanh", "erf"])
@pytest.mark.parametrize("lm", ["qwen2", "qwen3"])
def test_restatement_matches_hf(lm, act):
    """fp32 restatement vs InternVLForConditionalGeneration at atol 1e-4: image features (tower with layer scale + pixel shuffle +
    projector) and the logits of every prompt row.  transformers' activation is configurable: `gelu_pytorch_tanh` is the
    reference's graph (act="tanh"), `gelu` the original InternViT's (act="erf"); the restatement follows either."""
    cfg, W = R.tiny_cfg(lm), _weights(lm, torch.float32)
    model = _hf_model(cfg, W, act)
    ids, pix = _request(cfg, "three_tiles")
    with torch.no_grad():
        hf_feats = model.model.get_image_features(pixel_values=torch.from_numpy(pix)).pooler_output
        hf_logits = model(input_ids=torch.from_numpy(ids), pixel_values=torch.from_numpy(pix)).logits[0]
    feats = R.image_features(W, cfg, torch.from_numpy(pix), act=act)
    np.testing.assert_allclose(feats.numpy(), hf_feats.reshape(feats.shape).numpy(), rtol=0, atol=1e-4)
    logits = R.prefill_logits(W, cfg, ids, torch.from_numpy(pix), act=act)
    np.testing.assert_allclose(logits.numpy(), hf_logits.numpy(), rtol=0, atol=1e-4)


# ---------------------------------------------------------------- 1-D RoPE as M-RoPE, position table at the native size
@pytest.mark.parametrize("lm", ["qwen2", "qwen3"])
def test_plain_rope_is_mrope_with_one_position_on_all_axes(lm):
    """the engine rotates with M-RoPE: with the same position on the three axes the chunked selector (Qwen2 form) and the
    interleaved one (Qwen3 form, VLM_MODE_QWEN3) both give nn.RoPE's rotation bit for bit"""
    cfg, W = R.tiny_cfg(lm), _weights(lm, BF)
    ids, pix = _request(cfg, "one_tile")
    emb = R.get_input_embeddings(W, cfg, ids, torch.from_numpy(pix))
    plain = R.language_model(W, cfg, emb)
    half = cfg.text.hd // 2
    for sel in (O.chunked_position_selector([half // 4, 3 * half // 8, 3 * half // 8], half),
                R.interleaved_position_selector([24, 20, 20] if half == 64 else [half // 2, half // 4, half // 4], half)):
        assert len(set(sel.tolist())) == 3
        assert torch.equal(R.language_model(W, cfg, emb, selector=sel), plain)


def test_position_interpolation_is_the_identity_at_the_native_tile():
    """`interpolate` (bicubic, align_corners=False) onto the table's own grid samples at the integer positions with cubic weights
    (0, 1, 0, 0): the table comes back unchanged, so the tower adds the learned rows as they are"""
    g = torch.Generator().manual_seed(0)
    for S in (4, 32):
        t = torch.randn(1, 8, S, S, generator=g)
        assert torch.equal(torch.nn.functional.interpolate(t, size=(S, S), mode="bicubic", align_corners=False), t)


# ---------------------------------------------------------------- processor
def test_tile_plans_match_the_reference():
    from mlx_vlm_amd.models.internvl_chat.processor import dynamic_preprocess, tile_plan

    from PIL import Image

    kinds = set()
    for c in TILING:
        grid, boxes, thumb = tile_plan(c["width"], c["height"], c["min_num"], c["max_num"], 448, c["use_thumbnail"])
        assert [grid[0] * 448, grid[1] * 448] == c["resized_to"], c
        assert [list(b) for b in boxes] == c["boxes"], c
        assert thumb == c["thumbnail"] and len(boxes) + int(thumb) == c["n_tiles"], c
        tiles = dynamic_preprocess(Image.new("RGB", (c["width"], c["height"])), c["min_num"], c["max_num"], 448, c["use_thumbnail"])
        assert len(tiles) == c["n_tiles"] and {t.size for t in tiles} == {(448, 448)}
        kinds.add((len(boxes) == c["max_num"], thumb, c["use_thumbnail"]))
    assert {(True, True, True), (False, False, True), (False, False, False), (False, True, True)} <= kinds     # max_num hit; thumbnail on / off


def test_pixel_values_match_the_reference_transform():
    from PIL import Image

    from mlx_vlm_amd.models.internvl_chat.processor import InternVLImageProcessor, transform

    img = Image.fromarray(G["processor.image_hwc"])
    assert np.array_equal(transform(img, 56), G["processor.transform_56"])
    out = InternVLImageProcessor(size=56, dynamic_max_num=4, dynamic_use_thumbnail=True).preprocess([img])
    assert out["pixel_values"].dtype == np.float32 and np.array_equal(out["pixel_values"], G["processor.pixel_values"])
    assert out["num_patches_list"] == G["processor.num_patches_list"].tolist() == [3]
    assert np.array_equal(InternVLImageProcessor(size=56, dynamic_max_num=4)(G["processor.image_hwc"])["pixel_values"], G["processor.pixel_values"])


class _Tok:
    """whitespace tokenizer over a growing vocabulary; the three image markers are split off as tokens of their own"""
    chat_template = None
    eos_token_id = 1

    def __init__(self):
        self.vocab = {"<pad>": 0, "<IMG_CONTEXT>": 1001, "<img>": 1003, "</img>": 1004}
        self.padding_side = "right"

    def convert_tokens_to_ids(self, t):
        return self.vocab[t]

    def __call__(self, texts, padding=True, **kw):
        rows = []
        for t in texts:
            for m in ("<IMG_CONTEXT>", "<img>", "</img>"):
                t = t.replace(m, f" {m} ")
            rows.append([self.vocab.setdefault(w, len(self.vocab) + 2000) for w in t.split()])
        L = max(len(r) for r in rows)
        pad = lambda r: [0] * (L - len(r)) + r if self.padding_side == "left" else r + [0] * (L - len(r))   # noqa: E731
        return {"input_ids": [pad(r) for r in rows], "attention_mask": [[int(x != 0) for x in pad(r)] for r in rows]}


def test_prompt_expansion_counts():
    from mlx_vlm_amd.models.internvl_chat.processor import InternVLChatProcessor, InternVLImageProcessor

    proc = InternVLChatProcessor(InternVLImageProcessor(size=56, dynamic_max_num=4), _Tok(), image_size=56, patch_size=14)
    assert proc.num_image_token == 4 and proc.img_context_token_id == 1001
    assert InternVLChatProcessor(tokenizer=_Tok()).num_image_token == 256
    wide, square = np.zeros((50, 100, 3), np.uint8), np.zeros((60, 60, 3), np.uint8)
    out = proc(text="<image>\nwhat is this", images=[wide])
    ids = out["input_ids"]
    assert out["pixel_values"].shape == (3, 3, 56, 56) and out["image_token_index"] == 1001
    assert int((ids == 1001).sum()) == 4 * 3 and int((ids == 1003).sum()) == int((ids == 1004).sum()) == 1
    # two images, one placeholder in the text: the missing one goes in front; tiles 3 and 1
    out = proc(text="compare <image> now", images=[wide, square])
    ids = out["input_ids"][0].tolist()
    assert out["pixel_values"].shape[0] == 4 and ids.count(1001) == 16 and ids.count(1003) == 2
    first = ids.index(1003)
    assert ids[first + 1:first + 13] == [1001] * 12 and ids[first + 13] == 1004          # the 3-tile image takes the FIRST marker
    # one prompt per image; the shorter one is padded on the left
    out = proc(text=["a <image> b c d", "e"], images=[square, wide])
    assert out["input_ids"].shape[0] == 2 and out["attention_mask"][0, 0] == 0 and out["attention_mask"][1, 0] == 1
    assert [int((r == 1001).sum()) for r in out["input_ids"]] == [4, 12]
    assert "pixel_values" not in proc(text="no image")
    with pytest.raises(NotImplementedError, match="video"):
        proc(text="x", videos=[1])


def test_processor_reads_the_checkpoints_tiling_keys(tmp_path):
    from mlx_vlm_amd.models.internvl_chat.processor import InternVLChatProcessor

    (tmp_path / "config.json").write_text(json.dumps(dict(force_image_size=56, max_dynamic_patch=6, min_dynamic_patch=2, use_thumbnail=False,
                                                          downsample_ratio=0.5, vision_config=dict(image_size=448, patch_size=[14, 14]))))
    p = InternVLChatProcessor.from_pretrained(str(tmp_path), tokenizer=_Tok())
    ip = p.image_processor
    assert (ip.size, ip.dynamic_max_num, ip.dynamic_min_num, ip.dynamic_use_thumbnail, p.num_image_token) == (56, 6, 2, False, 4)
    (tmp_path / "processor_config.json").write_text(json.dumps(dict(num_image_token=7, image_size=28)))
    p = InternVLChatProcessor.from_pretrained(str(tmp_path), tokenizer=_Tok())
    assert p.image_processor.size == 28 and p.num_image_token == 7


def test_message_format_is_the_references():
    from mlx_vlm_amd.prompt_utils import apply_chat_template, get_message_json

    m = get_message_json("internvl_chat", "hi", num_images=2)
    assert m == {"role": "user", "content": [{"type": "image"}, {"type": "image"}, {"type": "text", "text": "hi", "content": "hi"}]}
    assert get_message_json("internvl_chat", "ok", role="assistant", num_images=2) == {"role": "assistant", "content": "ok"}
    assert get_message_json("internvl_chat", "s", role="system") == {"role": "system", "content": [{"type": "text", "text": "s", "content": "s"}]}
    msgs = apply_chat_template(None, {"model_type": "internvl_chat"}, "describe", return_messages=True, num_images=1)
    assert msgs[0]["content"][0] == {"type": "image"}


# ---------------------------------------------------------------- host logic
def test_pixel_shuffle_table():
    from mlx_vlm_amd.models.internvl_chat import pixel_shuffle_index

    for P, r in ((16, 0.5), (1024, 0.5), (64, 0.25)):
        idx = pixel_shuffle_index(P, r)
        assert idx.dtype == np.int32 and np.array_equal(idx, G[f"pixel_shuffle.{P}.{r}"])
        # ... and as a row gather it IS base.pixel_shuffle, for any channel count
        x = torch.arange(2 * P * 6, dtype=torch.float32).reshape(2, P, 6)
        want = R.pixel_shuffle(x, r)
        got = x[:, torch.from_numpy(idx.astype(np.int64)).reshape(-1)].reshape(2, idx.shape[0], -1)
        assert torch.equal(got, want)
    assert pixel_shuffle_index(16, 0.5).tolist() == [[0, 1, 4, 5], [2, 3, 6, 7], [8, 9, 12, 13], [10, 11, 14, 15]]
    with pytest.raises(NotImplementedError):
        pixel_shuffle_index(15, 0.5)


def _host_model(lm="qwen2", **over):
    from mlx_vlm_amd.models.internvl_chat import Model, ModelConfig

    d = R.model_config_dict(R.tiny_cfg(lm))
    for k, v in over.items():
        sect, key = k.split("__")
        d[sect][key] = v
    return Model(ModelConfig.from_dict(d), device="cpu", kv_pool_tokens=1024, max_seqs=2)


def test_cls_and_position_assembly_on_the_host():
    """the tower's load step on the CPU: CLS row = T(class_embedding + position_embedding[0]) once, the patch rows' residual
    operand = position rows 1.., the layer-scale rows stacked behind the biases, the gather table of n tiles"""
    cfg, W = R.tiny_cfg("qwen2"), _weights("qwen2", BF)
    m = _host_model()
    vt = m.vision_model
    vt.load_weights({k[len("vision_model."):]: v for k, v in W.items() if k.startswith("vision_model.")})
    emb = R.vision_embeddings(W, cfg, torch.zeros(1, 3, 56, 56, dtype=BF))
    assert torch.equal(vt._w["cls_row"][0], emb[0, 0])
    assert torch.equal(vt._w["pos"], W["vision_model.embeddings.position_embedding"][0, 1:])
    assert vt._w["wpatch"].shape == (128, 640) and not vt._w["wpatch"][:, 588:].any()
    bo, b2 = vt._w["1.bo"], vt._w["1.b2"]
    assert bo.shape == b2.shape == (2, 128) and bo.is_contiguous()
    assert torch.equal(bo[0], W["vision_model.encoder.layers.1.attn.proj.bias"]) and torch.equal(bo[1], W["vision_model.encoder.layers.1.ls1"])
    assert torch.equal(b2[1], W["vision_model.encoder.layers.1.ls2"])
    assert m.tokens_per_tile == 4 and m.shuffle_index.shape == (4, 4)
    rows = (np.arange(3)[:, None, None] * 17 + 1 + m.shuffle_index[None]).reshape(-1)
    assert rows.min() == 1 and rows.max() == 50 and 17 not in rows and 34 not in rows        # every CLS row is skipped
    with pytest.raises(NotImplementedError, match="native"):
        vt.embeddings(torch.zeros(1, 3, 28, 28))


def test_sanitize():
    m = _host_model()
    conv = torch.from_numpy(G["sanitize.hf_conv"])
    out = m.vision_model.sanitize({"embeddings.patch_embedding.weight": conv, "embeddings.position_ids": torch.zeros(3),
                                   "encoder.layers.0.ls1": torch.ones(4)})
    assert list(out) == G["sanitize.ref_keys"].tolist()
    assert np.array_equal(out["embeddings.patch_embedding.weight"].numpy(), G["sanitize.ref_conv"])
    again = m.vision_model.sanitize(out)
    assert torch.equal(again["embeddings.patch_embedding.weight"], out["embeddings.patch_embedding.weight"])     # already (O, kH, kW, C)
    W = _weights("qwen2", BF)
    hf = R.to_hf_keys(W)
    hf["language_model.model.layers.0.self_attn.rotary_emb.inv_freq"] = torch.zeros(4)
    san = m.sanitize(hf)
    assert set(san) == set(W) and all(torch.equal(san[k], W[k]) for k in W)


def test_config_mirrors_the_reference():
    from mlx_vlm_amd.models.internvl_chat import ModelConfig, VisionConfig

    v = VisionConfig.from_dict(dict(model_type="intern_vit_6b", image_size=[448, 448], patch_size=[14], unknown=1))
    assert (v.image_size, v.patch_size, v.hidden_size, v.qk_normalization, v.norm_type) == (448, 14, 1024, False, "layer_norm")
    c = ModelConfig.from_dict(R.model_config_dict(R.tiny_cfg("qwen3")))
    assert c.text_config.head_dim == 128 and c.text_config.attention_bias is False and c.downsample_ratio == 0.5
    assert c.image_token_index == 1001 and ModelConfig(text_config=None, vision_config=None, model_type="internvl_chat").image_token_index == 151667


def test_load_dispatches_on_model_type():
    from mlx_vlm_amd import utils

    arch, mt = utils.get_model_and_args({"model_type": "internvl_chat"})
    assert mt == "internvl_chat" and arch.__name__.endswith("models.internvl_chat") and hasattr(arch, "Model") and hasattr(arch, "ModelConfig")


def test_refusals():
    from mlx_vlm_amd import utils

    with pytest.raises(NotImplementedError, match="InternViT-6B"):
        _host_model(vision_config__qk_normalization=True)
    with pytest.raises(NotImplementedError, match="InternViT-6B"):
        _host_model(vision_config__norm_type="rms_norm")
    for mt in ("internlm2", "internlm3", "gpt_oss", "qwen3_moe", "llama"):
        with pytest.raises(NotImplementedError, match=mt):
            _host_model(text_config__model_type=mt)
    with pytest.raises(NotImplementedError, match="attention_bias"):
        _host_model(text_config__attention_bias=False)
    with pytest.raises(NotImplementedError, match="head_dim"):
        _host_model("qwen3", text_config__head_dim=64)
    m = _host_model()
    with pytest.raises(NotImplementedError, match="4-bit attention projections with head_dim 64"):
        m.language_model.load_weights({"model.layers.0.self_attn.q_proj.scales": torch.zeros(1)})
    with pytest.raises(NotImplementedError, match="video"):
        m.get_input_embeddings(np.zeros((1, 4), dtype=np.int64), None, video_grid_thw=np.array([[2, 4, 4]]))
    with pytest.raises(NotImplementedError, match="image_preprocess='device'"):
        utils.load_processor("/nonexistent", m.config, image_preprocess="device")


def test_convert_and_apc_refuse_the_family(tmp_path):
    from mlx_vlm_amd import convert

    src = tmp_path / "src"
    src.mkdir()
    (src / "config.json").write_text(json.dumps(R.model_config_dict(R.tiny_cfg("qwen2"))))
    with pytest.raises(NotImplementedError, match="internvl_chat"):
        convert(str(src), str(tmp_path / "out"), quantize=True)
    assert not hasattr(_host_model(), "merge_input_ids_with_image_features")          # what BatchGenerator(apc_manager=) asks for


# ---------------------------------------------------------------- the C ABI
def test_abi_still_60_names_at_version_8_and_the_flag_is_documented():
    root = os.path.dirname(HERE)
    hdr = open(os.path.join(root, "include", "vlm_hip.h")).read()
    assert len(set(re.findall(r"\b(vlm_[a-z0-9_]+)\s*\(", hdr))) == 60
    from mlx_vlm_amd import _lib, ops

    assert len(_lib.SIGNATURES) == 60
    assert re.search(r"vlm_abi_version\(void\)\s*\{\s*return 8;", open(os.path.join(root, "mlx-vlm_amd", "csrc", "engine.hip")).read())
    flags = {n: int(v) for n, v in re.findall(r"#define (VLM_EPI_[A-Z0-9_]+) (\d+)", hdr)}
    assert flags["VLM_EPI_LAYERSCALE"] == ops.EPI_LAYERSCALE == 512
    others = [v for n, v in flags.items() if n != "VLM_EPI_LAYERSCALE"] + [32]          # 32: VLM_EPI_ROPE2D, taken inside the library
    assert all(v & 512 == 0 for v in others)
    assert "[2][N]" in hdr and "[2][E]" in hdr
    b = ops.bias_scale(torch.arange(8.0), torch.arange(8.0) + 8)
    assert b.shape == (2, 8) and b.dtype == torch.bfloat16 and b.is_contiguous() and b.reshape(-1).tolist() == list(range(16))
