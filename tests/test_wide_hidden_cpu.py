"""Hidden sizes up to 8192 on the host: the model builds at Qwen2-VL-72B's text widths, wider ones are refused at
construction, and the C ABI is what it was (60 names, version 8)."""
import os
import re

import pytest
import torch

from oracle import qwen2_vl as oq
from oracle import quant as Q

BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg_72b(hidden=8192, layers=1, vocab=2048):
    """Qwen2-VL-72B's text config - hidden 8192, 64 query heads over 8 KV heads of 128, intermediate 29568, untied head - at one
    layer and a 2048-row vocabulary (the real 152064 rows are 2.5 GB per table: no width changes with them); tiny tower"""
    text = oq.TextCfg(hidden_size=hidden, num_hidden_layers=layers, intermediate_size=29568, num_attention_heads=64,
                      num_key_value_heads=8, vocab_size=vocab, tie_word_embeddings=False)
    return oq.Cfg(text=text, vision=oq.VisionCfg(depth=1, embed_dim=160, hidden_size=hidden, num_heads=2),
                  image_token_id=1001, video_token_id=1002, vision_start_token_id=1003)


def test_72b_text_widths_build_and_pack_4bit_on_the_host():
    from mlx_vlm_amd.models import quantized as Qz
    from mlx_vlm_amd.models.qwen2_vl import Model
    from tests.helpers import model_config_from_oracle

    cfg = _cfg_72b()
    W = oq.random_weights(cfg, seed=3, dtype=BF, std=0.02, fast=True)
    ck, ow = Q.quantize_checkpoint(W, predicate=lambda p, v: p.startswith("language_model."))
    del W
    model = Model(model_config_from_oracle(cfg), device="cpu", kv_pool_tokens=1024, max_seqs=2)
    model.load_weights({k: (v.view(torch.uint32) if v.dtype == torch.int32 else v) for k, v in ck.items()})
    lm = model.language_model
    assert lm.quantized and lm.head_dim == 128
    t = cfg.text
    wqkv, wgu, wdown, wo = lm._w["0.wqkv"], lm._w["0.wgu"], lm._w["0.wdown"], lm._w["0.wo"]
    assert isinstance(wqkv, Qz.QuantW) and wqkv.shape == ((64 + 2 * 8) * 128, 8192)
    assert wgu.shape == (2 * 29568, 8192) and wdown.shape == (8192, 29568) and wo.shape == (8192, 8192)
    assert torch.equal(wgu.wq[1::2], ow["language_model.model.layers.0.mlp.up_proj.weight"].wq)
    assert lm._w["embed"].shape == (t.vocab_size, 8192)


@pytest.mark.parametrize("hidden", [8320, 16384])
def test_hidden_past_8192_is_refused_at_construction(hidden):
    from mlx_vlm_amd.models.qwen2_vl import Model
    from tests.helpers import model_config_from_oracle

    with pytest.raises(NotImplementedError, match="8192"):
        Model(model_config_from_oracle(_cfg_72b(hidden=hidden)), device="cpu", kv_pool_tokens=1024, max_seqs=2)


def test_bf16_model_builds_at_hidden_8192():
    from mlx_vlm_amd.models.qwen2_vl import Model
    from tests.helpers import model_config_from_oracle

    model = Model(model_config_from_oracle(_cfg_72b()), device="cpu", kv_pool_tokens=1024, max_seqs=2)
    assert model.language_model.args.hidden_size == 8192 and model.language_model.n_kv_heads == 8


def test_abi_is_unchanged_60_names_version_8():
    hdr = open(os.path.join(ROOT, "include", "vlm_hip.h")).read()
    assert len(set(re.findall(r"\b(vlm_[a-z0-9_]+)\s*\(", hdr))) == 60
    src = open(os.path.join(ROOT, "mlx-vlm_amd", "csrc", "engine.hip")).read()
    assert re.search(r"int vlm_abi_version\(void\) \{ return 8; \}", src)
