"""Shared helpers of tests/test_convert_cpu.py and tests/test_convert_gpu.py: a tiny Qwen2-VL checkpoint on disk in the HF
layout (what tests/test_engine_gpu.py::_write_tiny_checkpoint writes, plus the `torch_dtype` / `_name_or_path` keys every
real HF config carries) and readers of a checkpoint directory."""
from __future__ import annotations

import glob
import json
import os

import torch


def qwen2_vl_hf_config(cfg) -> dict:
    t, v = cfg.text, cfg.vision
    return dict(model_type="qwen2_vl", hidden_size=t.hidden_size, num_hidden_layers=t.num_hidden_layers,
                intermediate_size=t.intermediate_size, num_attention_heads=t.num_attention_heads,
                num_key_value_heads=t.num_key_value_heads, vocab_size=t.vocab_size, rms_norm_eps=t.rms_norm_eps,
                rope_theta=t.rope_theta, rope_scaling={"type": "mrope", "mrope_section": list(t.mrope_section)},
                tie_word_embeddings=t.tie_word_embeddings, image_token_id=cfg.image_token_id,
                video_token_id=cfg.video_token_id, vision_start_token_id=cfg.vision_start_token_id, eos_token_id=[1],
                torch_dtype="bfloat16", _name_or_path="tiny/qwen2-vl",
                vision_config=dict(model_type="qwen2_vl", depth=v.depth, embed_dim=v.embed_dim, hidden_size=v.hidden_size,
                                   num_heads=v.num_heads, patch_size=v.patch_size, mlp_ratio=int(v.mlp_ratio),
                                   in_channels=v.in_channels, spatial_merge_size=v.spatial_merge_size,
                                   temporal_patch_size=v.temporal_patch_size))


def to_hf_names(W) -> dict:
    """oracle (= sanitized, MLX-format) names -> the classic HF Qwen2-VL names; conv weight (O,T,H,W,C) -> HF (O,C,T,H,W)"""
    hf = {}
    for k, w in W.items():
        w = w.contiguous()
        if k.startswith("vision_tower."):
            hk = "visual." + k[len("vision_tower."):]
            if "patch_embed.proj.weight" in k:
                w = w.permute(0, 4, 1, 2, 3).contiguous()
        elif k.startswith("language_model.model."):
            hk = "model." + k[len("language_model.model."):]
        else:
            hk = "lm_head." + k[len("language_model.lm_head."):]
        hf[hk] = w
    return hf


def write_tiny_checkpoint(path, cfg, W, hf_layout: bool = True, config_extra=None, tokenizer: bool = True):
    """config.json + model.safetensors (+ a WordLevel tokenizer with the special vision tokens and a preprocessor config).
    hf_layout=False: the tensors go to disk under the names they have (an MLX-format checkpoint, e.g. a quantized one)."""
    from safetensors.torch import save_file

    os.makedirs(path, exist_ok=True)
    conf = qwen2_vl_hf_config(cfg)
    conf.update(config_extra or {})
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(conf, f)
    tensors = to_hf_names(W) if hf_layout else {k: v.contiguous() for k, v in W.items()}
    save_file({k: (v.view(torch.uint32) if v.dtype == torch.int32 else v) for k, v in tensors.items()},
              os.path.join(path, "model.safetensors"))
    with open(os.path.join(path, "preprocessor_config.json"), "w") as f:
        json.dump(dict(image_mean=[0.5] * 3, image_std=[0.5] * 3), f)
    if not tokenizer:
        return
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast

    t = cfg.text
    vocab = {f"t{i}": i for i in range(t.vocab_size)}
    for name, idx in (("<unk>", 0), ("<eos>", 1), ("<pad>", 2), ("<|image_pad|>", cfg.image_token_id),
                      ("<|video_pad|>", cfg.video_token_id), ("<|vision_start|>", cfg.vision_start_token_id),
                      ("<|vision_end|>", cfg.vision_start_token_id + 1)):
        del vocab[f"t{idx}"]
        vocab[name] = idx
    tok = Tokenizer(models.WordLevel(vocab, unk_token="<unk>"))
    tok.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    fast = PreTrainedTokenizerFast(tokenizer_object=tok, eos_token="<eos>", pad_token="<pad>", unk_token="<unk>")
    fast.add_special_tokens({"additional_special_tokens": ["<|image_pad|>", "<|video_pad|>", "<|vision_start|>", "<|vision_end|>"]})
    fast.save_pretrained(str(path))


def read_tensors(path) -> dict:
    """every tensor of every *.safetensors of a directory; uint32 words come back as their int32 bit patterns"""
    from safetensors.torch import load_file

    out = {}
    for f in sorted(glob.glob(os.path.join(path, "*.safetensors"))):
        out.update(load_file(f))
    return {k: (v.view(torch.int32) if v.dtype == torch.uint32 else v) for k, v in out.items()}


def read_metadata(file) -> dict:
    from safetensors import safe_open

    with safe_open(file, framework="pt") as f:
        return f.metadata()


def assert_same_tensors(got: dict, want: dict):
    """same keys, dtypes, shapes and bits (int32 patterns compared as they are, floats through their bit patterns)"""
    assert sorted(got) == sorted(want), (sorted(set(got) ^ set(want))[:8])
    for k, w in want.items():
        g = got[k]
        w = w.view(torch.int32) if w.dtype == torch.uint32 else w
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        bits = {2: torch.int16, 4: torch.int32}[g.element_size()]
        assert torch.equal(g.contiguous().view(bits), w.contiguous().view(bits)), k
