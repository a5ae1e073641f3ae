"""Torch restatement of mlx_vlm.models.qwen2_5_vl (TEST HELPER, not a test), in the style of oracle/qwen2_vl.py.

Follows the reference's qwen2_5_vl/{vision,qwen2_5_vl}.py function by function on torch-CPU tensors, every op's bf16 rounding
through oracle.ops; the language half IS oracle.qwen2_vl (the reference's two language.py files differ in comments and in the
tiling of position ids it makes itself for batched text-only calls).  Weights: a flat dict under the reference's sanitized names
(`vision_tower.*`, `language_model.model.*`).  Pinned to the reference itself by tests/golden/qwen2_5_vl_tiny_ref.npz and to
transformers by qwen2_5_vl_tiny_hf.npz (tests/test_qwen2_5_vl_cpu.py).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

from oracle import ops
from oracle import qwen2_vl as oq


@dataclass
class VisionCfg:
    depth: int = 32
    hidden_size: int = 1280
    intermediate_size: int = 3420
    out_hidden_size: int = 1536
    num_heads: int = 16
    patch_size: int = 14
    in_channels: int = 3
    spatial_merge_size: int = 2
    temporal_patch_size: int = 2
    window_size: int = 112
    fullatt_block_indexes: List[int] = field(default_factory=lambda: [7, 15, 23, 31])


@dataclass
class Cfg:
    text: oq.TextCfg = field(default_factory=oq.TextCfg)
    vision: VisionCfg = field(default_factory=VisionCfg)
    image_token_id: int = 151655
    video_token_id: int = 151656
    vision_start_token_id: int = 151652


def tiny_cfg(**vision_over) -> Cfg:
    """oracle.qwen2_vl.tiny_cfg()'s text half + a two-block tower: block 0 windowed, block 1 full; 2 heads of 80; an
    intermediate size that is no multiple of 8 (as 3420 is not)."""
    t = oq.tiny_cfg()
    v = VisionCfg(depth=2, hidden_size=160, intermediate_size=172, out_hidden_size=256, num_heads=2, fullatt_block_indexes=[1])
    for k, val in vision_over.items():
        setattr(v, k, val)
    return Cfg(text=t.text, vision=v, image_token_id=t.image_token_id, video_token_id=t.video_token_id,
               vision_start_token_id=t.vision_start_token_id)


def real_width_cfg(depth: int = 2, fullatt=(1,)) -> Cfg:
    """the real tower widths (1280 / 16 heads / 3420 / out 2048) over the tiny text model"""
    c = tiny_cfg(depth=depth, hidden_size=1280, intermediate_size=3420, out_hidden_size=2048, num_heads=16,
                 fullatt_block_indexes=list(fullatt))
    return c


def random_weights(cfg: Cfg, seed: int = 0, dtype=torch.bfloat16, std: float = 0.02, embed_std: Optional[float] = None,
                   tower_only: bool = False) -> Dict[str, torch.Tensor]:
    """Synthetic checkpoint in the manner of oracle.qwen2_vl.random_weights: Linear / Embedding ~ N(0, std^2), norm weights
    1 + noise, biases small noise."""
    g = torch.Generator().manual_seed(seed)
    W: Dict[str, torch.Tensor] = {}

    def rn(*shape, s=std):
        return (torch.randn(*shape, generator=g) * s).to(dtype)

    v = cfg.vision
    E, I = v.hidden_size, v.intermediate_size
    W["vision_tower.patch_embed.proj.weight"] = rn(E, v.temporal_patch_size, v.patch_size, v.patch_size, v.in_channels)
    for i in range(v.depth):
        p = f"vision_tower.blocks.{i}."
        W[p + "norm1.weight"] = (1 + rn(E, s=0.05).float()).to(dtype)
        W[p + "norm2.weight"] = (1 + rn(E, s=0.05).float()).to(dtype)
        W[p + "attn.qkv.weight"] = rn(3 * E, E)
        W[p + "attn.qkv.bias"] = rn(3 * E)
        W[p + "attn.proj.weight"] = rn(E, E)
        W[p + "attn.proj.bias"] = rn(E)
        for n in ("gate_proj", "up_proj"):
            W[p + f"mlp.{n}.weight"] = rn(I, E)
            W[p + f"mlp.{n}.bias"] = rn(I)
        W[p + "mlp.down_proj.weight"] = rn(E, I)
        W[p + "mlp.down_proj.bias"] = rn(E)
    M = E * v.spatial_merge_size ** 2
    W["vision_tower.merger.ln_q.weight"] = (1 + rn(E, s=0.05).float()).to(dtype)
    W["vision_tower.merger.mlp.0.weight"] = rn(M, M)
    W["vision_tower.merger.mlp.0.bias"] = rn(M)
    W["vision_tower.merger.mlp.2.weight"] = rn(v.out_hidden_size, M)
    W["vision_tower.merger.mlp.2.bias"] = rn(v.out_hidden_size)
    if tower_only:
        return W
    t = cfg.text
    D = t.hidden_size
    hd = D // t.num_attention_heads
    W["language_model.model.embed_tokens.weight"] = rn(t.vocab_size, D, s=embed_std or std)
    for i in range(t.num_hidden_layers):
        p = f"language_model.model.layers.{i}."
        W[p + "input_layernorm.weight"] = (1 + rn(D, s=0.05).float()).to(dtype)
        W[p + "post_attention_layernorm.weight"] = (1 + rn(D, s=0.05).float()).to(dtype)
        for n, rows in (("q_proj", t.num_attention_heads * hd), ("k_proj", t.num_key_value_heads * hd),
                        ("v_proj", t.num_key_value_heads * hd)):
            W[p + f"self_attn.{n}.weight"] = rn(rows, D)
            W[p + f"self_attn.{n}.bias"] = rn(rows)
        W[p + "self_attn.o_proj.weight"] = rn(D, t.num_attention_heads * hd)
        W[p + "mlp.gate_proj.weight"] = rn(t.intermediate_size, D)
        W[p + "mlp.up_proj.weight"] = rn(t.intermediate_size, D)
        W[p + "mlp.down_proj.weight"] = rn(D, t.intermediate_size)
    W["language_model.model.norm.weight"] = (1 + rn(D, s=0.05).float()).to(dtype)
    if not t.tie_word_embeddings:
        W["language_model.lm_head.weight"] = rn(t.vocab_size, D, s=embed_std or std)
    return W


# --------------------------------------------------------------------------
# vision tower (qwen2_5_vl/vision.py)
# --------------------------------------------------------------------------
def get_window_index(cfg: Cfg, grid_thw):
    """VisionModel.get_window_index (vision.py:261-324) -> (window_index int64, cu_window_seqlens int64 WITH repeats)."""
    v = cfg.vision
    ms, unit = v.spatial_merge_size, v.spatial_merge_size ** 2
    vw = v.window_size // ms // v.patch_size
    window_index, cu, base = [], [0], 0
    for gt, gh, gw in np.asarray(grid_thw).tolist():
        lh, lw = gh // ms, gw // ms
        index = np.arange(gt * lh * lw).reshape(gt, lh, lw)
        ph, pw = vw - lh % vw, vw - lw % vw
        nh, nw = (lh + ph) // vw, (lw + pw) // vw
        padded = np.pad(index, ((0, 0), (0, ph), (0, pw)), constant_values=-100)
        padded = padded.reshape(gt, nh, vw, nw, vw).transpose(0, 1, 3, 2, 4).reshape(gt, nh * nw, vw, vw)
        seqlens = (padded != -100).sum(axis=(2, 3)).reshape(-1)
        flat = padded.reshape(-1)
        window_index.append(flat[flat != -100] + base)
        cu.extend((np.cumsum(seqlens) * unit + cu[-1]).tolist())
        base += gt * lh * lw
    return np.concatenate(window_index).astype(np.int64), np.asarray(cu, dtype=np.int64)


def unique_first(cu) -> np.ndarray:
    """vision.py:337-346: first occurrence of each value"""
    seen, out = set(), []
    for x in np.asarray(cu).tolist():
        if x not in seen:
            seen.add(x)
            out.append(x)
    return np.asarray(out, dtype=np.int64)


def patch_embed(W, cfg: Cfg, pixel_values):
    """PatchEmbed (vision.py:69-103)"""
    v = cfg.vision
    x = pixel_values.reshape(-1, v.in_channels, v.temporal_patch_size, v.patch_size, v.patch_size)
    x = x.permute(0, 2, 3, 4, 1).reshape(x.shape[0], -1)
    return ops.linear(x, W["vision_tower.patch_embed.proj.weight"].reshape(v.hidden_size, -1))


def vision_attention(W, p, cfg: Cfg, x, cu_seqlens, freqs):
    """Attention (vision.py:124-163)"""
    H, N = cfg.vision.num_heads, x.shape[0]
    qkv = ops.linear(x, W[p + "qkv.weight"], W[p + "qkv.bias"]).reshape(N, 3, H, -1)
    q, k, v = qkv[:, 0], qkv[:, 1], qkv[:, 2]
    q = ops.apply_rotary_pos_emb_vision(q, freqs)
    k = ops.apply_rotary_pos_emb_vision(k, freqs)
    D = q.shape[-1]
    outs = []
    for a, b in zip(cu_seqlens[:-1], cu_seqlens[1:]):
        o = ops.sdpa(q[a:b].permute(1, 0, 2)[None], k[a:b].permute(1, 0, 2)[None], v[a:b].permute(1, 0, 2)[None], scale=D ** -0.5)
        outs.append(o[0].permute(1, 0, 2))
    return ops.linear(torch.cat(outs, dim=0).reshape(N, -1), W[p + "proj.weight"], W[p + "proj.bias"])


def vision_mlp(W, p, x):
    """MLP (vision.py:166-174): down(silu(gate(x)) * up(x)), biases everywhere"""
    g = ops.linear(x, W[p + "gate_proj.weight"], W[p + "gate_proj.bias"])
    u = ops.linear(x, W[p + "up_proj.weight"], W[p + "up_proj.bias"])
    return ops.linear(ops.swiglu(g, u), W[p + "down_proj.weight"], W[p + "down_proj.bias"])


def vision_block(W, i, cfg: Cfg, x, cu_seqlens, freqs):
    """Qwen2VLVisionBlock (vision.py:177-193)"""
    p = f"vision_tower.blocks.{i}."
    x = ops.add(x, vision_attention(W, p + "attn.", cfg, ops.rms_norm(x, W[p + "norm1.weight"], 1e-6), cu_seqlens, freqs))
    return ops.add(x, vision_mlp(W, p + "mlp.", ops.rms_norm(x, W[p + "norm2.weight"], 1e-6)))


def patch_merger(W, cfg: Cfg, x):
    """PatchMerger (vision.py:106-121)"""
    p = "vision_tower.merger."
    m = cfg.vision.hidden_size * cfg.vision.spatial_merge_size ** 2
    x = ops.rms_norm(x, W[p + "ln_q.weight"], 1e-6).reshape(-1, m)
    x = ops.gelu_erf(ops.linear(x, W[p + "mlp.0.weight"], W[p + "mlp.0.bias"]))
    return ops.linear(x, W[p + "mlp.2.weight"], W[p + "mlp.2.bias"])


def vision_tower(W, cfg: Cfg, pixel_values, grid_thw, patch_embeds=None, return_tables: bool = False):
    """VisionModel.__call__ (vision.py:326-393).  `patch_embeds` (tests only): start from given PatchEmbed outputs."""
    v = cfg.vision
    unit = v.spatial_merge_size ** 2
    x = patch_embed(W, cfg, pixel_values) if patch_embeds is None else patch_embeds
    freqs = ops.vision_rotary_freqs(np.asarray(grid_thw), v.hidden_size // v.num_heads, v.spatial_merge_size)
    wi, cu_win = get_window_index(cfg, grid_thw)
    cu_win = unique_first(cu_win)
    N = x.shape[0]
    idx = torch.from_numpy(wi)
    x = x.reshape(N // unit, unit, -1)[idx].reshape(N, -1)
    freqs = freqs.reshape(N // unit, unit, -1)[idx].reshape(N, -1)
    cu_full = oq.vision_cu_seqlens(grid_thw).astype(np.int64)
    for i in range(v.depth):
        x = vision_block(W, i, cfg, x, cu_full if i in v.fullatt_block_indexes else cu_win, freqs)
    out = patch_merger(W, cfg, x)
    rev = np.argsort(wi, kind="stable")
    out = out[torch.from_numpy(rev)]
    if return_tables:
        return out, {"window_index": wi, "cu_window": cu_win, "cu_full": cu_full, "reverse_index": rev}
    return out


# --------------------------------------------------------------------------
# model (qwen2_5_vl/qwen2_5_vl.py) over oracle.qwen2_vl's language half
# --------------------------------------------------------------------------
def get_input_embeddings(W, cfg: Cfg, input_ids, pixel_values=None, image_grid_thw=None, mask=None):
    """Model.get_input_embeddings (qwen2_5_vl.py:20-76) -> inputs_embeds, position_ids, rope_deltas"""
    emb = oq.embed_tokens(W, input_ids)
    if pixel_values is None:
        pos, deltas = oq.get_rope_index(cfg, input_ids, attention_mask=mask)
        return emb, pos, deltas
    dtype = W["vision_tower.patch_embed.proj.weight"].dtype
    feats = vision_tower(W, cfg, pixel_values.to(dtype), image_grid_thw)
    emb = oq.merge_input_ids_with_image_features(cfg, feats, emb, input_ids)
    pos, deltas = oq.get_rope_index(cfg, input_ids, image_grid_thw, None, mask)
    return emb, pos, deltas


def prefill_logits(W, cfg: Cfg, input_ids, pixel_values=None, image_grid_thw=None, rope_mode: str = "fused"):
    """logits of every prompt row, no cache -> [L, V].  rope_mode as oracle.qwen2_vl: "fused" = the fused M-RoPE kernel's
    numerics (what the engine runs), "fallback" = the pure-MLX path (what the reference takes over the shim)."""
    emb, pos, _ = get_input_embeddings(W, cfg, input_ids, pixel_values, image_grid_thw)
    pos = np.asarray(pos)
    if pos.ndim == 2:
        pos = np.broadcast_to(pos[None], (3,) + pos.shape)
    h = oq.qwen2_model(W, cfg, emb, None, torch.from_numpy(np.ascontiguousarray(pos)), rope_mode)
    return oq.lm_head(W, cfg, h)[0]


def generate_greedy(W, cfg: Cfg, input_ids, pixel_values=None, image_grid_thw=None, max_tokens: int = 16,
                    return_logprobs: bool = False, return_logits: bool = False, rope_mode: str = "fused"):
    """generate_step at temperature 0 (oracle.qwen2_vl.generate_greedy with this family's embeddings)"""
    input_ids = np.asarray(input_ids)
    assert input_ids.shape[0] == 1
    emb, pos, deltas = get_input_embeddings(W, cfg, input_ids, pixel_values, image_grid_thw)
    pos = np.asarray(pos)
    if pos.ndim == 2:
        pos = np.broadcast_to(pos[None], (3,) + pos.shape)
    cache = oq._make_prompt_cache(cfg)
    h = oq.qwen2_model(W, cfg, emb, cache, torch.from_numpy(np.ascontiguousarray(pos)), rope_mode)
    logits = oq.lm_head(W, cfg, h)[:, -1, :]
    toks, all_lp, all_logits = [], [], []
    delta = int(deltas[0, 0])
    for n in range(max_tokens):
        lp = ops.logprobs_from_logits(logits)
        y = int(ops.argmax_first(lp)[0])
        toks.append(y)
        all_lp.append(lp[0].clone())
        all_logits.append(logits[0].clone())
        if n == max_tokens - 1:
            break
        e = oq.embed_tokens(W, np.array([[y]]))
        pid = torch.full((3, 1, 1), oq._cache_offset(cache[0]) + delta, dtype=torch.long)
        h = oq.qwen2_model(W, cfg, e, cache, pid, rope_mode)
        logits = oq.lm_head(W, cfg, h)[:, -1, :]
    if return_logprobs:
        return toks, torch.stack(all_lp)
    if return_logits:
        return toks, torch.stack(all_logits)
    return toks


def synth_request(cfg: Cfg, grids, n_text: int = 12, seed: int = 0):
    """A prompt over images GIVEN AS GRIDS (the image processor never emits a 2 x 2 grid: its smallest image is 56 x 56 pixels)
    -> (input_ids [1, L] int64, pixel_values f32 [N, C*T*ps*ps] uniform in [-1, 1), grid_thw int64 [n, 3])"""
    rng = np.random.default_rng(seed)
    v = cfg.vision
    thw = np.asarray(grids, dtype=np.int64).reshape(-1, 3)
    ids: List[int] = []
    if len(thw):
        N = int(thw.prod(axis=1).sum())
        pix = rng.uniform(-1.0, 1.0, (N, v.in_channels * v.temporal_patch_size * v.patch_size ** 2)).astype(np.float32)
        for g in thw:
            ids += [cfg.vision_start_token_id] + [cfg.image_token_id] * (int(g.prod()) // v.spatial_merge_size ** 2)
            ids += [cfg.vision_start_token_id + 1] + rng.integers(3, 1000, 3).tolist()
    else:
        pix = None
    ids += rng.integers(3, 1000, n_text).tolist()
    return np.array([ids], dtype=np.int64), pix, (thw if len(thw) else None)


# --------------------------------------------------------------------------
# product-model construction (the counterpart of tests/helpers.build_product_model)
# --------------------------------------------------------------------------
def model_config_dict(cfg: Cfg, quantization=None) -> dict:
    t, v = cfg.text, cfg.vision
    d = dict(
        model_type="qwen2_5_vl", hidden_size=t.hidden_size, num_hidden_layers=t.num_hidden_layers,
        intermediate_size=t.intermediate_size, num_attention_heads=t.num_attention_heads,
        num_key_value_heads=t.num_key_value_heads, rms_norm_eps=t.rms_norm_eps, vocab_size=t.vocab_size,
        rope_theta=t.rope_theta, rope_scaling={"type": "mrope", "mrope_section": list(t.mrope_section)},
        tie_word_embeddings=t.tie_word_embeddings, image_token_id=cfg.image_token_id, video_token_id=cfg.video_token_id,
        vision_start_token_id=cfg.vision_start_token_id,
        vision_config=dict(model_type="qwen2_5_vl", depth=v.depth, hidden_size=v.hidden_size,
                           intermediate_size=v.intermediate_size, out_hidden_size=v.out_hidden_size, num_heads=v.num_heads,
                           patch_size=v.patch_size, in_channels=v.in_channels, spatial_merge_size=v.spatial_merge_size,
                           temporal_patch_size=v.temporal_patch_size, window_size=v.window_size,
                           fullatt_block_indexes=list(v.fullatt_block_indexes)))
    if quantization:
        d["quantization"] = quantization
    return d


def write_checkpoint(path, cfg: Cfg, W, quantization=None):
    """HF Qwen2.5-VL layout on disk: config.json (text parameters at the root, "model_type": "qwen2_5_vl"), model.safetensors
    under the HF key names (visual.* / model.*; conv weight (O, C, T, H, W)), a WordLevel tokenizer with the vision tokens."""
    import json

    from safetensors.torch import save_file
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast

    conf = model_config_dict(cfg, quantization)
    conf["eos_token_id"] = [1]
    (path / "config.json").write_text(json.dumps(conf))
    hf = {}
    for k, w in W.items():
        w = w.contiguous()
        if k.startswith("vision_tower."):
            hk = "visual." + k[len("vision_tower."):]
            if "patch_embed.proj.weight" in k:
                w = w.permute(0, 4, 1, 2, 3).contiguous()          # (O, T, H, W, C) -> HF (O, C, T, H, W)
        elif k.startswith("language_model.model."):
            hk = "model." + k[len("language_model.model."):]
        else:
            hk = "lm_head." + k[len("language_model.lm_head."):]
        hf[hk] = w
    save_file(hf, str(path / "model.safetensors"))
    vocab = {f"t{i}": i for i in range(cfg.text.vocab_size)}
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
    (path / "preprocessor_config.json").write_text(json.dumps(dict(image_mean=[0.5] * 3, image_std=[0.5] * 3)))


def build_product_model(cfg: Cfg, W, device="cuda", **kw):
    from mlx_vlm_amd.models.qwen2_5_vl import Model, ModelConfig

    m = Model(ModelConfig.from_dict(model_config_dict(cfg)), device=device, **kw)
    m.load_weights(W)
    return m
