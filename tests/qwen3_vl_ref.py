"""Torch restatement of mlx_vlm.models.qwen3_vl (TEST HELPER, not a test), in the style of oracle/qwen2_vl.py.

Follows the reference's qwen3_vl/{vision,language,qwen3_vl}.py function by function on torch-CPU tensors, every op's bf16
rounding through oracle.ops.  Weights: a flat dict under the reference's sanitized names (`vision_tower.*`,
`language_model.model.*`).  Pinned to the reference itself by tests/golden/qwen3_vl_tiny_ref.npz (bit-exact, fallback rope mode)
and to transformers by qwen3_vl_tiny_hf.npz (tests/test_qwen3_vl_cpu.py).

rope_mode as in oracle.qwen2_vl: "fused" = the numerics of the reference's fused M-RoPE kernel (fp32 angle, fp32 rotation, one
rounding - what the engine runs), "fallback" = its pure-MLX path (cos / sin rounded to T, typed multiplies and add - what the
reference takes over the MLX stand-in).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

from oracle import ops
from oracle import qwen2_vl as oq

F32 = torch.float32


@dataclass
class VisionCfg:
    depth: int = 24
    hidden_size: int = 1024
    intermediate_size: int = 4096
    out_hidden_size: int = 2048
    num_heads: int = 16
    patch_size: int = 16
    in_channels: int = 3
    spatial_merge_size: int = 2
    temporal_patch_size: int = 2
    num_position_embeddings: int = 2304
    deepstack_visual_indexes: List[int] = field(default_factory=lambda: [5, 11, 17])


@dataclass
class TextCfg:
    hidden_size: int = 2048
    num_hidden_layers: int = 28
    intermediate_size: int = 6144
    num_attention_heads: int = 16
    num_key_value_heads: int = 8
    head_dim: int = 128
    vocab_size: int = 151936
    rms_norm_eps: float = 1e-6
    rope_theta: float = 5000000.0
    mrope_section: List[int] = field(default_factory=lambda: [24, 20, 20])
    tie_word_embeddings: bool = True


@dataclass
class Cfg:
    text: TextCfg = field(default_factory=TextCfg)
    vision: VisionCfg = field(default_factory=VisionCfg)
    image_token_id: int = 151655
    video_token_id: int = 151656
    vision_start_token_id: int = 151652


def tiny_cfg(**vision_over) -> Cfg:
    """4 decoder layers of 4 : 2 heads of 128 over hidden 256 (n_heads * head_dim != hidden, as in the 4B model); a tower of 3
    blocks, 2 heads of 64, an intermediate size that is no multiple of 64 (as the 8B's 4304 is not), an 8 x 8 position table and
    two DeepStack taps - one behind the first block, one behind the last."""
    t = TextCfg(hidden_size=256, num_hidden_layers=4, intermediate_size=512, num_attention_heads=4, num_key_value_heads=2,
                head_dim=128, vocab_size=2048)
    v = VisionCfg(depth=3, hidden_size=128, intermediate_size=344, out_hidden_size=256, num_heads=2, num_position_embeddings=64,
                  deepstack_visual_indexes=[0, 2])
    for k, val in vision_over.items():
        setattr(v, k, val)
    return Cfg(text=t, vision=v, image_token_id=2001, video_token_id=2002, vision_start_token_id=2003)


def random_weights(cfg: Cfg, seed: int = 0, dtype=torch.bfloat16, std: float = 0.02, embed_std: Optional[float] = None,
                   tower_only: bool = False) -> Dict[str, torch.Tensor]:
    """Synthetic checkpoint in the manner of oracle.qwen2_vl.random_weights: Linear / Embedding ~ N(0, std^2), norm weights
    1 + noise (the q / k norms too: drawn around 1, not equal to 1), biases small noise."""
    g = torch.Generator().manual_seed(seed)
    W: Dict[str, torch.Tensor] = {}

    def rn(*shape, s=std):
        return (torch.randn(*shape, generator=g) * s).to(dtype)

    def near1(n, s=0.05):
        return (1 + rn(n, s=s).float()).to(dtype)

    v = cfg.vision
    E, I = v.hidden_size, v.intermediate_size
    M = E * v.spatial_merge_size ** 2
    W["vision_tower.patch_embed.proj.weight"] = rn(E, v.temporal_patch_size, v.patch_size, v.patch_size, v.in_channels)
    W["vision_tower.patch_embed.proj.bias"] = rn(E)
    W["vision_tower.pos_embed.weight"] = rn(v.num_position_embeddings, E, s=0.1)
    for i in range(v.depth):
        p = f"vision_tower.blocks.{i}."
        for n in ("norm1", "norm2"):
            W[p + n + ".weight"] = near1(E)
            W[p + n + ".bias"] = rn(E)
        W[p + "attn.qkv.weight"] = rn(3 * E, E)
        W[p + "attn.qkv.bias"] = rn(3 * E)
        W[p + "attn.proj.weight"] = rn(E, E)
        W[p + "attn.proj.bias"] = rn(E)
        W[p + "mlp.linear_fc1.weight"] = rn(I, E)
        W[p + "mlp.linear_fc1.bias"] = rn(I)
        W[p + "mlp.linear_fc2.weight"] = rn(E, I)
        W[p + "mlp.linear_fc2.bias"] = rn(E)

    def merger(p, norm_dim):
        W[p + "norm.weight"] = near1(norm_dim)
        W[p + "norm.bias"] = rn(norm_dim)
        W[p + "linear_fc1.weight"] = rn(M, M)
        W[p + "linear_fc1.bias"] = rn(M)
        W[p + "linear_fc2.weight"] = rn(v.out_hidden_size, M)
        W[p + "linear_fc2.bias"] = rn(v.out_hidden_size)

    merger("vision_tower.merger.", E)
    for j in range(len(v.deepstack_visual_indexes)):
        merger(f"vision_tower.deepstack_merger_list.{j}.", M)
    if tower_only:
        return W
    t = cfg.text
    D, hd = t.hidden_size, t.head_dim
    W["language_model.model.embed_tokens.weight"] = rn(t.vocab_size, D, s=embed_std or std)
    for i in range(t.num_hidden_layers):
        p = f"language_model.model.layers.{i}."
        W[p + "input_layernorm.weight"] = near1(D)
        W[p + "post_attention_layernorm.weight"] = near1(D)
        W[p + "self_attn.q_proj.weight"] = rn(t.num_attention_heads * hd, D)
        W[p + "self_attn.k_proj.weight"] = rn(t.num_key_value_heads * hd, D)
        W[p + "self_attn.v_proj.weight"] = rn(t.num_key_value_heads * hd, D)
        W[p + "self_attn.o_proj.weight"] = rn(D, t.num_attention_heads * hd)
        W[p + "self_attn.q_norm.weight"] = near1(hd, s=0.1)
        W[p + "self_attn.k_norm.weight"] = near1(hd, s=0.1)
        W[p + "mlp.gate_proj.weight"] = rn(t.intermediate_size, D)
        W[p + "mlp.up_proj.weight"] = rn(t.intermediate_size, D)
        W[p + "mlp.down_proj.weight"] = rn(D, t.intermediate_size)
    W["language_model.model.norm.weight"] = near1(D)
    if not t.tie_word_embeddings:
        W["language_model.lm_head.weight"] = rn(t.vocab_size, D, s=embed_std or std)
    return W


# --------------------------------------------------------------------------
# typed elementary graphs
# --------------------------------------------------------------------------
def gelu_tanh(x):
    """nn.GELU(approx="tanh") = mlx.nn.gelu_approx: 0.5 * x * (1 + tanh(sqrt(2 / pi) * (x + 0.044715 * x ** 3)))
    (vision.py:169).  Typed graph, left to right as Python evaluates it: T(0.5) * x -> T; x ** 3 -> T; T(0.044715) * . -> T;
    x + . -> T; T(sqrt(2 / pi)) * . -> T; tanh -> T; 1 + . -> T; product -> T."""
    T = x.dtype
    xf = x.to(F32)
    half = (ops._c(0.5, T) * xf).to(T)
    x3 = torch.pow(xf, 3.0).to(T)
    inner = (xf + (ops._c(0.044715, T) * x3.to(F32)).to(T).to(F32)).to(T)
    arg = (ops._c(math.sqrt(2 / math.pi), T) * inner.to(F32)).to(T)
    th = torch.tanh(arg.to(F32)).to(T)
    one = (1.0 + th.to(F32)).to(T)
    return (half.to(F32) * one.to(F32)).to(T)


def interleaved_position_selector(mrope_section, freq_dim: int):
    """_interleaved_position_selector (rope_utils.py:511-516): frequency index f -> position axis (0 = t, 1 = h, 2 = w)"""
    sel = [0] * freq_dim
    for dim, offset in enumerate((1, 2), start=1):
        for idx in range(offset, min(mrope_section[dim] * 3, freq_dim), 3):
            sel[idx] = dim
    return torch.tensor(sel, dtype=torch.int64)


# --------------------------------------------------------------------------
# vision tower (qwen3_vl/vision.py)
# --------------------------------------------------------------------------
def patch_embed(W, cfg: Cfg, pixel_values):
    """PatchEmbed (vision.py:69-103): nn.Conv3d(kernel = stride, bias=True) over the rows reshaped to (N, C, T, ph, pw) - restated
    as the convolution it is (fp32 accumulate, + bias, one rounding), so that fp32 runs sum in the order of the goldens"""
    v = cfg.vision
    w = W["vision_tower.patch_embed.proj.weight"]                       # (O, T, H, W, C) as the reference holds it
    x = pixel_values.reshape(-1, v.in_channels, v.temporal_patch_size, v.patch_size, v.patch_size)
    k = (v.temporal_patch_size, v.patch_size, v.patch_size)
    y = torch.nn.functional.conv3d(x.to(F32), w.permute(0, 4, 1, 2, 3).to(F32), W["vision_tower.patch_embed.proj.bias"].to(F32), stride=k)
    return y.reshape(-1, v.hidden_size).to(w.dtype)


def pos_embed_tables(cfg: Cfg, grid_thw):
    """fast_pos_embed_interpolate's index / weight lists (vision.py:299-342) in the reference's own order (image by image,
    row-major h x w, NOT yet permuted) -> (idx int64 [4, sum h w], weights float32 [4, sum h w])"""
    S = int(cfg.vision.num_position_embeddings ** 0.5)
    idx_list: List[List[int]] = [[] for _ in range(4)]
    w_list: List[List[float]] = [[] for _ in range(4)]
    for t, h, w in np.asarray(grid_thw).tolist():
        hs = torch.linspace(0, S - 1, int(h), dtype=F32)
        ws = torch.linspace(0, S - 1, int(w), dtype=F32)
        hf, wf = hs.to(torch.int32), ws.to(torch.int32)
        hc, wc = torch.clamp(hf + 1, max=S - 1), torch.clamp(wf + 1, max=S - 1)
        dh, dw = hs - hf.to(F32), ws - wf.to(F32)
        bh, bhc = hf * S, hc * S
        indices = [(bh[:, None] + wf[None, :]).flatten(), (bh[:, None] + wc[None, :]).flatten(),
                   (bhc[:, None] + wf[None, :]).flatten(), (bhc[:, None] + wc[None, :]).flatten()]
        weights = [((1 - dh)[:, None] * (1 - dw)[None, :]).flatten(), ((1 - dh)[:, None] * dw[None, :]).flatten(),
                   (dh[:, None] * (1 - dw)[None, :]).flatten(), (dh[:, None] * dw[None, :]).flatten()]
        for i in range(4):
            idx_list[i].extend(indices[i].tolist())
            w_list[i].extend(weights[i].tolist())
    return np.asarray(idx_list, dtype=np.int64), np.asarray(w_list, dtype=np.float32)


def fast_pos_embed_interpolate(W, cfg: Cfg, grid_thw):
    """vision.py:299-377: weights in the table's dtype, four typed products summed left to right, rows into merge-unit order"""
    table = W["vision_tower.pos_embed.weight"]
    T = table.dtype
    idx, wt = pos_embed_tables(cfg, grid_thw)
    wT = torch.from_numpy(wt).to(T)
    e = (table[torch.from_numpy(idx)].to(F32) * wT[:, :, None].to(F32)).to(T)
    s = ops.add(ops.add(ops.add(e[0], e[1]), e[2]), e[3])
    m = cfg.vision.spatial_merge_size
    out, off = [], 0
    for t, h, w in np.asarray(grid_thw).tolist():
        pe = s[off:off + h * w]
        off += h * w
        pe = pe.repeat(t, 1).reshape(t, h // m, m, w // m, m, -1).permute(0, 1, 3, 2, 4, 5).reshape(-1, pe.shape[-1])
        out.append(pe)
    return torch.cat(out, dim=0)


def vision_block(W, i, cfg: Cfg, x, cu_seqlens, freqs):
    """Qwen3VLMoEVisionBlock (vision.py:175-191): LayerNorm blocks, tanh-GELU MLP"""
    p = f"vision_tower.blocks.{i}."
    h = ops.layer_norm(x, W[p + "norm1.weight"], W[p + "norm1.bias"])
    x = ops.add(x, oq.vision_attention(W, p + "attn.", cfg, h, cu_seqlens, freqs))
    h = ops.layer_norm(x, W[p + "norm2.weight"], W[p + "norm2.bias"])
    h = gelu_tanh(ops.linear(h, W[p + "mlp.linear_fc1.weight"], W[p + "mlp.linear_fc1.bias"]))
    return ops.add(x, ops.linear(h, W[p + "mlp.linear_fc2.weight"], W[p + "mlp.linear_fc2.bias"]))


def patch_merger(W, p, cfg: Cfg, x, postshuffle: bool):
    """PatchMerger (vision.py:106-123): the LayerNorm runs over hidden (main merger) or over the 2 x 2 unit's 4 * hidden values
    after the reshape (use_postshuffle_norm, the DeepStack mergers)"""
    m = cfg.vision.hidden_size * cfg.vision.spatial_merge_size ** 2
    if postshuffle:
        x = ops.layer_norm(x.reshape(-1, m), W[p + "norm.weight"], W[p + "norm.bias"])
    else:
        x = ops.layer_norm(x, W[p + "norm.weight"], W[p + "norm.bias"]).reshape(-1, m)
    x = ops.gelu_erf(ops.linear(x, W[p + "linear_fc1.weight"], W[p + "linear_fc1.bias"]))
    return ops.linear(x, W[p + "linear_fc2.weight"], W[p + "linear_fc2.bias"])


def vision_tower(W, cfg: Cfg, pixel_values, grid_thw, patch_embeds=None):
    """VisionModel.__call__ (vision.py:379-425) -> (features, [tap features in block order])"""
    v = cfg.vision
    x = patch_embed(W, cfg, pixel_values) if patch_embeds is None else patch_embeds
    x = ops.add(x, fast_pos_embed_interpolate(W, cfg, grid_thw))
    freqs = ops.vision_rotary_freqs(np.asarray(grid_thw), v.hidden_size // v.num_heads, v.spatial_merge_size)
    cu = oq.vision_cu_seqlens(grid_thw).astype(np.int64)
    taps = []
    for i in range(v.depth):
        x = vision_block(W, i, cfg, x, cu, freqs)
        if i in v.deepstack_visual_indexes:
            j = v.deepstack_visual_indexes.index(i)
            taps.append(patch_merger(W, f"vision_tower.deepstack_merger_list.{j}.", cfg, x, True))
    return patch_merger(W, "vision_tower.merger.", cfg, x, False), taps


# --------------------------------------------------------------------------
# language model (qwen3_vl/language.py)
# --------------------------------------------------------------------------
def llm_attention(W, p, cfg: Cfg, x, cache, position_ids, causal: bool, rope_mode: str = "fused"):
    """Attention (language.py:40-136): bias-free projections, RMSNorm(head_dim) on every q / k head, interleaved M-RoPE"""
    t = cfg.text
    B, L, _ = x.shape
    H, Hkv, hd = t.num_attention_heads, t.num_key_value_heads, t.head_dim
    q = ops.rms_norm(ops.linear(x, W[p + "q_proj.weight"]).reshape(B, L, H, hd), W[p + "q_norm.weight"], t.rms_norm_eps).permute(0, 2, 1, 3)
    k = ops.rms_norm(ops.linear(x, W[p + "k_proj.weight"]).reshape(B, L, Hkv, hd), W[p + "k_norm.weight"], t.rms_norm_eps).permute(0, 2, 1, 3)
    v = ops.linear(x, W[p + "v_proj.weight"]).reshape(B, L, Hkv, hd).permute(0, 2, 1, 3)
    if position_ids is None:
        off = cache.offset if cache is not None else 0
        position_ids = torch.arange(off, off + L)[None, None].expand(3, B, L)
    inv = ops.mrope_inv_freq(hd, t.rope_theta)
    sel = interleaved_position_selector(t.mrope_section, hd // 2)
    q = ops.mrope_apply(q, position_ids, inv, sel, rope_mode)
    k = ops.mrope_apply(k, position_ids, inv, sel, rope_mode)
    if cache is not None:
        k, v = cache.update_and_fetch(k, v)
    if hasattr(cache, "bits"):
        from oracle import quant
        o = quant.quantized_sdpa(q, k, v, scale=hd ** -0.5, causal=causal and L > 1, group_size=cache.group_size, bits=cache.bits)
    else:
        o = ops.sdpa(q, k, v, scale=hd ** -0.5, causal=causal, q_offset=k.shape[2] - L)
    return ops.linear(o.permute(0, 2, 1, 3).reshape(B, L, -1), W[p + "o_proj.weight"])


def decoder_layer(W, i, cfg: Cfg, x, cache, position_ids, causal, rope_mode="fused"):
    """Qwen3VLDecoderLayer (language.py:139-170)"""
    p = f"language_model.model.layers.{i}."
    eps = cfg.text.rms_norm_eps
    h = ops.add(x, llm_attention(W, p + "self_attn.", cfg, ops.rms_norm(x, W[p + "input_layernorm.weight"], eps), cache,
                                 position_ids, causal, rope_mode))
    hn = ops.rms_norm(h, W[p + "post_attention_layernorm.weight"], eps)
    r = ops.linear(ops.swiglu(ops.linear(hn, W[p + "mlp.gate_proj.weight"]), ops.linear(hn, W[p + "mlp.up_proj.weight"])),
                   W[p + "mlp.down_proj.weight"])
    return ops.add(h, r)


def deepstack_process(h, visual_pos_masks, visual_embeds):
    """Qwen3VLModel._deepstack_process (language.py:250-283): per batch row, the rows at visual positions get the next
    n_visual rows of visual_embeds added (one typed add)"""
    out, offset = [], 0
    m = np.asarray(visual_pos_masks).astype(bool)
    for b in range(h.shape[0]):
        idx = np.nonzero(m[b])[0]
        hb = h[b]
        if idx.size:
            emb = visual_embeds[offset:offset + idx.size]
            offset += idx.size
            if emb.shape[0] == idx.size:
                hb = hb.clone()
                ti = torch.from_numpy(idx)
                hb[ti] = ops.add(hb[ti], emb)
        out.append(hb)
    return torch.stack(out)


def qwen3_model(W, cfg: Cfg, inputs_embeds, cache, position_ids, rope_mode="fused", visual_pos_masks=None,
                deepstack_visual_embeds=None):
    """Qwen3VLModel (language.py:173-248)"""
    h = inputs_embeds
    L = h.shape[1]
    if cache is None:
        cache = [None] * cfg.text.num_hidden_layers
    for i in range(cfg.text.num_hidden_layers):
        h = decoder_layer(W, i, cfg, h, cache[i], position_ids, causal=L > 1, rope_mode=rope_mode)
        if deepstack_visual_embeds is not None and i < len(deepstack_visual_embeds):
            h = deepstack_process(h, visual_pos_masks, deepstack_visual_embeds[i])
    return ops.rms_norm(h, W["language_model.model.norm.weight"], cfg.text.rms_norm_eps)


get_rope_index = oq.get_rope_index          # language.py:299-485 gives qwen2_vl's positions for text and images (pinned by the goldens)
lm_head = oq.lm_head
embed_tokens = oq.embed_tokens


# --------------------------------------------------------------------------
# model (qwen3_vl/qwen3_vl.py)
# --------------------------------------------------------------------------
@dataclass
class Features:
    inputs_embeds: torch.Tensor
    position_ids: np.ndarray
    rope_deltas: np.ndarray
    visual_pos_masks: Optional[np.ndarray] = None
    deepstack_visual_embeds: Optional[List[torch.Tensor]] = None
    image_features: Optional[torch.Tensor] = None


def get_input_embeddings(W, cfg: Cfg, input_ids, pixel_values=None, image_grid_thw=None, mask=None, cached_image_features=None):
    """Model.get_input_embeddings (qwen3_vl.py:44-133); cached_image_features: no DeepStack (70-79)"""
    input_ids = np.asarray(input_ids)
    emb = embed_tokens(W, input_ids)
    if pixel_values is None and cached_image_features is None:
        pos, deltas = get_rope_index(cfg, input_ids, attention_mask=mask)
        return Features(emb, pos, deltas)
    taps = None
    if cached_image_features is not None:
        feats = cached_image_features
    else:
        dtype = W["vision_tower.patch_embed.proj.weight"].dtype
        feats, taps = vision_tower(W, cfg, pixel_values.to(dtype), image_grid_thw)
    vmask = (input_ids == cfg.image_token_id) | (input_ids == cfg.video_token_id)
    emb = emb.clone()
    emb[torch.from_numpy(vmask)] = feats.to(emb.dtype)
    pos, deltas = get_rope_index(cfg, input_ids, image_grid_thw, None, mask)
    return Features(emb, pos, deltas, vmask, taps, feats)


def _pos3(pos):
    pos = np.asarray(pos)
    if pos.ndim == 2:
        pos = np.broadcast_to(pos[None], (3,) + pos.shape)
    return torch.from_numpy(np.ascontiguousarray(pos))


def prefill_logits(W, cfg: Cfg, input_ids, pixel_values=None, image_grid_thw=None, rope_mode: str = "fused",
                   cached_image_features=None, return_features: bool = False):
    """logits of every prompt row, no cache -> [L, V]"""
    f = get_input_embeddings(W, cfg, input_ids, pixel_values, image_grid_thw, cached_image_features=cached_image_features)
    h = qwen3_model(W, cfg, f.inputs_embeds, None, _pos3(f.position_ids), rope_mode, f.visual_pos_masks, f.deepstack_visual_embeds)
    out = lm_head(W, cfg, h)[0]
    return (out, f) if return_features else out


def _prefill_with_cache(W, cfg, input_ids, pixel_values, image_grid_thw, rope_mode, max_kv_size=None):
    f = get_input_embeddings(W, cfg, input_ids, pixel_values, image_grid_thw)
    cache = oq._make_prompt_cache(cfg, max_kv_size)
    h = qwen3_model(W, cfg, f.inputs_embeds, cache, _pos3(f.position_ids), rope_mode, f.visual_pos_masks, f.deepstack_visual_embeds)
    return f, cache, h


def generate_greedy(W, cfg: Cfg, input_ids, pixel_values=None, image_grid_thw=None, max_tokens: int = 16,
                    return_logits: bool = False, rope_mode: str = "fused"):
    """generate_step at temperature 0: prefill with DeepStack, then decode steps at pos = cache offset + rope delta without it"""
    input_ids = np.asarray(input_ids)
    assert input_ids.shape[0] == 1
    f, cache, h = _prefill_with_cache(W, cfg, input_ids, pixel_values, image_grid_thw, rope_mode)
    logits = lm_head(W, cfg, h)[:, -1, :]
    toks, all_logits = [], []
    delta = int(np.asarray(f.rope_deltas)[0, 0])
    for n in range(max_tokens):
        lp = ops.logprobs_from_logits(logits)
        y = int(ops.argmax_first(lp)[0])
        toks.append(y)
        all_logits.append(logits[0].clone())
        if n == max_tokens - 1:
            break
        pid = torch.full((3, 1, 1), oq._cache_offset(cache[0]) + delta, dtype=torch.long)
        h = qwen3_model(W, cfg, embed_tokens(W, np.array([[y]])), cache, pid, rope_mode)
        logits = lm_head(W, cfg, h)[:, -1, :]
    return (toks, torch.stack(all_logits)) if return_logits else toks


def decode_teacher_forced(W, cfg: Cfg, input_ids, pixel_values=None, image_grid_thw=None, forced_tokens=(),
                          rope_mode: str = "fused", kv_bits=None, kv_group_size: int = 64, quantized_kv_start: int = 0,
                          max_kv_size: Optional[int] = None):
    """-> logits [1 + len(forced_tokens), V]: row 0 = last prompt row, row i = after feeding forced_tokens[i - 1]"""
    from oracle import quant

    input_ids = np.asarray(input_ids)
    f, cache, h = _prefill_with_cache(W, cfg, input_ids, pixel_values, image_grid_thw, rope_mode, max_kv_size)
    quant.maybe_quantize_kv_cache(cache, quantized_kv_start, kv_group_size, kv_bits)
    rows = [lm_head(W, cfg, h[:, -1:, :])[0, 0]]
    delta = int(np.asarray(f.rope_deltas)[0, 0])
    for y in forced_tokens:
        pid = torch.full((3, 1, 1), oq._cache_offset(cache[0]) + delta, dtype=torch.long)
        h = qwen3_model(W, cfg, embed_tokens(W, np.array([[int(y)]])), cache, pid, rope_mode)
        quant.maybe_quantize_kv_cache(cache, quantized_kv_start, kv_group_size, kv_bits)
        rows.append(lm_head(W, cfg, h)[0, -1])
    return torch.stack(rows)


def qknorm_rope(qkv, cfg_heads, pos3, inv_freq, mrope_section, q_norm_w, k_norm_w, eps, interleaved: bool = True):
    """What the QK-norm rotary kernel computes on token-major rows qkv [T, (Hq + 2 Hkv) * D] (fused mode) -> the new rows
    (v columns unchanged).  pos3 int [3, T]."""
    Hq, Hkv, D = cfg_heads
    T = qkv.shape[0]
    q = qkv[:, :Hq * D].reshape(T, Hq, D)
    k = qkv[:, Hq * D:(Hq + Hkv) * D].reshape(T, Hkv, D)
    sel = interleaved_position_selector(mrope_section, D // 2) if interleaved else ops.chunked_position_selector(mrope_section, D // 2)
    pid = torch.as_tensor(np.asarray(pos3), dtype=torch.long).reshape(3, 1, T)
    q = ops.mrope_apply(ops.rms_norm(q, q_norm_w, eps).permute(1, 0, 2)[None], pid, inv_freq, sel, "fused")[0].permute(1, 0, 2)
    k = ops.mrope_apply(ops.rms_norm(k, k_norm_w, eps).permute(1, 0, 2)[None], pid, inv_freq, sel, "fused")[0].permute(1, 0, 2)
    return torch.cat([q.reshape(T, -1), k.reshape(T, -1), qkv[:, (Hq + Hkv) * D:]], dim=1)


def synth_request(cfg: Cfg, grids, n_text: int = 12, seed: int = 0):
    """A prompt over images GIVEN AS GRIDS -> (input_ids [1, L] int64, pixel_values f32 [N, C*T*ps*ps] uniform in [-1, 1),
    grid_thw int64 [n, 3]); text ids stay below 1000"""
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
# product-model construction
# --------------------------------------------------------------------------
def model_config_dict(cfg: Cfg, quantization=None) -> dict:
    t, v = cfg.text, cfg.vision
    d = dict(
        model_type="qwen3_vl", image_token_id=cfg.image_token_id, video_token_id=cfg.video_token_id,
        vision_start_token_id=cfg.vision_start_token_id, vision_end_token_id=cfg.vision_start_token_id + 1,
        tie_word_embeddings=t.tie_word_embeddings,
        text_config=dict(model_type="qwen3_vl_text", hidden_size=t.hidden_size, num_hidden_layers=t.num_hidden_layers,
                         intermediate_size=t.intermediate_size, num_attention_heads=t.num_attention_heads,
                         num_key_value_heads=t.num_key_value_heads, head_dim=t.head_dim, rms_norm_eps=t.rms_norm_eps,
                         vocab_size=t.vocab_size, rope_theta=t.rope_theta, max_position_embeddings=32768,
                         rope_scaling={"rope_type": "default", "mrope_section": list(t.mrope_section), "mrope_interleaved": True},
                         tie_word_embeddings=t.tie_word_embeddings, attention_bias=False),
        vision_config=dict(model_type="qwen3_vl", depth=v.depth, hidden_size=v.hidden_size, intermediate_size=v.intermediate_size,
                           out_hidden_size=v.out_hidden_size, num_heads=v.num_heads, patch_size=v.patch_size,
                           in_channels=v.in_channels, spatial_merge_size=v.spatial_merge_size,
                           temporal_patch_size=v.temporal_patch_size, num_position_embeddings=v.num_position_embeddings,
                           deepstack_visual_indexes=list(v.deepstack_visual_indexes)))
    if quantization:
        d["quantization"] = quantization
    return d


def to_hf_keys(W):
    """the inverse of Model.sanitize + VisionModel.sanitize: HF Qwen3-VL key names, conv weight (O, C, T, H, W)"""
    hf = {}
    for k, w in W.items():
        w = w.contiguous()
        if k.startswith("vision_tower."):
            hk = "model.visual." + k[len("vision_tower."):]
            if "patch_embed.proj.weight" in k:
                w = w.permute(0, 4, 1, 2, 3).contiguous()
        elif k.startswith("language_model.model."):
            hk = "model.language_model." + k[len("language_model.model."):]
        else:
            hk = "lm_head." + k[len("language_model.lm_head."):]
        hf[hk] = w
    return hf


def write_checkpoint(path, cfg: Cfg, W, quantization=None):
    """HF Qwen3-VL layout on disk: config.json (text_config / vision_config nested), model.safetensors under the HF key names, a
    WordLevel tokenizer with the vision tokens, preprocessor_config.json."""
    import json

    from safetensors.torch import save_file
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast

    conf = model_config_dict(cfg, quantization)
    conf["eos_token_id"] = [1]
    (path / "config.json").write_text(json.dumps(conf))
    save_file(to_hf_keys(W), str(path / "model.safetensors"))
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
    (path / "preprocessor_config.json").write_text(json.dumps(dict(image_mean=[0.5] * 3, image_std=[0.5] * 3, patch_size=16,
                                                                  merge_size=2, temporal_patch_size=2)))


def build_product_model(cfg: Cfg, W, device="cuda", **kw):
    from mlx_vlm_amd.models.qwen3_vl import Model, ModelConfig

    m = Model(ModelConfig.from_dict(model_config_dict(cfg)), device=device, **kw)
    m.load_weights(W)
    return m
