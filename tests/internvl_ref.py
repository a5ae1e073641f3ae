"""Torch restatement of mlx_vlm.models.internvl_chat (TEST HELPER, not a test), in the style of tests/qwen3_vl_ref.py.

Follows the reference's internvl_chat/{vision,language,internvl_chat}.py function by function on torch-CPU tensors, every op's
bf16 rounding through oracle.ops.  Weights: a flat dict under the checkpoint's own names (`vision_model.*`, `mlp1.{0,1,3}.*`,
`language_model.model.*`, `language_model.lm_head.weight`).  Pinned to the reference itself by
tests/golden/internvl_tiny_ref.npz (bit-exact in bf16 and fp32; tests/test_internvl_cpu.py).

The typed graph of the layer scale (vision.py:126-132), the thing this family adds to the encoder layer:

    x = T(x + T(proj(..) * ls1))          proj(..) = T(acc + bias): three roundings behind the accumulator

The vision MLP's `nn.GELU(approx="precise")` is MLX's tanh approximation (tests/qwen3_vl_ref.py::gelu_tanh); `act="erf"` is the
exact form the original InternViT (and transformers) computes.  mlp1's `nn.GELU()` is the erf form.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

from oracle import ops
from tests.qwen3_vl_ref import gelu_tanh, interleaved_position_selector

F32 = torch.float32


@dataclass
class VisionCfg:
    hidden_size: int = 1024
    num_attention_heads: int = 16
    patch_size: int = 14
    num_hidden_layers: int = 24
    intermediate_size: int = 4096
    image_size: int = 448
    num_channels: int = 3
    layer_norm_eps: float = 1e-6

    @property
    def grid(self):
        return self.image_size // self.patch_size

    @property
    def num_patches(self):
        return self.grid ** 2


@dataclass
class TextCfg:
    model_type: str = "qwen2"
    hidden_size: int = 1536
    num_hidden_layers: int = 28
    intermediate_size: int = 8960
    num_attention_heads: int = 12
    num_key_value_heads: int = 2
    head_dim: Optional[int] = None
    vocab_size: int = 151674
    rms_norm_eps: float = 1e-6
    rope_theta: float = 1000000.0
    tie_word_embeddings: bool = False

    @property
    def attention_bias(self):
        return self.model_type == "qwen2"

    @property
    def hd(self):
        return self.head_dim or self.hidden_size // self.num_attention_heads


@dataclass
class Cfg:
    text: TextCfg = field(default_factory=TextCfg)
    vision: VisionCfg = field(default_factory=VisionCfg)
    image_token_index: int = 151667
    video_token_index: int = 151656
    downsample_ratio: float = 0.5

    @property
    def tokens_per_tile(self):
        return int(self.vision.num_patches * self.downsample_ratio ** 2)


def tiny_cfg(lm: str = "qwen2") -> Cfg:
    """tower: depth 2, hidden 128, 2 heads of 64, intermediate 256, image 56 / patch 14 -> 17 tokens per tile, 4 behind the shuffle.
    Language model, 2 layers: qwen2 = 4 : 2 heads of 64 over hidden 256 with bias (the spread into 128-wide slots), qwen3 = 4 : 2
    heads of 128 over hidden 256 (n_heads * head_dim != hidden) with QK-norm."""
    v = VisionCfg(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256, image_size=56)
    t = TextCfg(model_type=lm, hidden_size=256, num_hidden_layers=2, intermediate_size=512, num_attention_heads=4,
                num_key_value_heads=2, head_dim=128 if lm == "qwen3" else None, vocab_size=1024)
    return Cfg(text=t, vision=v, image_token_index=1001, video_token_index=1002)


def random_weights(cfg: Cfg, seed: int = 0, dtype=torch.bfloat16, std: float = 0.05, embed_std: float = 0.2,
                   tower_only: bool = False) -> Dict[str, torch.Tensor]:
    """Synthetic checkpoint: Linear / Embedding ~ N(0, std^2), norm weights 1 + noise, biases small noise, ls1 / ls2 uniform in
    [0.05, 0.5] (with ls = 1 the layer scale would be invisible)."""
    g = torch.Generator().manual_seed(seed)
    W: Dict[str, torch.Tensor] = {}

    def rn(*shape, s=std):
        return (torch.randn(*shape, generator=g) * s).to(dtype)

    def near1(n, s=0.05):
        return (1 + rn(n, s=s).float()).to(dtype)

    v = cfg.vision
    E, I = v.hidden_size, v.intermediate_size
    V = "vision_model."
    W[V + "embeddings.class_embedding"] = rn(1, 1, E, s=0.5)
    W[V + "embeddings.position_embedding"] = rn(1, v.num_patches + 1, E, s=0.3)
    W[V + "embeddings.patch_embedding.weight"] = rn(E, v.patch_size, v.patch_size, v.num_channels)
    W[V + "embeddings.patch_embedding.bias"] = rn(E, s=0.1)
    for i in range(v.num_hidden_layers):
        p = f"{V}encoder.layers.{i}."
        for n in ("norm1", "norm2"):
            W[p + n + ".weight"] = near1(E)
            W[p + n + ".bias"] = rn(E)
        W[p + "attn.qkv.weight"], W[p + "attn.qkv.bias"] = rn(3 * E, E, s=0.1), rn(3 * E, s=0.1)
        W[p + "attn.proj.weight"], W[p + "attn.proj.bias"] = rn(E, E, s=0.1), rn(E, s=0.1)
        W[p + "mlp.fc1.weight"], W[p + "mlp.fc1.bias"] = rn(I, E, s=0.1), rn(I, s=0.1)
        W[p + "mlp.fc2.weight"], W[p + "mlp.fc2.bias"] = rn(E, I, s=0.1), rn(E, s=0.1)
        for n in ("ls1", "ls2"):
            W[p + n] = (0.05 + 0.45 * torch.rand(E, generator=g)).to(dtype)
    M = E * int(round(1 / cfg.downsample_ratio)) ** 2
    D = cfg.text.hidden_size
    W["mlp1.0.weight"], W["mlp1.0.bias"] = near1(M), rn(M)
    W["mlp1.1.weight"], W["mlp1.1.bias"] = rn(D, M), rn(D, s=0.1)
    W["mlp1.3.weight"], W["mlp1.3.bias"] = rn(D, D), rn(D, s=0.1)
    if tower_only:
        return W
    t = cfg.text
    hd, H, Hkv = t.hd, t.num_attention_heads, t.num_key_value_heads
    LM = "language_model.model."
    W[LM + "embed_tokens.weight"] = rn(t.vocab_size, D, s=embed_std)
    for i in range(t.num_hidden_layers):
        p = f"{LM}layers.{i}."
        W[p + "input_layernorm.weight"] = near1(D)
        W[p + "post_attention_layernorm.weight"] = near1(D)
        for n, rows in (("q_proj", H * hd), ("k_proj", Hkv * hd), ("v_proj", Hkv * hd)):
            W[p + f"self_attn.{n}.weight"] = rn(rows, D)
            if t.attention_bias:
                W[p + f"self_attn.{n}.bias"] = rn(rows, s=0.1)
        W[p + "self_attn.o_proj.weight"] = rn(D, H * hd)
        if not t.attention_bias:
            W[p + "self_attn.q_norm.weight"] = near1(hd, s=0.1)
            W[p + "self_attn.k_norm.weight"] = near1(hd, s=0.1)
        W[p + "mlp.gate_proj.weight"] = rn(t.intermediate_size, D)
        W[p + "mlp.up_proj.weight"] = rn(t.intermediate_size, D)
        W[p + "mlp.down_proj.weight"] = rn(D, t.intermediate_size)
    W[LM + "norm.weight"] = near1(D)
    if not t.tie_word_embeddings:
        W["language_model.lm_head.weight"] = rn(t.vocab_size, D, s=embed_std)
    return W


# --------------------------------------------------------------------------
# vision tower (internvl_chat/vision.py)
# --------------------------------------------------------------------------
def mul(a, b):
    """a * b in T (vision.py:128,130: the layer scale)"""
    return (a.to(F32) * b.to(F32)).to(ops._result_type(a, b))


def layerscale_epilogue(a, w, bias, ls, res, acc_dtype=F32):
    """What VLM_EPI_BIAS | VLM_EPI_RESIDUAL | VLM_EPI_LAYERSCALE computes: res + ls * Linear(a), as the typed graph rounds it
    (fp32 accumulate, then the three roundings).  acc_dtype=float64: the accumulator in double, for inputs whose sums are exact."""
    T = a.dtype
    y = (a.to(acc_dtype) @ w.to(acc_dtype).T + bias.to(acc_dtype)).to(F32).to(T)
    return ops.add(res, mul(y, ls))


def lattice_operands(M: int, N: int, K: int, seed: int = 0, dtype=torch.bfloat16):
    """Operands on which every sum of the layer-scale GEMM is EXACT whatever its order: A in {-4 .. 4}, W in {-2 .. 2} (|acc| <=
    8 K <= 32768 at K = 4096: integers below 2^24, exact in fp32 in any grouping), bias an integer in [-8, 8] - so acc + bias is an
    integer below 2^16; ls a power of two in {1/4, 1/2, 1, 2}; res an integer in [-16, 16].  The roundings to bf16 are then the
    only inexact steps, and they are the same in every implementation that rounds at the same three points.  (Scaling by a
    power of two commutes with rounding, so the first two roundings act as one here; that one - integers above 256 - and the
    last show on these operands, the random-operand tests see all three.)"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-4, 5, (M, K), generator=g).to(dtype)
    w = torch.randint(-2, 3, (N, K), generator=g).to(dtype)
    bias = torch.randint(-8, 9, (N,), generator=g).to(dtype)
    ls = (2.0 ** torch.randint(-2, 2, (N,), generator=g).float()).to(dtype)
    res = torch.randint(-16, 17, (M, N), generator=g).to(dtype)
    return a, w, bias, ls, res


def vision_embeddings(W, cfg: Cfg, pixel_values, conv: bool = True):
    """VisionEmbeddings (vision.py:202-222), pixel_values [B, 3, S, S] at the native size (where `interpolate` is the identity).
    conv=True restates the Conv2d as the convolution it is (fp32 sums in the order of the goldens), conv=False as the GEMM over
    (kH, kW, C)-major patches the engine runs."""
    v = cfg.vision
    V = "vision_model.embeddings."
    w, b = W[V + "patch_embedding.weight"], W[V + "patch_embedding.bias"]
    B = pixel_values.shape[0]
    assert tuple(pixel_values.shape[2:]) == (v.image_size, v.image_size)
    if conv:
        y = torch.nn.functional.conv2d(pixel_values.to(F32), w.permute(0, 3, 1, 2).to(F32), b.to(F32), stride=v.patch_size)
        y = y.flatten(2).transpose(1, 2).to(ops._result_type(pixel_values, w))                  # [B, P, E], row-major (h, w)
    else:
        P, G = v.patch_size, v.grid
        x = pixel_values.permute(0, 2, 3, 1).reshape(B, G, P, G, P, v.num_channels).permute(0, 1, 3, 2, 4, 5)
        y = ops.linear(x.reshape(B, G * G, -1), w.reshape(w.shape[0], -1), b)
    cls = W[V + "class_embedding"].expand(B, 1, -1).to(w.dtype)
    return ops.add(torch.cat([cls, y], dim=1), W[V + "position_embedding"])


def encoder_layer(W, i: int, cfg: Cfg, x, act: str = "tanh"):
    """EncoderLayer (vision.py:97-132) with Attention (27-80) and MLP (83-94)"""
    v = cfg.vision
    p = f"vision_model.encoder.layers.{i}."
    B, L, E = x.shape
    H = v.num_attention_heads
    y = ops.layer_norm(x, W[p + "norm1.weight"], W[p + "norm1.bias"], v.layer_norm_eps)
    qkv = ops.linear(y, W[p + "attn.qkv.weight"], W[p + "attn.qkv.bias"]).reshape(B, L, 3, H, E // H).permute(2, 0, 3, 1, 4)
    o = ops.sdpa(qkv[0], qkv[1], qkv[2], scale=(E // H) ** -0.5).permute(0, 2, 1, 3).reshape(B, L, E)
    x = ops.add(x, mul(ops.linear(o, W[p + "attn.proj.weight"], W[p + "attn.proj.bias"]), W[p + "ls1"]))
    y = ops.layer_norm(x, W[p + "norm2.weight"], W[p + "norm2.bias"], v.layer_norm_eps)
    y = ops.linear(y, W[p + "mlp.fc1.weight"], W[p + "mlp.fc1.bias"])
    y = gelu_tanh(y) if act == "tanh" else ops.gelu_erf(y)
    return ops.add(x, mul(ops.linear(y, W[p + "mlp.fc2.weight"], W[p + "mlp.fc2.bias"]), W[p + "ls2"]))


def vision_tower(W, cfg: Cfg, pixel_values, embeddings=None, act: str = "tanh", conv: bool = True):
    """VisionModel (vision.py:225-245) -> last hidden state [B, 1 + P, E]"""
    x = vision_embeddings(W, cfg, pixel_values, conv) if embeddings is None else embeddings
    for i in range(cfg.vision.num_hidden_layers):
        x = encoder_layer(W, i, cfg, x, act)
    return x


def pixel_shuffle(x, shuffle_ratio: float):
    """models/base.py:436-458"""
    B, N, _ = x.shape
    g = int(math.sqrt(N))
    x = x.reshape(B, g, g, -1)
    B, h, w, c = x.shape
    x = x.reshape(B, h, int(w * shuffle_ratio), int(c / shuffle_ratio)).permute(0, 2, 1, 3)
    x = x.reshape(B, int(h * shuffle_ratio), int(w * shuffle_ratio), int(c / shuffle_ratio ** 2)).permute(0, 2, 1, 3)
    return x.reshape(B, -1, x.shape[-1])


def connector(W, cfg: Cfg, hidden):
    """internvl_chat.py:65-75: drop CLS, pixel shuffle, mlp1 = LayerNorm (eps 1e-5, nn.LayerNorm's default) -> Linear -> GELU -> Linear"""
    x = pixel_shuffle(hidden[:, 1:, :], cfg.downsample_ratio)
    x = ops.layer_norm(x, W["mlp1.0.weight"], W["mlp1.0.bias"], 1e-5)
    x = ops.gelu_erf(ops.linear(x, W["mlp1.1.weight"], W["mlp1.1.bias"]))
    return ops.linear(x, W["mlp1.3.weight"], W["mlp1.3.bias"])


def image_features(W, cfg: Cfg, pixel_values, act: str = "tanh", conv: bool = True):
    """-> [tiles * tokens_per_tile, D]"""
    dtype = W["vision_model.embeddings.patch_embedding.weight"].dtype
    f = connector(W, cfg, vision_tower(W, cfg, pixel_values.to(dtype), act=act, conv=conv))
    return f.reshape(-1, f.shape[-1])


# --------------------------------------------------------------------------
# language model (internvl_chat/language.py)
# --------------------------------------------------------------------------
def attention(W, p: str, cfg: Cfg, x, cache, selector=None):
    """Attention (language.py:17-90): q / k / v with bias XOR RMSNorm(head_dim) on every q / k head, nn.RoPE (mx.fast.rope: fp32
    angles and rotation, one rounding) at offset = cache.offset, KVCache, causal SDPA, o_proj.  `selector`: run the rotation as
    M-RoPE with that frequency -> axis table and the same position on all three axes (what the engine does)."""
    t = cfg.text
    B, L, _ = x.shape
    H, Hkv, hd = t.num_attention_heads, t.num_key_value_heads, t.hd

    def proj(n, heads):
        y = ops.linear(x, W[p + n + "_proj.weight"], W.get(p + n + "_proj.bias")).reshape(B, L, heads, hd)
        if not t.attention_bias and n in ("q", "k"):
            y = ops.rms_norm(y, W[p + n + "_norm.weight"], t.rms_norm_eps)
        return y.permute(0, 2, 1, 3)

    q, k, v = proj("q", H), proj("k", Hkv), proj("v", Hkv)
    off = cache.offset if cache is not None else 0
    pos = torch.arange(off, off + L)[None].expand(B, L)
    inv = ops.mrope_inv_freq(hd, t.rope_theta)
    if selector is not None:
        pos = pos[None].expand(3, B, L)
    q = ops.mrope_apply(q, pos, inv, selector, "fused")
    k = ops.mrope_apply(k, pos, inv, selector, "fused")
    if cache is not None:
        k, v = cache.update_and_fetch(k, v)
    if hasattr(cache, "bits"):
        from oracle import quant

        o = quant.quantized_sdpa(q, k, v, scale=hd ** -0.5, causal=L > 1, group_size=cache.group_size, bits=cache.bits)
    else:
        o = ops.sdpa(q, k, v, scale=hd ** -0.5, causal=L > 1, q_offset=k.shape[2] - L)
    return ops.linear(o.permute(0, 2, 1, 3).reshape(B, L, -1), W[p + "o_proj.weight"])


def decoder_layer(W, i: int, cfg: Cfg, x, cache, selector=None):
    """Qwen2VLDecoderLayer (language.py:93-116)"""
    p = f"language_model.model.layers.{i}."
    eps = cfg.text.rms_norm_eps
    h = ops.add(x, attention(W, p + "self_attn.", cfg, ops.rms_norm(x, W[p + "input_layernorm.weight"], eps), cache, selector))
    hn = ops.rms_norm(h, W[p + "post_attention_layernorm.weight"], eps)
    act = ops.swiglu(ops.linear(hn, W[p + "mlp.gate_proj.weight"]), ops.linear(hn, W[p + "mlp.up_proj.weight"]))
    return ops.add(h, ops.linear(act, W[p + "mlp.down_proj.weight"]))


def lm_head(W, cfg: Cfg, h):
    t = cfg.text
    return ops.linear(h, W["language_model.model.embed_tokens.weight"] if t.tie_word_embeddings else W["language_model.lm_head.weight"])


def language_model(W, cfg: Cfg, inputs_embeds, cache=None, selector=None, last_only: bool = False):
    """Qwen2Model + head (language.py:119-181) -> logits [B, L, V] (last_only: [B, 1, V], the same values for that row)"""
    h = inputs_embeds
    cache = cache or [None] * cfg.text.num_hidden_layers
    for i in range(cfg.text.num_hidden_layers):
        h = decoder_layer(W, i, cfg, h, cache[i], selector)
    if last_only:
        h = h[:, -1:, :]
    return lm_head(W, cfg, ops.rms_norm(h, W["language_model.model.norm.weight"], cfg.text.rms_norm_eps))


def embed_tokens(W, input_ids):
    """nn.Embedding; nn.QuantizedEmbedding for a 4-bit checkpoint (dequantize of the rows)"""
    e = W["language_model.model.embed_tokens.weight"]
    idx = torch.as_tensor(np.asarray(input_ids), dtype=torch.long)
    return e.rows(idx) if hasattr(e, "wq") else e[idx]


# --------------------------------------------------------------------------
# model (internvl_chat/internvl_chat.py)
# --------------------------------------------------------------------------
def get_input_embeddings(W, cfg: Cfg, input_ids, pixel_values=None, cached_image_features=None, image_token_index=None,
                         act: str = "tanh", conv: bool = True):
    """Model.get_input_embeddings (internvl_chat.py:34-107) -> [B, L, D]"""
    ids = np.asarray(input_ids)
    emb = embed_tokens(W, ids)
    if pixel_values is None and cached_image_features is None:
        return emb
    feats = cached_image_features if cached_image_features is not None else image_features(W, cfg, pixel_values, act, conv)
    where = ids == (cfg.image_token_index if image_token_index is None else image_token_index)
    if where.sum() == 0:
        where = ids == cfg.video_token_index
    emb = emb.clone()
    emb[torch.from_numpy(where)] = feats.reshape(-1, feats.shape[-1]).to(emb.dtype)
    return emb


def prefill_logits(W, cfg: Cfg, input_ids, pixel_values=None, **kw):
    """logits of every prompt row, no cache -> [L, V]"""
    return language_model(W, cfg, get_input_embeddings(W, cfg, input_ids, pixel_values, **kw))[0]


def generate_greedy(W, cfg: Cfg, input_ids, pixel_values=None, max_tokens: int = 8, return_logits: bool = False, **kw):
    ids = np.asarray(input_ids)
    assert ids.shape[0] == 1
    cache = [ops.KVCache() for _ in range(cfg.text.num_hidden_layers)]
    logits = language_model(W, cfg, get_input_embeddings(W, cfg, ids, pixel_values, **kw), cache, last_only=True)[:, -1, :]
    toks, rows = [], []
    for n in range(max_tokens):
        y = int(ops.argmax_first(ops.logprobs_from_logits(logits))[0])
        toks.append(y)
        rows.append(logits[0].clone())
        if n == max_tokens - 1:
            break
        logits = language_model(W, cfg, embed_tokens(W, np.array([[y]])), cache)[:, -1, :]
    return (toks, torch.stack(rows)) if return_logits else toks


def decode_teacher_forced(W, cfg: Cfg, input_ids, pixel_values=None, forced_tokens=(), kv_bits=None, kv_group_size: int = 64,
                          quantized_kv_start: int = 0, **kw):
    """-> logits [1 + len(forced_tokens), V]: row 0 = last prompt row, row i = after feeding forced_tokens[i - 1]"""
    from oracle import quant

    ids = np.asarray(input_ids)
    assert ids.shape[0] == 1
    cache = [ops.KVCache() for _ in range(cfg.text.num_hidden_layers)]
    rows = [language_model(W, cfg, get_input_embeddings(W, cfg, ids, pixel_values, **kw), cache, last_only=True)[0, 0]]
    quant.maybe_quantize_kv_cache(cache, quantized_kv_start, kv_group_size, kv_bits)
    for y in forced_tokens:
        rows.append(language_model(W, cfg, embed_tokens(W, np.array([[int(y)]])), cache)[0, -1])
        quant.maybe_quantize_kv_cache(cache, quantized_kv_start, kv_group_size, kv_bits)
    return torch.stack(rows)


def synth_request(cfg: Cfg, tiles_per_image, n_text: int = 12, seed: int = 0):
    """A prompt over images GIVEN AS TILE COUNTS -> (input_ids [1, L] int64, pixel_values f32 [tiles, 3, S, S] uniform in
    [-1, 1) or None); text ids stay below 1000, <img> / </img> are image_token_index + 2 / + 3"""
    rng = np.random.default_rng(seed)
    v = cfg.vision
    ids: List[int] = rng.integers(3, 1000, 3).tolist()
    n_tiles = int(sum(tiles_per_image))
    for n in tiles_per_image:
        ids += [cfg.image_token_index + 2] + [cfg.image_token_index] * (cfg.tokens_per_tile * int(n)) + [cfg.image_token_index + 3]
        ids += rng.integers(3, 1000, 2).tolist()
    ids += rng.integers(3, 1000, n_text).tolist()
    pix = rng.uniform(-1.0, 1.0, (n_tiles, v.num_channels, v.image_size, v.image_size)).astype(np.float32) if n_tiles else None
    return np.array([ids], dtype=np.int64), pix


# --------------------------------------------------------------------------
# product-model construction
# --------------------------------------------------------------------------
def model_config_dict(cfg: Cfg, quantization=None) -> dict:
    t, v = cfg.text, cfg.vision
    text = dict(model_type=t.model_type, hidden_size=t.hidden_size, num_hidden_layers=t.num_hidden_layers,
                intermediate_size=t.intermediate_size, num_attention_heads=t.num_attention_heads,
                num_key_value_heads=t.num_key_value_heads, rms_norm_eps=t.rms_norm_eps, vocab_size=t.vocab_size,
                rope_theta=t.rope_theta, tie_word_embeddings=t.tie_word_embeddings, attention_bias=t.attention_bias)
    if t.head_dim:
        text["head_dim"] = t.head_dim
    d = dict(model_type="internvl_chat", image_token_index=cfg.image_token_index, video_token_index=cfg.video_token_index,
             downsample_ratio=cfg.downsample_ratio, text_config=text,
             vision_config=dict(model_type="intern_vit_6b", hidden_size=v.hidden_size, num_attention_heads=v.num_attention_heads,
                                patch_size=v.patch_size, num_hidden_layers=v.num_hidden_layers,
                                intermediate_size=v.intermediate_size, image_size=v.image_size, num_channels=v.num_channels,
                                layer_norm_eps=v.layer_norm_eps, qkv_bias=True, qk_normalization=False, norm_type="layer_norm"))
    if quantization:
        d["quantization"] = quantization
    return d


def to_hf_keys(W):
    """the checkpoint layout on disk: the same names, the conv weight in torch layout (O, C, kH, kW)"""
    return {k: (w.permute(0, 3, 1, 2) if k.endswith("patch_embedding.weight") else w).contiguous() for k, w in W.items()}


def write_checkpoint(path, cfg: Cfg, W, quantization=None):
    """config.json (+ the tiling keys the processor reads), model.safetensors, a WordLevel tokenizer with the image tokens"""
    import json

    from safetensors.torch import save_file
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast

    conf = model_config_dict(cfg, quantization)
    conf.update(eos_token_id=[1], max_dynamic_patch=4, min_dynamic_patch=1, use_thumbnail=True)
    (path / "config.json").write_text(json.dumps(conf))
    save_file(to_hf_keys(W), str(path / "model.safetensors"))
    vocab = {f"t{i}": i for i in range(cfg.text.vocab_size)}
    special = (("<unk>", 0), ("<eos>", 1), ("<pad>", 2), ("<IMG_CONTEXT>", cfg.image_token_index),
               ("<img>", cfg.image_token_index + 2), ("</img>", cfg.image_token_index + 3))
    for name, idx in special:
        del vocab[f"t{idx}"]
        vocab[name] = idx
    tok = Tokenizer(models.WordLevel(vocab, unk_token="<unk>"))
    tok.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    fast = PreTrainedTokenizerFast(tokenizer_object=tok, eos_token="<eos>", pad_token="<pad>", unk_token="<unk>")
    fast.add_special_tokens({"additional_special_tokens": ["<IMG_CONTEXT>", "<img>", "</img>"]})
    fast.save_pretrained(str(path))


def build_product_model(cfg: Cfg, W, device="cuda", **kw):
    from mlx_vlm_amd.models.internvl_chat import Model, ModelConfig

    m = Model(ModelConfig.from_dict(model_config_dict(cfg)), device=device, **kw)
    m.load_weights(W)
    return m
