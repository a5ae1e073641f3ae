"""The first form's separate-rope path of vlm_vit_forward on the GPU: a plain qkv GEMM + bias followed by vlm_rope2d_vision,
taken by a Qwen2-VL tower loaded under VLM_VIT_ROPE_FUSED=0 (or at a head_dim that is no multiple of 16)."""
import pytest
import torch

from oracle import qwen2_vl as oq
from tests.helpers import build_product_model, synth_request

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _rel_rms_err(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30))


def test_vision_tower_separate_rope_vs_oracle(monkeypatch):
    """config, weights, seed and request of test_engine_gpu.test_vision_tower_vs_oracle, and its bar for two blocks + merger:
    relative rms < 2e-2 (measured: 0.0055 on either rope path)."""
    cfg = oq.tiny_cfg()
    W = oq.random_weights(cfg, seed=1234, dtype=BF, std=0.05, embed_std=0.2)
    monkeypatch.setenv("VLM_VIT_ROPE_FUSED", "0")
    plain = build_product_model(cfg, W, kv_pool_tokens=2048, max_seqs=4).vision_tower
    assert plain.rope_fused is False
    monkeypatch.delenv("VLM_VIT_ROPE_FUSED")
    fused = build_product_model(cfg, W, kv_pool_tokens=2048, max_seqs=4).vision_tower
    assert fused.rope_fused is True
    # not vacuous: the fused tower holds the q / k rows interleaved, this one as the checkpoint has them
    name = "blocks.0.attn.qkv.weight"
    assert plain._w[name].shape == fused._w[name].shape and not torch.equal(plain._w[name], fused._w[name])

    _, pix, thw = synth_request(cfg, [(56, 84), (112, 56)], seed=3)
    ref = oq.vision_tower(W, cfg, torch.from_numpy(pix).to(BF), thw)
    out = plain(torch.from_numpy(pix), thw)
    assert out.shape == ref.shape
    e, ef = _rel_rms_err(out, ref), _rel_rms_err(fused(torch.from_numpy(pix), thw), ref)
    print(f"separate rope: rel-rms {e:.4f}; rope in the GEMM epilogue: {ef:.4f}")
    assert e < 2e-2, e      # bf16 through 2 blocks + merger: ~1% rms
