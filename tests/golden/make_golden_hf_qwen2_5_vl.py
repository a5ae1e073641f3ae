"""HuggingFace goldens for the Qwen2.5-VL family (run once, in the build container; only the .npz is committed).

    python tests/golden/make_golden_hf_qwen2_5_vl.py       # writes tests/golden/qwen2_5_vl_tiny_hf.npz

Source of truth: transformers (5.15.0) `Qwen2_5_VLForConditionalGeneration` on torch-CPU fp32, eager attention, on the tiny
config and seeded weights of tests/qwen2_5_vl_ref.py (loaded through the inverse of `sanitize`).  Recorded per case: tower
features, position ids + rope deltas, prompt logits.  As for Qwen2-VL, HF fp32 pins the model SEMANTICS of the family - the
window order, the window table, RMSNorm / biased SwiGLU blocks, which blocks attend over the whole image - not MLX's bf16
rounding.

Where the reference departs from HF (nothing of it is absorbed in a tolerance; tests/test_qwen2_5_vl_cpu.py):
  * none was found on the image path at these grids: tower features, position ids and prompt logits of the restatement - which is
    bit-identical to the reference in bf16 - agree with HF to 1e-4.  (HF drops the zero-length windows with
    torch.unique_consecutive, the reference with a first-occurrence scan: the same table for a non-decreasing sequence.)
  * HF's get_rope_index scales the temporal position of VIDEO frames by `tokens_per_second`; the reference's does not.  Video is
    out of scope here, so no test depends on it.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = {"one_image": [(1, 12, 20)], "three_images": [(1, 8, 8), (1, 2, 2), (1, 10, 6)]}


def hf_model(cfg, W):
    from transformers import Qwen2_5_VLConfig, Qwen2_5_VLForConditionalGeneration

    t, v = cfg.text, cfg.vision
    hcfg = Qwen2_5_VLConfig(
        text_config=dict(hidden_size=t.hidden_size, num_hidden_layers=t.num_hidden_layers,
                         intermediate_size=t.intermediate_size, num_attention_heads=t.num_attention_heads,
                         num_key_value_heads=t.num_key_value_heads, vocab_size=t.vocab_size, rms_norm_eps=t.rms_norm_eps,
                         rope_theta=t.rope_theta, rope_scaling={"type": "mrope", "mrope_section": t.mrope_section},
                         tie_word_embeddings=t.tie_word_embeddings, max_position_embeddings=32768,
                         bos_token_id=0, eos_token_id=1, pad_token_id=2),
        vision_config=dict(depth=v.depth, hidden_size=v.hidden_size, intermediate_size=v.intermediate_size,
                           out_hidden_size=v.out_hidden_size, num_heads=v.num_heads, patch_size=v.patch_size,
                           spatial_merge_size=v.spatial_merge_size, temporal_patch_size=v.temporal_patch_size,
                           in_channels=v.in_channels, window_size=v.window_size,
                           fullatt_block_indexes=list(v.fullatt_block_indexes), hidden_act="silu"),
        image_token_id=cfg.image_token_id, video_token_id=cfg.video_token_id,
        vision_start_token_id=cfg.vision_start_token_id, vision_end_token_id=cfg.vision_start_token_id + 1,
        tie_word_embeddings=t.tie_word_embeddings, bos_token_id=0, eos_token_id=1, pad_token_id=2,
    )
    hcfg._attn_implementation = "eager"
    m = Qwen2_5_VLForConditionalGeneration(hcfg).eval().to(torch.float32)
    sd = {}
    for k, w in W.items():
        w = w.to(torch.float32)
        if k.startswith("vision_tower."):
            hk = "model.visual." + k[len("vision_tower."):]
            if "patch_embed.proj.weight" in k:
                w = w.permute(0, 4, 1, 2, 3).contiguous()  # (O,T,H,W,C) -> (O,C,T,H,W)
        elif k.startswith("language_model.model."):
            hk = "model.language_model." + k[len("language_model.model."):]
        elif k.startswith("language_model.lm_head."):
            hk = "lm_head." + k[len("language_model.lm_head."):]
        else:
            raise KeyError(k)
        sd[hk] = w
    if t.tie_word_embeddings:
        sd["lm_head.weight"] = sd["model.language_model.embed_tokens.weight"]
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all("rotary" in k or "inv_freq" in k for k in missing), missing
    return m


def main():
    import qwen2_5_vl_ref as R

    torch.manual_seed(0)
    torch.set_num_threads(4)
    cfg = R.tiny_cfg()
    W = R.random_weights(cfg, seed=1234, dtype=torch.float32, std=0.05, embed_std=0.2)
    hf = hf_model(cfg, W)
    blob = {}
    for name, grids in CASES.items():
        ids, pix, thw = R.synth_request(cfg, grids, seed=len(grids))
        with torch.no_grad():
            tid, tpix, tthw = torch.from_numpy(ids), torch.from_numpy(pix), torch.from_numpy(thw)
            mm = (tid == cfg.image_token_id).to(torch.int32)
            out = hf(input_ids=tid, pixel_values=tpix, image_grid_thw=tthw, mm_token_type_ids=mm, use_cache=False)
            feats = hf.model.visual(tpix, grid_thw=tthw)
            if not torch.is_tensor(feats):
                feats = feats.pooler_output if hasattr(feats, "pooler_output") else feats[0]
            pos, deltas = hf.model.get_rope_index(tid, mm_token_type_ids=mm, image_grid_thw=tthw)
        blob[name + ".grids"] = np.array(grids, dtype=np.int64)
        blob[name + ".hf_logits"] = out.logits[0].numpy().astype(np.float32)[::3]
        blob[name + ".hf_logits_last"] = out.logits[0, -1].numpy().astype(np.float32)
        blob[name + ".hf_image_features"] = feats.numpy().astype(np.float32)
        blob[name + ".hf_position_ids"] = pos.numpy().astype(np.int64)
        blob[name + ".hf_rope_deltas"] = deltas.numpy().astype(np.int64)
        print(name, ids.shape, pix.shape, thw.tolist(), out.logits.shape, feats.shape)
    out = os.path.join(HERE, "qwen2_5_vl_tiny_hf.npz")
    np.savez_compressed(out, **blob)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
