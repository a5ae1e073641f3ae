"""HuggingFace goldens for the Qwen3-VL family (run once, in the build container; only the .npz is committed).

    python tests/golden/make_golden_hf_qwen3_vl.py       # writes tests/golden/qwen3_vl_tiny_hf.npz

Source of truth: transformers (5.15.0) `Qwen3VLForConditionalGeneration` on torch-CPU fp32, eager attention, on the tiny config
and seeded weights of tests/qwen3_vl_ref.py (loaded through the inverse of `sanitize`).  Recorded per case: tower features and
DeepStack taps, position ids + rope deltas, prompt logits.  As for the other Qwen families, HF fp32 pins the model SEMANTICS -
the bilinear position rows and their merge-unit order, the tanh-GELU blocks, the post-shuffle tap mergers, QK-norm, the
interleaved M-RoPE selector, which decoder layers get which tap added - not MLX's bf16 rounding.

Where the reference departs from HF (nothing of it is absorbed in a tolerance; tests/test_qwen3_vl_cpu.py):
  * none was found on the image path at these grids: features, taps, position ids and prompt logits of the restatement - which
    is bit-identical to the reference in bf16 and fp32 - agree with HF to 1e-4.
  * HF's get_rope_index gives the frames of a VIDEO their own timestamps; the reference's does not.  Video is out of scope here,
    so no test depends on it.
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

CASES = {"one_image": [(1, 4, 6)], "three_images": [(1, 8, 8), (1, 2, 2), (1, 4, 6)]}


def hf_model(cfg, W):
    from transformers import Qwen3VLConfig, Qwen3VLForConditionalGeneration

    import qwen3_vl_ref as R

    t, v = cfg.text, cfg.vision
    rope = {"rope_type": "default", "mrope_section": list(t.mrope_section), "mrope_interleaved": True, "rope_theta": t.rope_theta}
    hcfg = Qwen3VLConfig(
        text_config=dict(hidden_size=t.hidden_size, num_hidden_layers=t.num_hidden_layers, intermediate_size=t.intermediate_size,
                         num_attention_heads=t.num_attention_heads, num_key_value_heads=t.num_key_value_heads,
                         head_dim=t.head_dim, vocab_size=t.vocab_size, rms_norm_eps=t.rms_norm_eps, rope_theta=t.rope_theta,
                         rope_scaling=rope, rope_parameters=rope, attention_bias=False,
                         tie_word_embeddings=t.tie_word_embeddings, max_position_embeddings=32768,
                         bos_token_id=0, eos_token_id=1, pad_token_id=2),
        vision_config=dict(depth=v.depth, hidden_size=v.hidden_size, intermediate_size=v.intermediate_size,
                           out_hidden_size=v.out_hidden_size, num_heads=v.num_heads, patch_size=v.patch_size,
                           spatial_merge_size=v.spatial_merge_size, temporal_patch_size=v.temporal_patch_size,
                           in_channels=v.in_channels, num_position_embeddings=v.num_position_embeddings,
                           deepstack_visual_indexes=list(v.deepstack_visual_indexes), hidden_act="gelu_pytorch_tanh"),
        image_token_id=cfg.image_token_id, video_token_id=cfg.video_token_id,
        vision_start_token_id=cfg.vision_start_token_id, vision_end_token_id=cfg.vision_start_token_id + 1,
        tie_word_embeddings=t.tie_word_embeddings, bos_token_id=0, eos_token_id=1, pad_token_id=2,
    )
    hcfg._attn_implementation = "eager"
    m = Qwen3VLForConditionalGeneration(hcfg).eval().to(torch.float32)
    sd = {k: w.to(torch.float32) for k, w in R.to_hf_keys(W).items()}
    if t.tie_word_embeddings:
        sd["lm_head.weight"] = sd["model.language_model.embed_tokens.weight"]
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all("rotary" in k or "inv_freq" in k for k in missing), missing
    return m


def main():
    import qwen3_vl_ref as R

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
            vis = hf.model.visual(tpix, grid_thw=tthw)
            if isinstance(vis, tuple):
                feats, taps = vis
            else:
                feats = vis.pooler_output if getattr(vis, "pooler_output", None) is not None else vis.last_hidden_state
                taps = vis.deepstack_features
            try:
                pos, deltas = hf.model.get_rope_index(tid, mm_token_type_ids=mm, image_grid_thw=tthw)
            except TypeError:
                pos, deltas = hf.model.get_rope_index(tid, image_grid_thw=tthw)
        blob[name + ".grids"] = np.array(grids, dtype=np.int64)
        blob[name + ".hf_logits"] = out.logits[0].numpy().astype(np.float32)[::3]
        blob[name + ".hf_logits_last"] = out.logits[0, -1].numpy().astype(np.float32)
        blob[name + ".hf_image_features"] = feats.numpy().astype(np.float32)
        for j, tap in enumerate(taps):
            blob[name + f".hf_tap{j}"] = tap.numpy().astype(np.float32)
        blob[name + ".hf_position_ids"] = pos.numpy().astype(np.int64)
        blob[name + ".hf_rope_deltas"] = deltas.numpy().astype(np.int64)
        print(name, ids.shape, pix.shape, thw.tolist(), out.logits.shape, feats.shape, len(taps))
    out = os.path.join(HERE, "qwen3_vl_tiny_hf.npz")
    np.savez_compressed(out, **blob)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
