"""Golden vectors for the Qwen3-VL family produced by the REFERENCE'S OWN Python files (run once, in the build container).

    VLM_REFERENCE_ROOT=<reference checkout> python tests/golden/make_golden_ref_qwen3_vl.py      # writes qwen3_vl_tiny_ref.npz

As tests/golden/make_golden_ref_qwen2_5_vl.py: `oracle/mlx_shim` stands in for `mlx`, and the reference's

    mlx_vlm/models/qwen3_vl/{config,vision,language,qwen3_vl}.py   (+ models/{base,cache,rope_utils,mlp}.py)

are imported and RUN unchanged, on tests/qwen3_vl_ref.py's tiny config (4 decoder layers, 4 : 2 heads of 128 over hidden 256;
tower depth 3, 2 heads of 64, an 8 x 8 position table, DeepStack taps behind blocks 0 and 2) with its seeded weights, in fp32
and in bf16.  Without Metal the reference takes its pure-MLX rope path: the "fallback" mode of the restatement.  Only
`mlx_vlm.turboquant` and the processing module are stubbed.  One behaviour of the stand-in is completed at run time, in this
process (nothing under oracle/ is edited): `a.at[rows].add(v)` with a bare index array, which MLX applies to the first axis
(language.py:279, the DeepStack add) and the stand-in knew for the last axis only.

Recorded: per model case and dtype the tower features and every tap, the merged input embeddings, the prefill logits (with
DeepStack) and 8 greedy steps on the cache (without) - the larger arrays as sampled rows; position ids and rope deltas (one
image, three images, text only); the interleaved selector; `rot_pos_emb`; `fast_pos_embed_interpolate` over an IDENTITY
position table in fp32, which lays the four corner indices and bilinear weights of every patch row open; the key map of
`sanitize`.  Only the .npz is read at test time.
"""
from __future__ import annotations

import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("VLM_REFERENCE_ROOT", "")          # a checkout of the reference (Blaizzy/mlx-vlm v0.6.15)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle", "mlx_shim"))

CASES = {"one_image": [(1, 4, 6)], "three_images": [(1, 8, 8), (1, 2, 2), (1, 4, 6)], "text_only": []}
INTERP_GRIDS = {"g4x6": [(1, 4, 6)], "g2x2": [(1, 2, 2)], "g8x8": [(1, 8, 8)], "g2x6x4": [(2, 6, 4)],
                "three": [(1, 8, 8), (1, 2, 2), (1, 4, 6)]}
FEAT_ROWS = slice(None, None, 2)
EMB_ROWS = slice(None, None, 3)
LOGIT_ROWS = slice(None, None, 7)


def import_reference():
    if not os.path.isdir(os.path.join(REF, "mlx_vlm")):
        raise SystemExit("set VLM_REFERENCE_ROOT to a checkout of the reference")
    import mlx.core as mx  # the shim

    def pkg(name, path):
        m = types.ModuleType(name)
        m.__path__ = [path]
        m.__package__ = name
        sys.modules[name] = m
        return m

    pkg("mlx_vlm", os.path.join(REF, "mlx_vlm"))
    pkg("mlx_vlm.models", os.path.join(REF, "mlx_vlm", "models"))
    pkg("mlx_vlm.models.qwen3_vl", os.path.join(REF, "mlx_vlm", "models", "qwen3_vl"))
    tq = types.ModuleType("mlx_vlm.turboquant")
    for n in ("BatchTurboQuantKVCache", "TurboQuantKVCache", "HybridQuantKVCache"):
        setattr(tq, n, type(n, (), {}))
    tq._state_length = lambda s: s[0].shape[-2]
    tq.turboquant_enabled = lambda *a, **k: False
    sys.modules["mlx_vlm.turboquant"] = tq
    sys.modules["mlx_vlm.models.qwen3_vl.processing_qwen3_vl"] = types.ModuleType("mlx_vlm.models.qwen3_vl.processing_qwen3_vl")
    q = importlib.import_module("mlx_vlm.models.qwen3_vl.qwen3_vl")
    cfgm = importlib.import_module("mlx_vlm.models.qwen3_vl.config")
    cache = importlib.import_module("mlx_vlm.models.cache")
    rope = importlib.import_module("mlx_vlm.models.rope_utils")
    for m in (q, cfgm, cache, rope):
        assert m.__file__.startswith(REF), m.__file__
    # language.py:279 `batch_result.at[batch_indices].add(sample_embeds)`: MLX's `a.at[rows]` with a bare index array addresses
    # the FIRST axis; the stand-in's `.at[]` restates the `[..., indices]` form alone and would take the rows for columns
    at, to_t = mx._At, mx._u
    last_axis_apply = at._apply

    def apply(self, v, fn):
        if isinstance(self._i, tuple):
            return last_axis_apply(self, v, fn)
        t = self._a._t.clone()
        rows = torch.as_tensor(to_t(self._i)).reshape(-1).tolist()
        vt = torch.as_tensor(to_t(v)).to(t.dtype)
        vt = vt.expand(len(rows), *t.shape[1:]) if vt.dim() < t.dim() or vt.shape[0] != len(rows) else vt
        for k, j in enumerate(rows):               # every update is applied, one after the other (mlx.core.array.at)
            t[j] = fn(t[j], vt[k])
        return mx.array(t)

    at._apply = apply
    return mx, q, cfgm, cache, rope


def f32(a):
    return np.asarray(a._t.to(torch.float32).numpy()) if hasattr(a, "_t") else np.asarray(a, dtype=np.float32)


def i64(a):
    return np.asarray(a._t.numpy()).astype(np.int64) if hasattr(a, "_t") else np.asarray(a, dtype=np.int64)


def main():
    import qwen3_vl_ref as R

    torch.manual_seed(0)
    torch.set_num_threads(4)
    mx, q, cfgm, cache_mod, rope = import_reference()
    cfg = R.tiny_cfg()
    mc = cfgm.ModelConfig.from_dict(R.model_config_dict(cfg))
    assert not isinstance(mc.text_config, dict) and not isinstance(mc.vision_config, dict)
    blob = {}
    model = None
    for dt_name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        W = R.random_weights(cfg, seed=1234, dtype=torch.float32, std=0.05, embed_std=0.2)
        model = q.Model(mc)
        weights = {k: mx.array(w.to(dt)) for k, w in W.items()}
        weights = model.vision_tower.sanitize(model.sanitize(weights))
        model.load_weights(list(weights.items()), strict=True)
        assert not model.language_model.model.layers[0].self_attn.rotary_emb.fused_apply      # the pure-MLX rope path
        for name, grids in CASES.items():
            ids, pix, thw = R.synth_request(cfg, grids, n_text=12 if grids else 19, seed=len(grids))
            input_ids = mx.array(ids.astype(np.int32))
            p = f"{name}.{dt_name}."
            if grids:
                pixel_values = mx.array(pix.astype(np.float32))
                grid = mx.array(thw.astype(np.int32))
                feats, taps = model.vision_tower(pixel_values.astype(dt), grid)
                emb = model.get_input_embeddings(input_ids, pixel_values, image_grid_thw=grid)
                kw = dict(pixel_values=pixel_values, image_grid_thw=grid)
                blob[p + "ref_image_features"] = f32(feats)[FEAT_ROWS]
                for j, t in enumerate(taps):
                    blob[p + f"ref_tap{j}"] = f32(t)[FEAT_ROWS]
                assert len(emb.deepstack_visual_embeds) == len(taps)
            else:
                emb = model.get_input_embeddings(input_ids, None)
                kw = {}
            kv = [cache_mod.KVCache() for _ in model.language_model.layers]
            model.language_model._rope_deltas = None
            model.language_model._position_ids = None
            out = model.language_model(input_ids, inputs_embeds=emb.inputs_embeds, cache=kv, position_ids=emb.position_ids,
                                       rope_deltas=emb.rope_deltas, visual_pos_masks=emb.visual_pos_masks,
                                       deepstack_visual_embeds=emb.deepstack_visual_embeds, **kw)
            logits = out.logits
            step_logits, toks = [], []
            y = mx.argmax(logits[:, -1, :], axis=-1)
            for _ in range(8):
                toks.append(int(y.item()))
                o = model.language_model(y[None] if y.ndim == 1 else y, cache=kv)
                step_logits.append(f32(o.logits[0, -1]))
                y = mx.argmax(o.logits[:, -1, :], axis=-1)
            blob[p + "ref_inputs_embeds"] = f32(emb.inputs_embeds[0])[EMB_ROWS]
            blob[p + "ref_prefill_logits"] = f32(logits[0])[LOGIT_ROWS]
            blob[p + "ref_prefill_last"] = f32(logits[0, -1])
            blob[p + "ref_decode_logits"] = np.stack(step_logits)
            blob[p + "ref_greedy"] = np.array(toks, dtype=np.int64)
            if dt_name == "f32":
                blob[name + ".ref_position_ids"] = i64(emb.position_ids)
                blob[name + ".ref_rope_deltas"] = i64(emb.rope_deltas).reshape(-1)
                blob[name + ".grids"] = np.array(grids, dtype=np.int64).reshape(-1, 3)
                if grids:
                    blob[name + ".ref_visual_pos_masks"] = np.asarray(emb.visual_pos_masks._t.numpy()).astype(bool)
            print(p, "logits", f32(logits[0]).shape, "greedy", toks)

    # ---- host tables by the reference's own functions (the fp32 model)
    t = cfg.text
    blob["selector.interleaved"] = i64(rope.mrope_position_selector("interleaved", t.mrope_section, t.head_dim // 2))
    blob["selector.interleaved_16_24_24"] = i64(rope.mrope_position_selector("interleaved", [16, 24, 24], 64))
    blob["selector.interleaved_8_4_4_dim16"] = i64(rope.mrope_position_selector("interleaved", [8, 4, 4], 16))
    vt = model.vision_tower
    S = vt.num_grid_per_side
    table = vt.pos_embed.weight
    vt.pos_embed.weight = mx.array(torch.eye(S * S, dtype=torch.float32))            # an identity table: see the module docstring
    for name, grids in INTERP_GRIDS.items():
        grid = mx.array(np.array(grids, dtype=np.int32))
        blob[f"interp.{name}.grids"] = np.array(grids, dtype=np.int64)
        blob[f"interp.{name}.dense"] = f32(vt.fast_pos_embed_interpolate(grid))
        blob[f"interp.{name}.rot_pos_emb"] = f32(vt.rot_pos_emb(grid))
    vt.pos_embed.weight = table

    # ---- checkpoint key remap + conv layout (Model.sanitize qwen3_vl.py:238-252, VisionModel.sanitize vision.py:427-445)
    hf_keys = ["model.visual.patch_embed.proj.weight", "model.visual.patch_embed.proj.bias", "model.visual.pos_embed.weight",
               "model.visual.merger.norm.weight", "model.visual.merger.linear_fc1.bias",
               "model.visual.deepstack_merger_list.1.linear_fc2.weight", "model.visual.blocks.0.attn.qkv.weight",
               "model.visual.blocks.2.mlp.linear_fc1.bias", "model.language_model.embed_tokens.weight",
               "model.language_model.norm.weight", "lm_head.weight", "model.language_model.layers.0.self_attn.q_norm.weight",
               "model.language_model.layers.3.mlp.down_proj.weight"]
    gen = torch.Generator().manual_seed(5)
    hf_w = {k: mx.array(torch.randn(4, 3, 2, 6, 6, generator=gen) if k.endswith("patch_embed.proj.weight")
                        else torch.randn(3, generator=gen)) for k in hf_keys}
    san = model.vision_tower.sanitize(model.sanitize(dict(hf_w)))
    blob["sanitize.hf_keys"] = np.array(hf_keys)
    blob["sanitize.ref_keys"] = np.array(list(san.keys()))
    blob["sanitize.hf_conv"] = f32(hf_w["model.visual.patch_embed.proj.weight"])
    blob["sanitize.ref_conv"] = f32(san["vision_tower.patch_embed.proj.weight"])

    out = os.path.join(HERE, "qwen3_vl_tiny_ref.npz")
    np.savez_compressed(out, **blob)
    print("wrote", out, os.path.getsize(out), "bytes;", len(blob), "arrays")


if __name__ == "__main__":
    main()
