"""Golden vectors for the Qwen2.5-VL family produced by the REFERENCE'S OWN Python files (run once, in the build container).

    python tests/golden/make_golden_ref_qwen2_5_vl.py      # needs the reference tree; writes qwen2_5_vl_tiny_ref.npz

As tests/golden/make_golden_ref.py: `oracle/mlx_shim` stands in for `mlx`, and the reference's

    mlx_vlm/models/qwen2_5_vl/{config,vision,language,qwen2_5_vl}.py   (+ models/{base,cache,rope_utils}.py)

are imported and RUN unchanged, on tests/qwen2_5_vl_ref.py's tiny config (depth 2, block 0 windowed, block 1 full; 2 heads of 80;
intermediate 172; out 256) with its seeded weights, in fp32 and in bf16.  The tower runs over the shim as it is, with one
exception: vision.py:341 puts array SCALARS into a `set`, so the shim's array class is given a `__hash__` here, at run time (by
value for one-element arrays); nothing under oracle/ is edited.

Recorded: for a list of grid sets the window index, the window table before and after the reference's de-duplication, the
full-image table and the reverse index; per model case and dtype the tower output, the merged input embeddings, the position
ids, the prefill logits and 8 greedy steps - the larger arrays as sampled rows.  Only the .npz is read at test time.
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
REF = os.environ.get("VLM_REFERENCE_ROOT", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle", "mlx_shim"))

# grid sets whose host tables are recorded (tests/test_qwen2_5_vl_cpu.py)
TABLE_GRIDS = {
    "g8x8": [(1, 8, 8)], "g12x20": [(1, 12, 20)], "g2x2": [(1, 2, 2)], "g2x4x6": [(2, 4, 6)], "g10x6": [(1, 10, 6)],
    "two": [(1, 12, 20), (1, 8, 8)], "three": [(1, 8, 8), (1, 2, 2), (1, 10, 6)],
}
# model cases: grids of one prompt
CASES = {"one_image": [(1, 12, 20)], "three_images": [(1, 8, 8), (1, 2, 2), (1, 10, 6)]}
FEAT_ROWS = slice(None, None, 2)
EMB_ROWS = slice(None, None, 3)
LOGIT_ROWS = slice(None, None, 7)


def import_reference():
    import mlx.core as mx  # the shim

    def pkg(name, path):
        m = types.ModuleType(name)
        m.__path__ = [path]
        m.__package__ = name
        sys.modules[name] = m
        return m

    pkg("mlx_vlm", os.path.join(REF, "mlx_vlm"))
    pkg("mlx_vlm.models", os.path.join(REF, "mlx_vlm", "models"))
    pkg("mlx_vlm.models.qwen2_5_vl", os.path.join(REF, "mlx_vlm", "models", "qwen2_5_vl"))
    tq = types.ModuleType("mlx_vlm.turboquant")
    for n in ("BatchTurboQuantKVCache", "TurboQuantKVCache", "HybridQuantKVCache"):
        setattr(tq, n, type(n, (), {}))
    tq._state_length = lambda s: s[0].shape[-2]
    tq.turboquant_enabled = lambda *a, **k: False
    sys.modules["mlx_vlm.turboquant"] = tq
    sys.modules["mlx_vlm.models.qwen2_5_vl.processing_qwen2_5_vl"] = types.ModuleType(
        "mlx_vlm.models.qwen2_5_vl.processing_qwen2_5_vl")
    q = importlib.import_module("mlx_vlm.models.qwen2_5_vl.qwen2_5_vl")
    cfgm = importlib.import_module("mlx_vlm.models.qwen2_5_vl.config")
    cache = importlib.import_module("mlx_vlm.models.cache")
    for m in (q, cfgm, cache):
        assert m.__file__.startswith(REF), m.__file__
    # vision.py:341 `if x not in seen` over array scalars: hash a one-element array by its value
    arr = type(mx.array(np.zeros(1, dtype=np.int32)))
    if getattr(arr, "__hash__", None) is None:
        arr.__hash__ = lambda self: hash(self.item()) if self.size == 1 else id(self)
    return mx, q, cfgm, cache


def f32(a):
    return np.asarray(a._t.to(torch.float32).numpy()) if hasattr(a, "_t") else np.asarray(a, dtype=np.float32)


def i64(a):
    return np.asarray(a._t.numpy()).astype(np.int64) if hasattr(a, "_t") else np.asarray(a, dtype=np.int64)


def main():
    import qwen2_5_vl_ref as R

    torch.manual_seed(0)
    torch.set_num_threads(4)
    mx, q, cfgm, cache_mod = import_reference()
    cfg = R.tiny_cfg()
    d = R.model_config_dict(cfg)
    d["max_position_embeddings"] = 32768
    mc = cfgm.ModelConfig.from_dict(d)
    if isinstance(mc.text_config, dict):
        mc.text_config = cfgm.TextConfig.from_dict(mc.text_config)
    if isinstance(mc.vision_config, dict):
        mc.vision_config = cfgm.VisionConfig.from_dict(mc.vision_config)
    blob = {}
    model = None
    for dt_name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        W = R.random_weights(cfg, seed=1234, dtype=torch.float32, std=0.05, embed_std=0.2)
        model = q.Model(mc)
        weights = {k: mx.array(w.to(dt)) for k, w in W.items()}
        weights = model.vision_tower.sanitize(model.sanitize(weights))
        model.load_weights(list(weights.items()), strict=True)
        for name, grids in CASES.items():
            ids, pix, thw = R.synth_request(cfg, grids, seed=len(grids))
            input_ids = mx.array(ids.astype(np.int32))
            pixel_values = mx.array(pix.astype(np.float32))
            grid = mx.array(thw.astype(np.int32))
            feats = model.vision_tower(pixel_values.astype(dt), grid, output_hidden_states=False)
            patches = model.vision_tower.patch_embed(pixel_values.astype(dt))
            emb = model.get_input_embeddings(input_ids, pixel_values, image_grid_thw=grid)
            kv = [cache_mod.KVCache() for _ in model.language_model.layers]
            out = model.language_model(input_ids, inputs_embeds=emb.inputs_embeds, cache=kv, position_ids=emb.position_ids,
                                       pixel_values=pixel_values, image_grid_thw=grid, rope_deltas=emb.rope_deltas)
            logits = out.logits
            step_logits, toks = [], []
            y = mx.argmax(logits[:, -1, :], axis=-1)
            for _ in range(8):
                toks.append(int(y.item()))
                o = model.language_model(y[None] if y.ndim == 1 else y, cache=kv)
                step_logits.append(f32(o.logits[0, -1]))
                y = mx.argmax(o.logits[:, -1, :], axis=-1)
            p = f"{name}.{dt_name}."
            blob[p + "ref_image_features"] = f32(feats)[FEAT_ROWS]
            if dt_name == "bf16":
                blob[p + "ref_patch_embed"] = f32(patches)          # in full: the restatement continues from it
            blob[p + "ref_inputs_embeds"] = f32(emb.inputs_embeds[0])[EMB_ROWS]
            blob[p + "ref_prefill_logits"] = f32(logits[0])[LOGIT_ROWS]
            blob[p + "ref_prefill_last"] = f32(logits[0, -1])
            blob[p + "ref_decode_logits"] = np.stack(step_logits)
            blob[p + "ref_greedy"] = np.array(toks, dtype=np.int64)
            if dt_name == "f32":
                blob[name + ".ref_position_ids"] = i64(emb.position_ids)
                blob[name + ".ref_rope_deltas"] = i64(emb.rope_deltas).reshape(-1)
                blob[name + ".grids"] = np.array(grids, dtype=np.int64)
            print(p, "feats", f32(feats).shape, "logits", f32(logits[0]).shape, "greedy", toks)

    # ---- host tables, by the reference's own get_window_index and the de-duplication / cu_seqlens / argsort of its __call__
    vt = model.vision_tower
    for name, grids in TABLE_GRIDS.items():
        grid = mx.array(np.array(grids, dtype=np.int32))
        wi, cu = vt.get_window_index(grid)
        seen, idx = set(), []
        for i, x in enumerate(cu):                                   # vision.py:337-346, verbatim
            if x not in seen:
                seen.add(x)
                idx.append(i)
        cu_d = cu[mx.array(idx, dtype=mx.int32)]
        cs = []
        for i in range(grid.shape[0]):                                # vision.py:360-373
            cs.append(mx.repeat(grid[i, 1] * grid[i, 2], int(grid[i, 0])))
        cu_full = mx.pad(mx.cumsum(mx.concatenate(cs).astype(mx.int32), axis=0), (1, 0), mode="constant", constant_values=0)
        blob[f"tables.{name}.grids"] = np.array(grids, dtype=np.int64)
        blob[f"tables.{name}.window_index"] = i64(wi)
        blob[f"tables.{name}.cu_window_raw"] = i64(cu)
        blob[f"tables.{name}.cu_window"] = i64(cu_d)
        blob[f"tables.{name}.cu_full"] = i64(cu_full)
        blob[f"tables.{name}.reverse_index"] = i64(mx.argsort(wi, axis=0))
        blob[f"tables.{name}.rot_pos_emb"] = f32(vt.rot_pos_emb(grid))[::5]
        print(name, "windows", np.diff(blob[f"tables.{name}.cu_window"]).tolist())

    # ---- checkpoint key remap + conv layout (Model.sanitize qwen2_5_vl.py:184-195, VisionModel.sanitize vision.py:395-413)
    hf_keys = ["visual.patch_embed.proj.weight", "visual.merger.ln_q.weight", "visual.merger.mlp.0.bias",
               "visual.blocks.0.attn.qkv.weight", "visual.blocks.1.mlp.gate_proj.bias", "visual.blocks.1.mlp.down_proj.weight",
               "visual.blocks.0.norm1.weight", "model.embed_tokens.weight", "model.norm.weight", "lm_head.weight",
               "model.layers.0.self_attn.q_proj.bias", "model.layers.1.mlp.down_proj.weight"]
    gen = torch.Generator().manual_seed(5)
    hf_w = {k: mx.array(torch.randn(4, 3, 2, 6, 6, generator=gen) if k.endswith("patch_embed.proj.weight")
                        else torch.randn(3, generator=gen)) for k in hf_keys}
    san = model.vision_tower.sanitize(model.sanitize(dict(hf_w)))
    blob["sanitize.hf_keys"] = np.array(hf_keys)
    blob["sanitize.ref_keys"] = np.array(list(san.keys()))
    blob["sanitize.hf_conv"] = f32(hf_w["visual.patch_embed.proj.weight"])
    blob["sanitize.ref_conv"] = f32(san["vision_tower.patch_embed.proj.weight"])

    out = os.path.join(HERE, "qwen2_5_vl_tiny_ref.npz")
    np.savez_compressed(out, **blob)
    print("wrote", out, os.path.getsize(out), "bytes;", len(blob), "arrays")


if __name__ == "__main__":
    main()
