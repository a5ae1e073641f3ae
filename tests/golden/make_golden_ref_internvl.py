"""Golden vectors for the InternVL family produced by the REFERENCE'S OWN Python files (run once, in the build container).

    VLM_REFERENCE_ROOT=<reference checkout> python tests/golden/make_golden_ref_internvl.py
        -> internvl_tiny_ref.npz, internvl_tiling_ref.json

As tests/golden/make_golden_ref_qwen3_vl.py: `oracle/mlx_shim` stands in for `mlx`, and the reference's

    mlx_vlm/models/internvl_chat/{config,vision,language,internvl_chat,processor}.py   (+ models/{base,cache,mlp}.py)

are imported and RUN unchanged, on tests/internvl_ref.py's tiny configs (tower: depth 2, hidden 128, 2 heads, 56 / 14 -> 17 tokens
per tile; language model: the Qwen2 form with biases and the Qwen3 form with QK-norm, 2 layers each) with its seeded weights, in
fp32 and in bf16.  Only `mlx_vlm.turboquant` is stubbed.  One layer of the stand-in is completed at run time, in this process
(nothing under oracle/ is edited): `nn.Upsample`, which the reference's `interpolate` builds for the position table.  The tiles
here have the native size, so its scale factors are 1 and 1; at scale 1 with align_corners=False a cubic kernel samples at the
integer positions with weights (0, 1, 0, 0), the identity - the stand-in returns its input for that case and refuses any other.

Recorded: per form, case (one tile; three tiles = 2 + thumbnail; text only) and dtype the tower's embeddings and last state, the
image features, the merged input embeddings, the prefill logits and 8 greedy steps on the cache (larger arrays as sampled rows);
`pixel_shuffle` over the token numbers; `VisionModel.sanitize` on a torch-layout conv weight.  From processor.py:
`dynamic_preprocess` over a list of image sizes - the resize target and every crop box it asks PIL for, and the number of tiles
returned - and `build_transform` + the image processor on one seeded image.  Only the two output files are read at test time.
"""
from __future__ import annotations

import importlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("VLM_REFERENCE_ROOT", "")          # a checkout of the reference (Blaizzy/mlx-vlm v0.6.15)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle", "mlx_shim"))

CASES = {"one_tile": [1], "three_tiles": [3], "text_only": []}
ROWS3 = slice(None, None, 3)
ROWS7 = slice(None, None, 7)
# (width, height, min_num, max_num, use_thumbnail): square, 2:1, 1:3, tiny, one that runs into max_num, thumbnail on / off
TILING = [(500, 500, 1, 12, True), (800, 400, 1, 12, True), (800, 400, 1, 12, False), (300, 900, 1, 12, True), (20, 10, 1, 12, True),
          (4000, 250, 1, 12, True), (4000, 250, 1, 6, True), (1000, 700, 1, 12, True), (640, 480, 2, 4, False), (448, 448, 1, 1, True),
          (1344, 896, 1, 12, True), (333, 1000, 1, 12, False)]


def import_reference():
    if not os.path.isdir(os.path.join(REF, "mlx_vlm")):
        raise SystemExit("set VLM_REFERENCE_ROOT to a checkout of the reference")
    import mlx.core as mx  # the shim
    import mlx.nn as nn

    class Upsample(nn.Module):                          # see the module docstring
        def __init__(self, scale_factor, mode="nearest", align_corners=False):
            super().__init__()
            self.scale_factor = scale_factor

        def __call__(self, x):
            s = self.scale_factor if isinstance(self.scale_factor, (tuple, list)) else (self.scale_factor,)
            if any(float(v) != 1.0 for v in s):
                raise NotImplementedError(f"Upsample stand-in: scale {s}")
            return x

    nn.Upsample = Upsample

    def pkg(name, path):
        m = types.ModuleType(name)
        m.__path__ = [path]
        m.__package__ = name
        sys.modules[name] = m
        return m

    pkg("mlx_vlm", os.path.join(REF, "mlx_vlm"))
    pkg("mlx_vlm.models", os.path.join(REF, "mlx_vlm", "models"))
    pkg("mlx_vlm.models.internvl_chat", os.path.join(REF, "mlx_vlm", "models", "internvl_chat"))
    tq = types.ModuleType("mlx_vlm.turboquant")
    for n in ("BatchTurboQuantKVCache", "TurboQuantKVCache", "HybridQuantKVCache"):
        setattr(tq, n, type(n, (), {}))
    tq._state_length = lambda s: s[0].shape[-2]
    tq.turboquant_enabled = lambda *a, **k: False
    sys.modules["mlx_vlm.turboquant"] = tq
    m = importlib.import_module("mlx_vlm.models.internvl_chat.internvl_chat")
    cfgm = importlib.import_module("mlx_vlm.models.internvl_chat.config")
    cache = importlib.import_module("mlx_vlm.models.cache")
    base = importlib.import_module("mlx_vlm.models.base")
    proc = importlib.import_module("mlx_vlm.models.internvl_chat.processor")
    for mod in (m, cfgm, cache, base, proc):
        assert mod.__file__.startswith(REF), mod.__file__
    return mx, m, cfgm, cache, base, proc


def f32(a):
    return np.asarray(a._t.to(torch.float32).numpy()) if hasattr(a, "_t") else np.asarray(a, dtype=np.float32)


def record_tiling(proc):
    """dynamic_preprocess over TILING with PIL's resize / crop observed"""
    from PIL import Image

    out = []
    real_resize, real_crop = Image.Image.resize, Image.Image.crop
    for (w, h, mn, mx_, thumb) in TILING:
        log = {"resize": [], "crop": []}

        def resize(self, size, *a, **k):
            log["resize"].append([int(size[0]), int(size[1])])
            return real_resize(self, size, *a, **k)

        def crop(self, box=None):
            log["crop"].append([int(v) for v in box])
            return real_crop(self, box)

        Image.Image.resize, Image.Image.crop = resize, crop
        try:
            tiles = proc.dynamic_preprocess(Image.new("RGB", (w, h)), min_num=mn, max_num=mx_, image_size=448, use_thumbnail=thumb)
        finally:
            Image.Image.resize, Image.Image.crop = real_resize, real_crop
        out.append(dict(width=w, height=h, min_num=mn, max_num=mx_, use_thumbnail=thumb, n_tiles=len(tiles),
                        resized_to=log["resize"][0], boxes=log["crop"], thumbnail=len(log["resize"]) > 1,
                        tile_sizes=sorted({tuple(t.size) for t in tiles})))
    return out


def main():
    from tests import internvl_ref as R

    torch.manual_seed(0)
    torch.set_num_threads(4)
    mx, M, cfgm, cache_mod, base, proc = import_reference()
    blob = {}
    model = None
    for lm in ("qwen2", "qwen3"):
        cfg = R.tiny_cfg(lm)
        d = R.model_config_dict(cfg)
        mc = cfgm.ModelConfig.from_dict(d)
        mc.text_config = cfgm.TextConfig.from_dict(d["text_config"])
        mc.vision_config = cfgm.VisionConfig.from_dict(d["vision_config"])
        for dt_name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
            W = R.random_weights(cfg, seed=1234, dtype=torch.float32)
            model = M.Model(mc)
            weights = {k: mx.array(w.to(dt)) for k, w in W.items()}
            model.load_weights(list(weights.items()), strict=True)
            assert model.language_model.model.layers[0].self_attn._use_qk_norm == (lm == "qwen3")
            for name, tiles in CASES.items():
                ids, pix = R.synth_request(cfg, tiles, n_text=12 if tiles else 19, seed=len(tiles) + sum(tiles))
                input_ids = mx.array(ids.astype(np.int32))
                p = f"{lm}.{name}.{dt_name}."
                if tiles:
                    pixel_values = mx.array(pix.astype(np.float32))
                    if lm == "qwen2":                      # the tower does not depend on the language model
                        x = pixel_values.astype(dt).transpose(0, 2, 3, 1)
                        E = cfg.vision.hidden_size
                        blob[p + "ref_vision_embeddings"] = f32(model.vision_model.embeddings(x)).reshape(-1, E)[ROWS3]
                        blob[p + "ref_vision_last"] = f32(model.vision_model(x, output_hidden_states=True)[0]).reshape(-1, E)[ROWS3]
                    emb = model.get_input_embeddings(input_ids, pixel_values[None])            # the 5-D form the processor emits
                    where = ids[0] == cfg.image_token_index
                    blob[p + "ref_image_features"] = f32(emb.inputs_embeds[0])[where]
                else:
                    emb = model.get_input_embeddings(input_ids, None)
                kv = [cache_mod.KVCache() for _ in model.language_model.layers]
                logits = model.language_model(None, inputs_embeds=emb.inputs_embeds, cache=kv).logits
                step_logits, toks = [], []
                y = mx.argmax(logits[:, -1, :], axis=-1)
                for _ in range(8):
                    toks.append(int(y.item()))
                    o = model.language_model(y[None] if y.ndim == 1 else y, cache=kv)
                    step_logits.append(f32(o.logits[0, -1]))
                    y = mx.argmax(o.logits[:, -1, :], axis=-1)
                blob[p + "ref_inputs_embeds"] = f32(emb.inputs_embeds[0])[ROWS3]
                blob[p + "ref_prefill_logits"] = f32(logits[0])[ROWS7]
                blob[p + "ref_prefill_last"] = f32(logits[0, -1])
                blob[p + "ref_decode_logits"] = np.stack(step_logits)
                blob[p + "ref_greedy"] = np.array(toks, dtype=np.int64)
                print(p, "logits", f32(logits[0]).shape, "greedy", toks)

    # ---- pixel_shuffle over the token numbers (models/base.py:436-458)
    for P, r in ((16, 0.5), (1024, 0.5), (64, 0.25)):
        t = mx.array(torch.arange(P, dtype=torch.float32).reshape(1, P, 1))
        blob[f"pixel_shuffle.{P}.{r}"] = f32(base.pixel_shuffle(t, r))[0].astype(np.int64)
    # ---- VisionModel.sanitize (vision.py:247-265)
    gen = torch.Generator().manual_seed(5)
    conv = torch.randn(8, 3, 2, 2, generator=gen)
    san = model.vision_model.sanitize({"embeddings.patch_embedding.weight": mx.array(conv), "embeddings.position_ids": mx.array(torch.zeros(3)),
                                       "encoder.layers.0.ls1": mx.array(torch.ones(4))})
    blob["sanitize.hf_conv"] = conv.numpy()
    blob["sanitize.ref_conv"] = f32(san["embeddings.patch_embedding.weight"])
    blob["sanitize.ref_keys"] = np.array(list(san.keys()))

    # ---- processor.py: one seeded image through build_transform and through the image processor
    from PIL import Image

    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (90, 150, 3), dtype=np.uint8)
    blob["processor.image_hwc"] = img
    blob["processor.transform_56"] = f32(proc.build_transform(56)(Image.fromarray(img)))
    ip = proc.InternVLImageProcessor(size=56, dynamic_max_num=4, dynamic_use_thumbnail=True)
    feats = ip.preprocess([Image.fromarray(img)])
    blob["processor.pixel_values"] = f32(feats["pixel_values"])
    blob["processor.num_patches_list"] = np.array(feats["num_patches_list"], dtype=np.int64)

    out = os.path.join(HERE, "internvl_tiny_ref.npz")
    np.savez_compressed(out, **blob)
    print("wrote", out, os.path.getsize(out), "bytes;", len(blob), "arrays")
    tiling = record_tiling(proc)
    with open(os.path.join(HERE, "internvl_tiling_ref.json"), "w") as f:
        json.dump(tiling, f, indent=1)
    print("wrote internvl_tiling_ref.json:", [(t["width"], t["height"], t["resized_to"], t["n_tiles"]) for t in tiling])


if __name__ == "__main__":
    main()
