"""convert(): the reference's `mlx_vlm.convert` (mlx_vlm/convert.py:282-454) for the part this engine can run - a local
checkpoint of one of the built families -> an MLX-format checkpoint, optionally quantized to MLX affine 4 bits / group 64 on
the device (`ops.quantize_w4`, the quantise direction of vlm_dequant_w4) or dequantized back to bf16 (`ops.dequant_w4`).

    python -m mlx_vlm_amd.convert --hf-path <dir> --mlx-path <dir> [-q] [--dtype bfloat16] [-d]

The source (HF layout or already MLX layout) is read through the family's own `sanitize` (utils.read_sanitized_weights on a host
object that never gets weights: no KV pool, no graph, no device memory), so the names and conv layouts written are the
MLX-format ones - what `load()` takes and what mlx-vlm itself writes.  Saving follows the reference's save_weights /
make_shards / save_config (utils.py:1293-1315, 1422-1500): shards of at most 5 GB in insertion order, safetensors metadata
{"format": "mlx"}, a key-sorted index, a key-sorted config without `_name_or_path` / `torch_dtype`.

Which tensors `quantize=True` takes - the reference's rule (convert.py:309-314, quant_utils.py:84-96, utils.py:548-560)
restated over the sanitized weight dict: a key `<path>.weight` whose tensor is 2-D (of the modules these families are made
of only nn.Linear and nn.Embedding have `to_quantized`, and only they hold a 2-D `weight`), whose path names no multimodal
module (MULTIMODAL_MODULES) and whose last dimension is a multiple of 64.  A quantized Linear / Embedding gets `.weight`
(uint32 words), `.scales`, `.biases` (bf16); its own `.bias` is left as it is.  Per family (QUANTIZED_PREFIXES / BF16_PREFIXES):

  qwen2_vl     quantized: language_model.model.embed_tokens, language_model.model.layers.* (q/k/v/o_proj, gate/up/down_proj),
               language_model.lm_head (untied checkpoints)
               bf16:      vision_tower.* (patch_embed, blocks, and the merger: it lives inside the tower)
  llava_bunny  quantized: language_model.model.embed_tokens, language_model.model.layers.*, language_model.model.lm_head,
               mm_projector.linear_1, mm_projector.linear_2
               bf16:      vision_tower.* (vision_tower.vision_tower.vision_model: position_embedding and pooling head too)
  phi3_v       quantized: model.embed_tokens, model.layers.* (qkv_proj, o_proj, gate_up_proj, down_proj), lm_head,
               model.vision_embed_tokens.img_projection.0 / .2
               bf16:      model.vision_embed_tokens.img_processor.* (its vision_model); glb_GN / sub_GN are no `.weight`
  idefics2     quantized: language_model.embed_tokens, language_model.layers.*, language_model.lm_head,
               connector.modality_projection.*, connector.perceiver_resampler.layers.* (q/k/v/o_proj, mlp);
               `connector.perceiver_resampler.latents` is no `.weight`
               bf16:      vision_model.*
Norm weights are 1-D and conv weights 4-D / 5-D everywhere, so the 2-D rule leaves them alone.  The loaders of qwen2_vl,
phi3_v and idefics2 read such a checkpoint (connector / projection Linears are dequantized once at load); the llava_bunny
loader takes bf16 language models only, so its 4-bit output is for readers of the MLX format.

Refused loudly (nothing is written): other bit widths / group sizes / modes, AWQ, the mixed-bit recipes, a predicate that
returns per-layer parameters, MTP drafter extraction, hub upload, families that are not built.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
from typing import Callable, Dict, List, Optional

import torch

from . import utils
from .models import quantized as Qz

MODEL_CONVERSION_DTYPES = ("float16", "bfloat16", "float32")
# path fragments of modules that stay in the model dtype (the names of the reference's skip_multimodal_module, utils.py:548-559)
MULTIMODAL_MODULES = ("vision_model", "vision_tower", "vl_connector", "sam_model", "audio_model", "audio_tower",
                      "code_predictor", "img_projector", "multi_modal_projector", "patch_merge_mlp")
FAMILIES = ("qwen2_vl", "llava_bunny", "phi3_v", "idefics2")
QUANTIZED_PREFIXES = {
    "qwen2_vl": ("language_model.model.embed_tokens", "language_model.model.layers.", "language_model.lm_head"),
    "llava_bunny": ("language_model.model.embed_tokens", "language_model.model.layers.", "language_model.model.lm_head",
                    "mm_projector.linear_1", "mm_projector.linear_2"),
    "phi3_v": ("model.embed_tokens", "model.layers.", "lm_head", "model.vision_embed_tokens.img_projection."),
    "idefics2": ("language_model.embed_tokens", "language_model.layers.", "language_model.lm_head",
                 "connector.modality_projection.", "connector.perceiver_resampler.layers."),
}
BF16_PREFIXES = {
    "qwen2_vl": ("vision_tower.",),
    "llava_bunny": ("vision_tower.",),
    "phi3_v": ("model.vision_embed_tokens.img_processor.",),
    "idefics2": ("vision_model.",),
}
_MAX_SHARD_BYTES = 5 << 30          # the reference's MAX_FILE_SIZE_GB = 5 (utils.py:1293-1304); tests shrink it to kilobytes
_DEVICE = "cuda"
_INDEX = "model.safetensors.index.json"


def skip_multimodal_module(path: str) -> bool:
    """reference utils.py:538-560"""
    return any(m in path for m in MULTIMODAL_MODULES)


def quantized_paths(weights: Dict[str, torch.Tensor], quant_predicate: Optional[Callable] = None) -> List[str]:
    """The `<path>`s of a sanitized weight dict that `quantize=True` turns into 4-bit triples (module docstring), in order.
    A callable `quant_predicate(path, tensor) -> bool` narrows the base rule; per-layer parameters (a dict) are refused."""
    out = []
    for k, v in weights.items():
        if not k.endswith(".weight") or v.dim() != 2 or v.shape[-1] % Qz.GROUP != 0:
            continue
        path = k[: -len(".weight")]
        if skip_multimodal_module(path):
            continue
        if quant_predicate is not None:
            r = quant_predicate(path, v)
            if isinstance(r, dict):
                raise NotImplementedError(f"quant_predicate returned per-layer parameters for {path}: {r}; only one "
                                          "setting (affine, 4 bits, group 64) for the whole checkpoint is built")
            if not r:
                continue
        out.append(path)
    return out


def _refuse(hf_path, q_group_size, q_bits, q_mode, quant_method, upload_repo, quantize, dequantize, quant_predicate, mtp):
    """every option that is not built raises here, before the source is read (style of generate.py: nothing is dropped)"""
    if quantize and dequantize:
        raise ValueError("Choose either quantize or dequantize, not both.")
    if (q_bits or Qz.BITS) != Qz.BITS or (q_group_size or Qz.GROUP) != Qz.GROUP or q_mode != "affine":
        raise NotImplementedError(f"q_bits={q_bits}, q_group_size={q_group_size}, q_mode={q_mode!r}: only affine, 4 bits, "
                                  "group size 64 is built (the loader runs nothing else)")
    if quant_method != "rtn":
        raise NotImplementedError(f"quant_method={quant_method!r}: only round-to-nearest ('rtn') is built, AWQ calibration is not")
    if isinstance(quant_predicate, str):
        raise NotImplementedError(f"quant_predicate={quant_predicate!r}: the mixed-bit recipes need 3 / 6 / 8 bit weights")
    if quant_predicate is not None and not callable(quant_predicate):
        raise TypeError("quant_predicate must be a callable (path, tensor) -> bool")
    if mtp:
        raise NotImplementedError("mtp=True: MTP drafter extraction is not built")
    if upload_repo is not None:
        raise NotImplementedError("upload_repo: there is no hub upload in this build (local directories only)")
    if not os.path.isdir(str(hf_path)):
        raise FileNotFoundError(f"{hf_path} is not a local model directory (no hub download in this build)")


def _family(config: dict) -> str:
    model_type = str(config.get("model_type", "")).lower()
    family = utils.MODEL_REMAPPING.get(model_type, model_type)
    if family not in FAMILIES:
        raise NotImplementedError(f"model_type {model_type!r}: convert is built for {', '.join(FAMILIES)}")
    return family


def _resolve_dtype(config: dict, dtype: Optional[str]) -> Optional[str]:
    """reference convert.py:323-327"""
    if dtype is None:
        dtype = config.get("torch_dtype", None)
    if dtype is None and config.get("text_config"):
        dtype = config["text_config"].get("dtype", None)
    return dtype


def make_shards(weights: Dict[str, torch.Tensor], max_bytes: int) -> List[Dict[str, torch.Tensor]]:
    """reference utils.py:1293-1314: insertion order, a new shard when the next tensor would pass the limit (a tensor above
    the limit sits alone; no empty shard is opened for it)"""
    shards, shard, size = [], {}, 0
    for k, v in weights.items():
        if shard and size + v.nbytes > max_bytes:
            shards.append(shard)
            shard, size = {}, 0
        shard[k] = v
        size += v.nbytes
    shards.append(shard)
    return shards


def save_weights(save_path: str, weights: Dict[str, torch.Tensor]) -> None:
    """reference utils.py:1422-1476"""
    from safetensors.torch import save_file

    os.makedirs(save_path, exist_ok=True)
    shards = make_shards(weights, _MAX_SHARD_BYTES)
    n = len(shards)
    fmt = "model-{:05d}-of-{:05d}.safetensors" if n > 1 else "model.safetensors"
    index = {"metadata": {"total_size": sum(v.nbytes for v in weights.values())}, "weight_map": {}}
    for i, shard in enumerate(shards):
        name = fmt.format(i + 1, n)
        save_file(shard, os.path.join(save_path, name), metadata={"format": "mlx"})
        for k in shard:
            index["weight_map"][k] = name
    index["weight_map"] = {k: index["weight_map"][k] for k in sorted(index["weight_map"])}
    with open(os.path.join(save_path, _INDEX), "w") as f:
        json.dump(index, f, indent=4)


def save_config(config: dict, config_path: str) -> None:
    """reference utils.py:1479-1500"""
    config = dict(config)
    config.pop("_name_or_path", None)
    config.pop("torch_dtype", None)
    with open(config_path, "w") as f:
        json.dump(dict(sorted(config.items())), f, indent=4)


def _copy_sidecars(src: str, dst: str) -> None:
    """every file of the source that is no weight file, old index or config (tokenizer, processor and generation settings,
    chat templates, remote code), and every sub-directory, verbatim (reference convert.py:385-419)"""
    for name in sorted(os.listdir(src)):
        p = os.path.join(src, name)
        if os.path.isdir(p):
            if os.path.samefile(p, dst):          # the output directory sits inside the source
                continue
            shutil.copytree(p, os.path.join(dst, name), dirs_exist_ok=True)
        elif not name.endswith(".safetensors") and name not in (_INDEX, "config.json"):
            shutil.copy2(p, os.path.join(dst, name))


def _quantize_weights(weights, paths) -> Dict[str, torch.Tensor]:
    """one tensor at a time: host -> device -> ops.quantize_w4 -> host"""
    chosen, out = set(paths), {}
    for k, v in weights.items():
        path = k[: -len(".weight")] if k.endswith(".weight") else None
        if path in chosen:
            q = Qz.quantize(v, _DEVICE)
            out[k] = q.wq.view(torch.uint32)
            out[path + ".scales"], out[path + ".biases"] = Qz.split_sb(q)
        else:
            out[k] = v
    return out


def _dequantize_weights(weights) -> Dict[str, torch.Tensor]:
    """reference quant_utils.py:114-150: every `<path>` with `.scales` becomes a bf16 `.weight` again (ops.dequant_w4)"""
    paths = {k[: -len(".scales")] for k in weights if k.endswith(".scales")}
    for p in sorted(paths):
        if weights[p + ".scales"].dtype != torch.bfloat16 or weights[p + ".biases"].dtype != torch.bfloat16:
            raise NotImplementedError(f"{p}: scales / biases are {weights[p + '.scales'].dtype}; the dequantize kernel reads "
                                      "bfloat16 (pass dtype=\"bfloat16\")")
    out = {}
    for k, v in weights.items():
        path = k.rsplit(".", 1)[0]
        if path in paths and k.endswith((".scales", ".biases")):
            continue
        if path in paths and k.endswith(".weight"):
            v = Qz.dequantize_bf16(Qz.take(weights, path), _DEVICE).cpu()
        out[k] = v
    return out


def convert(
    hf_path: str,
    mlx_path: str = "mlx_model",
    quantize: bool = False,
    q_group_size: int = 64,
    q_bits: int = 4,
    q_mode: str = "affine",
    quant_method: str = "rtn",
    calibration: str = "text",
    calibration_data: Optional[str] = None,
    dtype: Optional[str] = None,
    upload_repo: str = None,
    revision: Optional[str] = None,
    dequantize: bool = False,
    trust_remote_code: bool = True,
    quant_predicate: Optional[str] = None,
    mtp: bool = False,
    mtp_output: Optional[str] = None,
):
    """reference convert.py:282-454.  `hf_path`: a local checkpoint directory.  `calibration*` belong to AWQ, `revision` to
    the hub and `mtp_output` to the MTP drafter, all refused; `trust_remote_code` has nothing to act on (no remote code runs)."""
    _refuse(hf_path, q_group_size, q_bits, q_mode, quant_method, upload_repo, quantize, dequantize, quant_predicate, mtp)
    hf_path, mlx_path = str(hf_path), str(mlx_path)
    if os.path.exists(mlx_path) and os.path.samefile(hf_path, mlx_path):
        raise ValueError("mlx_path is the source directory")
    print("[INFO] Loading")
    config = utils.load_config(hf_path)
    _family(config)
    weights = utils.read_sanitized_weights(hf_path, utils.sanitizer(config), config)

    dtype = _resolve_dtype(config, dtype)
    if quantize and dtype is not None and dtype != "bfloat16":
        raise NotImplementedError(f"quantize=True with dtype {dtype!r}: the quantize kernel reads bfloat16 and scales / biases "
                                  "are stored in the model dtype - pass dtype=\"bfloat16\"")
    if dtype in MODEL_CONVERSION_DTYPES:
        print("[INFO] Using dtype:", dtype)
        td = getattr(torch, dtype)
        weights = {k: (v.to(td) if v.is_floating_point() else v) for k, v in weights.items()}

    if quantize:
        if any(k.endswith(".scales") for k in weights):
            raise ValueError(f"{hf_path} is already quantized (it holds `.scales`); dequantize it first")
        paths = quantized_paths(weights, quant_predicate)
        not_bf16 = [p for p in paths if weights[p + ".weight"].dtype != torch.bfloat16]
        if not_bf16:
            raise NotImplementedError(f"{not_bf16[0]}.weight is {weights[not_bf16[0] + '.weight'].dtype} and the checkpoint "
                                      "names no dtype: the quantize kernel reads bfloat16 - pass dtype=\"bfloat16\"")
        print("[INFO] Quantizing")
        config.setdefault("vision_config", {})
        weights = _quantize_weights(weights, paths)
        config["quantization"] = {"group_size": Qz.GROUP, "bits": Qz.BITS, "mode": "affine"}
        config["quantization_config"] = config["quantization"]        # "support hf model tree" (quant_utils.py:105-106)
    if dequantize:
        print("[INFO] Dequantizing")
        weights = _dequantize_weights(weights)
        config.pop("quantization", None)
        config.pop("quantization_config", None)

    save_weights(mlx_path, {k: v.contiguous() for k, v in weights.items()})
    _copy_sidecars(hf_path, mlx_path)
    save_config(config, os.path.join(mlx_path, "config.json"))


def configure_parser() -> argparse.ArgumentParser:
    """the reference's flag names (convert.py:457-570) for what is built"""
    p = argparse.ArgumentParser(description="Convert a local Hugging Face or MLX checkpoint to MLX format")
    p.add_argument("--hf-path", "--model", type=str, required=True, help="Path to the source checkpoint directory.")
    p.add_argument("--mlx-path", type=str, default="mlx_model", help="Path to save the MLX model.")
    p.add_argument("-q", "--quantize", action="store_true", help="Generate a quantized model.")
    p.add_argument("--q-group-size", type=int, default=None, help="Group size for quantization (64).")
    p.add_argument("--q-bits", type=int, default=None, help="Bits per weight for quantization (4).")
    p.add_argument("--q-mode", type=str, default="affine", choices=["affine", "mxfp4", "nvfp4", "mxfp8"],
                   help="The quantization mode (affine).")
    p.add_argument("--dtype", type=str, default=None, choices=MODEL_CONVERSION_DTYPES,
                   help="Type to save the parameters in. Defaults to config.json's `torch_dtype`.")
    p.add_argument("-d", "--dequantize", action="store_true", default=False, help="Dequantize a quantized model.")
    return p


def main(argv=None):
    convert(**vars(configure_parser().parse_args(argv)))


# `mlx_vlm_amd.convert` names both this module and the function (as in the reference, whose package rebinds the name eagerly).
# The package imports lazily, so once this module is loaded the import system binds the MODULE on the package: make it
# callable, with the function's signature, so `from mlx_vlm_amd import convert` works in either order (as generate.py does).
import inspect as _inspect
import sys as _sys
import types as _types


class _CallableModule(_types.ModuleType):
    def __call__(self, *args, **kwargs):
        return convert(*args, **kwargs)


__signature__ = _inspect.signature(convert)
_sys.modules[__name__].__class__ = _CallableModule

if __name__ == "__main__":
    main()
