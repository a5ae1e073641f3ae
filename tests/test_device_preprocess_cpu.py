"""Image preprocessing on the device, host side (no GPU): the resampling tables the HIP kernels of
csrc/image_preprocess.hip read must be Pillow's.  `image_ops.resample_coeffs` + the numpy emulation of the two integer passes
(`resize_u8_reference` below: what the kernels compute, operation for operation) is held to `PIL.Image.resize` bit for
bit; the GPU tests then hold the kernels to the same images.  Also here: the default processor did not change, the
`image_preprocess` keyword of `load_processor`, and the ctypes mirror of the header's struct."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
from PIL import Image

from mlx_vlm_amd import _lib, image_ops
from mlx_vlm_amd.models.qwen2_vl.processing_qwen2_vl import Qwen2VLImageProcessor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (H, W) -> (rh, rw)
SHAPES = [((40, 60), (56, 84)),        # upscale, ksize 5
          ((37, 91), (28, 84)),        # downscale, odd row bytes
          ((300, 200), (112, 84)),     # long kernels
          ((100, 64), (224, 140)),
          ((17, 500), (28, 784)),      # up in one axis, down in the other
          ((64, 64), (56, 64)),        # vertical pass only
          ((480, 640), (476, 644))]    # a photograph's near-identity resize
PIL_FILTER = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}


def _pass_reference(src, coeffs, bounds):
    """one resampling pass along axis 0 of u8 [in, ...] -> u8 [out, ...]: the kernels' arithmetic in int32"""
    bits = image_ops.PRECISION_BITS
    out = np.empty((coeffs.shape[0],) + src.shape[1:], dtype=np.uint8)
    s32 = src.astype(np.int32)
    for xx in range(coeffs.shape[0]):
        x0, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = np.full(src.shape[1:], 1 << (bits - 1), dtype=np.int32)
        for i in range(n):
            acc += s32[x0 + i] * coeffs[xx, i]
        out[xx] = np.clip(acc >> bits, 0, 255).astype(np.uint8)
    return out


def resize_u8_reference(image_hwc, rh, rw, filter="bicubic"):
    """numpy emulation of the device resize of u8 [H, W, C]: horizontal pass, rounding to u8, vertical pass; a pass whose
    size does not change is skipped"""
    H, W = image_hwc.shape[:2]
    x = image_hwc
    if rw != W:
        x = np.swapaxes(_pass_reference(np.swapaxes(x, 0, 1), *image_ops.resample_coeffs(W, rw, filter)), 0, 1)
    if rh != H:
        x = _pass_reference(x, *image_ops.resample_coeffs(H, rh, filter))
    return np.ascontiguousarray(x)


@pytest.mark.parametrize("filter", ["bicubic", "bilinear"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_coefficients_and_integer_passes_equal_pillow(shape, filter):
    (H, W), (rh, rw) = shape
    img = np.random.default_rng(H * 1000 + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    ref = np.array(Image.fromarray(img).resize((rw, rh), resample=PIL_FILTER[filter]))
    got = resize_u8_reference(img, rh, rw, filter)
    assert got.dtype == np.uint8 and got.shape == (rh, rw, 3)
    assert np.array_equal(got, ref), int((got != ref).sum())


def test_coefficient_table_layout_bounds_and_cache():
    k, b = image_ops.resample_coeffs(60, 84, "bicubic")
    assert k.dtype == np.int32 and b.dtype == np.int32 and k.shape == (84, 5) and b.shape == (84, 2)
    assert image_ops.resample_coeffs(300, 112, "bicubic")[0].shape == (112, 2 * 6 + 1)      # support 2 * 300 / 112 = 5.36
    assert image_ops.resample_coeffs(300, 112, "bilinear")[0].shape == (112, 2 * 3 + 1)
    for n_in, n_out, f in ((60, 84, "bicubic"), (91, 84, "bilinear"), (7, 56, "bicubic"), (1920, 1316, "bicubic")):
        k, b = image_ops.resample_coeffs(n_in, n_out, f)
        assert (b[:, 0] >= 0).all() and (b[:, 1] >= 1).all() and (b[:, 1] <= k.shape[1]).all()
        assert (b[:, 0] + b[:, 1] <= n_in).all()
        assert all((k[i, b[i, 1]:] == 0).all() for i in range(n_out))                     # the entries past the taps are 0
        # the weights are normalised before they are rounded: every row sums to 2^22 within one rounding per tap
        assert (np.abs(k.sum(axis=1).astype(np.int64) - (1 << 22)) <= k.shape[1]).all()
        # |sum k| * 255 + 2^21 stays inside int32: the accumulator of the kernels cannot overflow
        assert (np.abs(k.astype(np.int64)).sum(axis=1) * 255 + (1 << 21) < (1 << 31)).all()
    assert image_ops.resample_coeffs(60, 84, "bicubic")[0] is image_ops.resample_coeffs(60, 84, "bicubic")[0]
    assert not image_ops.resample_coeffs(60, 84, "bicubic")[0].flags.writeable
    with pytest.raises(ValueError):
        image_ops.resample_coeffs(60, 84, "lanczos")
    with pytest.raises(ValueError):
        image_ops.resample_coeffs(0, 84, "bicubic")


def test_default_processor_is_the_host_path():
    """Qwen2VLImageProcessor() returns what it returned before: numpy fp32 rows, equal to the float path of _process_one"""
    proc = Qwen2VLImageProcessor()
    assert proc.device is None
    rng = np.random.default_rng(3)
    for (H, W) in ((56, 56), (40, 60), (300, 200)):
        img = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
        out = proc([img])
        pv = out["pixel_values"]
        assert isinstance(pv, np.ndarray) and pv.dtype == np.float32 and pv.shape[1] == 1176
        rh, rw = int(out["image_grid_thw"][0, 1]) * 14, int(out["image_grid_thw"][0, 2]) * 14
        frame = np.transpose(np.array(Image.fromarray(np.transpose(img, (1, 2, 0))).resize((rw, rh), resample=Image.BICUBIC)),
                             (2, 0, 1)) if (H, W) != (rh, rw) else img
        # the float path: float32 input of the same frame takes the branch without the byte table
        x = proc._normalise(frame.astype(np.float32), rescale=True)
        gh, gw = rh // 14, rw // 14
        ref = np.repeat(x[None, None], 2, axis=1).reshape(1, 1, 2, 3, gh // 2, 2, 14, gw // 2, 2, 14)
        ref = ref.transpose(0, 1, 4, 7, 5, 8, 3, 2, 6, 9).reshape(gh * gw, 1176)
        assert np.array_equal(pv, ref)
        # and the device path's frame is the host path's frame
        assert np.array_equal(resize_u8_reference(np.ascontiguousarray(np.transpose(img, (1, 2, 0))), rh, rw),
                              np.transpose(frame, (1, 2, 0)))


def test_device_processor_keeps_the_host_path_for_float_images_and_never_falls_back():
    import torch

    proc = Qwen2VLImageProcessor(device="cuda")
    f32 = np.random.default_rng(4).random((3, 56, 56), dtype=np.float32)
    out = proc([f32])
    assert isinstance(out["pixel_values"], np.ndarray) and np.array_equal(out["pixel_values"], Qwen2VLImageProcessor()([f32])["pixel_values"])
    if not torch.cuda.is_available():
        with pytest.raises(_lib.VlmHipError):
            proc([np.zeros((3, 56, 56), dtype=np.uint8)])


def _tokenizer_dir(tmp_path, conf):
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast

    (tmp_path / "config.json").write_text(json.dumps(conf))
    vocab = {"<unk>": 0, "<eos>": 1, "<pad>": 2, **{f"w{i}": i for i in range(3, 64)}}
    tok = Tokenizer(models.WordLevel(vocab, unk_token="<unk>"))
    tok.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    PreTrainedTokenizerFast(tokenizer_object=tok, eos_token="<eos>", pad_token="<pad>", unk_token="<unk>").save_pretrained(str(tmp_path))


def test_load_processor_wiring_and_refusal_for_other_families(tmp_path):
    from types import SimpleNamespace

    from mlx_vlm_amd.utils import load_processor

    _tokenizer_dir(tmp_path, {"model_type": "qwen2_vl"})
    (tmp_path / "preprocessor_config.json").write_text(json.dumps({"min_pixels": 3136, "max_pixels": 200704, "patch_size": 14}))
    cfg = SimpleNamespace(model_type="qwen2_vl", eos_token_id=1)
    host = load_processor(str(tmp_path), cfg)
    assert host.image_processor.device is None and host.image_processor.max_pixels == 200704
    dev = load_processor(str(tmp_path), cfg, image_preprocess="device")
    assert dev.image_processor.device == "cuda" and dev.image_processor.max_pixels == 200704
    with pytest.raises(ValueError):
        load_processor(str(tmp_path), cfg, image_preprocess="gpu")
    for mt in ("llava_bunny", "bunny-llama", "idefics2", "phi3_v"):
        with pytest.raises(NotImplementedError):
            load_processor(str(tmp_path), SimpleNamespace(model_type=mt, eos_token_id=1), image_preprocess="device")


def test_struct_mirror_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "vlm_hip.h")).read()
    body = re.search(r"typedef struct vlm_image_patch_args \{(.*?)\} vlm_image_patch_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "int": ctypes.c_int, "long long": ctypes.c_longlong}
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.match(r"(const void\*|void\*|long long|int) (.+)", decl)
        assert m, decl
        fields += [(name.strip(), ctype[m.group(1)]) for name in m.group(2).split(",")]
    assert fields == list(_lib.ImagePatchArgs._fields_)
    assert _lib.CAST_PAD_IMAGE_MODE == -1 and "ld_src == -1" in hdr
    # the mode travels through the operation it replaces: no new name, same ABI version
    assert len(set(re.findall(r"\b(vlm_[a-z0-9_]+)\s*\(", hdr))) == 60
    assert "vlm_image_patch_args" not in _lib.SIGNATURES
