"""Image preprocessing on the device: the host half.

Pillow's 8-bit resampler (`Image.resize` on an RGB image) is fixed-point arithmetic over a table of integer
coefficients: a horizontal pass, a rounding to u8, a vertical pass.  `resample_coeffs` reproduces that table
(Pillow's `precompute_coeffs` + `normalize_coeffs_8bpc`, src/libImaging/Resample.c) bit for bit, so the HIP kernels of
csrc/image_preprocess.hip, which only multiply and shift, give Pillow's bytes (tests/test_device_preprocess_cpu.py holds
the table, with a numpy emulation of the two passes, to PIL on a machine without a GPU).

The rest is what the device path of the Qwen2-VL image processor needs around the kernels: the device copies of the
tables, cached per (in, out, filter), the bf16 rescale + normalise table, and the tag that lets the vision tower
take the processor's zero-padded patch matrix as it is."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import numpy as np

PRECISION_BITS = 32 - 8 - 2                      # Pillow's: an 8-bit pixel times a coefficient, summed, fits int32
FILTER_SUPPORT = {"bicubic": 2.0, "bilinear": 1.0}
PATCH_MATRIX_ATTR = "_vlm_patch_matrix"          # set by the device processor on its pixel_values (see tag_patch_matrix)


def _bicubic(x: np.ndarray) -> np.ndarray:
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def _bilinear(x: np.ndarray) -> np.ndarray:
    x = np.abs(x)
    return np.where(x < 1.0, 1.0 - x, 0.0)


_FILTERS = {"bicubic": _bicubic, "bilinear": _bilinear}
_coeff_cache: Dict[tuple, Tuple[np.ndarray, np.ndarray]] = {}


def resample_coeffs(in_size: int, out_size: int, filter: str = "bicubic") -> Tuple[np.ndarray, np.ndarray]:
    """-> (coeffs int32 [out_size, ksize], bounds int32 [out_size, 2] = (first source index, number of taps)): output
    sample xx is clip8((2^21 + sum_i src[xmin + i] * coeffs[xx, i]) >> 22).  All arithmetic is float64 in Pillow's
    order; the sum of the weights runs sequentially over the taps (np.sum adds pairwise and changes the last bit)."""
    if filter not in _FILTERS:
        raise ValueError(f"resample filter {filter!r}: bicubic and bilinear are built")
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"resample sizes must be positive, got {in_size} -> {out_size}")
    key = (in_size, out_size, filter)
    hit = _coeff_cache.get(key)
    if hit is not None:
        return hit
    f = _FILTERS[filter]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = FILTER_SUPPORT[filter] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)          # C's (int): toward zero
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    w = np.zeros((out_size, ksize), dtype=np.float64)
    ww = np.zeros(out_size, dtype=np.float64)
    for x in range(ksize):
        live = x < xmax
        wx = np.where(live, f((x + xmin - center + 0.5) * ss), 0.0)
        w[:, x] = wx
        ww = np.where(live, ww + wx, ww)
    w = np.where((ww != 0.0)[:, None], w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    fixed = w * float(1 << PRECISION_BITS)
    coeffs = np.where(w < 0, np.trunc(fixed - 0.5), np.trunc(fixed + 0.5)).astype(np.int32)
    bounds = np.stack([xmin, xmax], axis=1).astype(np.int32)
    # a table that points outside the image would make the kernels read a clamped (wrong) pixel: refuse it here
    if (bounds[:, 0] < 0).any() or (bounds[:, 1] < 0).any() or (bounds[:, 1] > ksize).any() \
            or (bounds[:, 0] + bounds[:, 1] > in_size).any():
        raise AssertionError(f"resample bounds leave the image for {in_size} -> {out_size} ({filter})")
    coeffs.setflags(write=False)
    bounds.setflags(write=False)
    if len(_coeff_cache) > 256:
        _coeff_cache.clear()
    _coeff_cache[key] = (coeffs, bounds)
    return coeffs, bounds


# ---------------------------------------------------------------------------------------------- device side
_device_tables: Dict[tuple, tuple] = {}


def device_tables(in_size: int, out_size: int, filter: str, device):
    """-> (coeffs, bounds, ksize) on `device`, or None when the pass is skipped (in_size == out_size).  Cached: a server
    sees the same sizes again and again, and the upload is two small copies.  The cache holds device memory for the life of
    the process: at most 256 tables of out_size * (ksize + 2) * 4 bytes, ~50 KB for a 1920 -> 1316 pass, then it is cleared."""
    import torch

    from . import _lib

    if in_size == out_size:
        return None
    key = (int(in_size), int(out_size), filter, str(torch.device(device)))
    hit = _device_tables.get(key)
    if hit is None:
        coeffs, bounds = resample_coeffs(in_size, out_size, filter)
        hit = (_lib.h2d(coeffs.copy(), device), _lib.h2d(bounds.copy(), device), int(coeffs.shape[1]))   # the cached arrays are read-only
        if len(_device_tables) > 256:
            _device_tables.clear()
        _device_tables[key] = hit
    return hit


def patch_k_for(patch_dim: int) -> int:
    """K of the patch GEMM: the row of C * T * ps * ps values zero padded to a multiple of 64 (models/qwen2_vl/vision.py)"""
    return (int(patch_dim) + 63) // 64 * 64


def tag_patch_matrix(buf, patch_dim: int):
    """buf: device bf16 [N, patch_k] whose columns patch_dim.. are zero (the caller vouches for it: it comes from the
    patchify kernel).  -> the logical [N, patch_dim] view, carrying `buf` so that the vision tower can feed the patch
    GEMM from it directly.  Strides alone would not prove the padding is zero; this attribute does, and any torch op on
    the view returns a tensor without it."""
    pv = buf[:, :patch_dim]
    setattr(pv, PATCH_MATRIX_ATTR, buf)
    return pv


def patch_matrix_of(pv, patch_dim: int, patch_k: int):
    """the zero-padded [N, patch_k] buffer behind a tagged pixel_values tensor, or None (then the tensor goes the
    ordinary way: fp32, cast_pad)"""
    import torch

    buf = getattr(pv, PATCH_MATRIX_ATTR, None)
    if buf is None or not isinstance(buf, torch.Tensor) or not isinstance(pv, torch.Tensor):
        return None
    if buf.dtype != torch.bfloat16 or not buf.is_cuda or buf.dim() != 2 or not buf.is_contiguous():
        return None
    if tuple(buf.shape) != (pv.shape[0], patch_k) or pv.shape[1] != patch_dim or pv.data_ptr() != buf.data_ptr() \
            or pv.stride() != buf.stride():
        return None
    return buf


def concat_patch_matrices(parts: List, patch_dim: Optional[int] = None):
    """dim-0 concatenation of tagged pixel_values of several requests that keeps the tag (one copy of the padded rows),
    or None when any part is not tagged - the caller then concatenates the ordinary way."""
    import torch

    bufs = [getattr(p, PATCH_MATRIX_ATTR, None) if isinstance(p, torch.Tensor) else None for p in parts]
    if not bufs or any(b is None for b in bufs):
        return None
    dims = {(p.shape[1], b.shape[1], b.device) for p, b in zip(parts, bufs)}
    if len(dims) != 1 or any(patch_matrix_of(p, p.shape[1], b.shape[1]) is None for p, b in zip(parts, bufs)):
        return None
    if len(parts) == 1:
        return parts[0]
    return tag_patch_matrix(torch.cat(bufs, dim=0), parts[0].shape[1])
