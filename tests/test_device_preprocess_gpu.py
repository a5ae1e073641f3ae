"""Image preprocessing on the device (csrc/image_preprocess.hip through vlm_cast_f32_bf16_pad's image mode), held to the host
path bit for bit at every stage: the resized u8 frame against PIL, the bf16 patch matrix against the cast of the host
processor's fp32 rows, and - because those are equal - image features, tokens and log-probs of the tiny model.  Nothing here
has a tolerance: the kernels are integer arithmetic and a table lookup."""
import ctypes as C

import numpy as np
import pytest
import torch
from PIL import Image

from mlx_vlm_amd import _lib, image_ops, ops
from mlx_vlm_amd.models.qwen2_vl.processing_qwen2_vl import Qwen2VLImageProcessor
from oracle import image_processor as oip
from oracle import qwen2_vl as oq
from tests.helpers import build_product_model

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = "cuda"
PIL_FILTER = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}
SHAPES = [((40, 60), (56, 84)), ((37, 91), (28, 84)), ((300, 200), (112, 84)), ((100, 64), (224, 140)), ((17, 500), (28, 784)),
          ((64, 64), (56, 64)),        # vertical pass only
          ((480, 640), (476, 644)),
          ((56, 70), (56, 84))]        # horizontal pass only
PATCH_DIM, PATCH_K = 1176, 1216


def _pil(img_hwc, rh, rw, filter):
    return np.array(Image.fromarray(img_hwc).resize((rw, rh), resample=PIL_FILTER[filter]))


def _device_resize(img_dev, rh, rw, filter):
    _, frame = ops.image_patches(img_dev, rh, rw, filter, None, return_frame=True)
    return frame.cpu().numpy()


@pytest.mark.parametrize("filter", ["bicubic", "bilinear"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_resized_frame_equals_pillow(shape, filter):
    (H, W), (rh, rw) = shape
    img = np.random.default_rng(H * 1000 + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    got = _device_resize(torch.from_numpy(img).to(DEV), rh, rw, filter)
    assert np.array_equal(got, _pil(img, rh, rw, filter))


@pytest.mark.parametrize("filter", ["bicubic", "bilinear"])
@pytest.mark.parametrize("kind", ["zeros", "full", "checkerboard"])
def test_resize_at_both_ends_of_the_clamp(kind, filter):
    """bicubic overshoots around a 0 / 255 edge: the accumulator leaves [0, 255 << 22] on both sides and the clamp decides"""
    H, W = 37, 91
    img = {"zeros": np.zeros((H, W, 3), np.uint8), "full": np.full((H, W, 3), 255, np.uint8),
           "checkerboard": (((np.add.outer(np.arange(H), np.arange(W)) & 1) * 255).astype(np.uint8)[:, :, None]
                            * np.ones((1, 1, 3), np.uint8))}[kind]
    for rh, rw in ((56, 140), (28, 84)):
        assert np.array_equal(_device_resize(torch.from_numpy(img).to(DEV), rh, rw, filter), _pil(img, rh, rw, filter))


def test_resize_of_a_strided_source():
    H, W, rh, rw = 37, 91, 56, 84
    wide = np.random.default_rng(8).integers(0, 256, (H, W + 9, 3), dtype=np.uint8)
    view = torch.from_numpy(wide).to(DEV)[:, 4:4 + W]
    assert view.stride(0) == (W + 9) * 3 and not view.is_contiguous()
    img = np.ascontiguousarray(wide[:, 4:4 + W])
    assert np.array_equal(_device_resize(view, rh, rw, "bicubic"), _pil(img, rh, rw, "bicubic"))
    # one pass alone reads the strided source too: vertical only, then horizontal only
    assert np.array_equal(_device_resize(view, 56, W, "bicubic"), _pil(img, 56, W, "bicubic"))
    assert np.array_equal(_device_resize(view, H, 84, "bicubic"), _pil(img, H, 84, "bicubic"))


# ------------------------------------------------------------------------------------------------ patch matrix
_HOST = Qwen2VLImageProcessor()
_DEVP = Qwen2VLImageProcessor(device=DEV)


def _host_matrix(images):
    """what the ViT reads on the host path: the cast of the fp32 rows, zero padded"""
    out = _HOST(images)
    return ops.cast_pad(_lib.h2d(out["pixel_values"], DEV), PATCH_K), out["image_grid_thw"]


@pytest.mark.parametrize("size", [(56, 56), (40, 60), (300, 200)], ids=lambda s: "%dx%d" % s)
def test_patch_matrix_equals_cast_of_the_host_rows(size):
    img = np.random.default_rng(size[0]).integers(0, 256, (3,) + size, dtype=np.uint8)
    ref, thw = _host_matrix([img])
    out = _DEVP([img])
    pv = out["pixel_values"]
    assert pv.is_cuda and pv.dtype == BF and tuple(pv.shape) == (ref.shape[0], PATCH_DIM)
    buf = image_ops.patch_matrix_of(pv, PATCH_DIM, PATCH_K)
    assert buf is not None and tuple(buf.shape) == tuple(ref.shape)
    assert torch.equal(buf.view(torch.int16), ref.view(torch.int16))
    assert np.array_equal(out["image_grid_thw"], thw) and out["image_grid_thw"].dtype == thw.dtype
    # the pad columns are WRITTEN as zeros: an output buffer full of NaN bit patterns comes out equal as well
    rh, rw = int(thw[0, 1]) * 14, int(thw[0, 2]) * 14
    dirty = torch.full((ref.shape[0], PATCH_K), float("nan"), dtype=BF, device=DEV)
    hwc = torch.from_numpy(np.ascontiguousarray(np.transpose(img, (1, 2, 0)))).to(DEV)
    ops.image_patches(hwc, rh, rw, "bicubic", _DEVP._device_lut(DEV), PATCH_K, out=dirty)
    assert torch.equal(dirty[:, PATCH_DIM:].view(torch.int16), torch.zeros_like(dirty[:, PATCH_DIM:]).view(torch.int16))
    assert torch.equal(dirty.view(torch.int16), ref.view(torch.int16))


def test_several_images_land_in_one_matrix():
    rng = np.random.default_rng(11)
    imgs = [rng.integers(0, 256, (3, 40, 60), dtype=np.uint8), rng.integers(0, 256, (3, 84, 56), dtype=np.uint8)]
    ref, thw = _host_matrix(imgs)
    out = _DEVP(imgs)
    buf = image_ops.patch_matrix_of(out["pixel_values"], PATCH_DIM, PATCH_K)
    assert buf is not None and torch.equal(buf.view(torch.int16), ref.view(torch.int16))
    assert np.array_equal(out["image_grid_thw"], thw)
    parts = [_host_matrix([im])[0] for im in imgs]
    assert torch.equal(buf.view(torch.int16), torch.cat(parts).view(torch.int16))


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def tiny():
    cfg = oq.tiny_cfg()
    W = oq.random_weights(cfg, seed=1234, dtype=BF, std=0.05, embed_std=0.2)
    return cfg, build_product_model(cfg, W, kv_pool_tokens=4096, max_seqs=4)


def _request(cfg, size, n_text, seed):
    """-> (ids [1, L], u8 image [3, H, W], host pixel_values, grid)"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (3,) + size, dtype=np.uint8)
    host = _HOST([img])
    ids = [cfg.vision_start_token_id, cfg.image_token_id, cfg.vision_start_token_id + 1] + rng.integers(3, 1000, n_text).tolist()
    ids = oip.expand_image_placeholders(ids, cfg.image_token_id, host["image_grid_thw"])
    return np.array([ids], dtype=np.int64), img, host["pixel_values"], host["image_grid_thw"]


def test_encode_image_features_are_bit_equal(tiny):
    cfg, model = tiny
    _, img, pix, thw = _request(cfg, (40, 60), 4, seed=41)
    dev = _DEVP([img])
    a = model.encode_image(torch.from_numpy(pix), image_grid_thw=thw)
    b = model.encode_image(dev["pixel_values"], image_grid_thw=dev["image_grid_thw"])
    assert a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))
    # a bf16 tensor nobody vouches for (a copy drops the tag) goes the ordinary way and gives the same features
    c = model.encode_image(dev["pixel_values"].clone(), image_grid_thw=thw)
    assert torch.equal(a.view(torch.int16), c.view(torch.int16))


def test_generate_step_tokens_and_logprobs_are_bit_equal(tiny):
    from mlx_vlm_amd.generate import generate_step

    cfg, model = tiny
    ids, img, pix, thw = _request(cfg, (40, 60), 10, seed=42)
    dev = _DEVP([img])

    def run(pv, grid):
        toks, lps = [], []
        for t, lp in generate_step(ids, model, pv, None, max_tokens=8, temperature=0.0, image_grid_thw=grid):
            toks.append(t)
            lps.append(lp.clone())
        return toks, torch.stack(lps)

    ta, la = run(torch.from_numpy(pix), thw)
    tb, lb = run(dev["pixel_values"], dev["image_grid_thw"])
    assert len(ta) == 8 and ta == tb
    assert torch.equal(la.view(torch.int16), lb.view(torch.int16))


def test_batch_generate_ids_with_device_pixel_values(tiny):
    from mlx_vlm_amd.generate import batch_generate_ids

    cfg, model = tiny
    reqs = [_request(cfg, (40, 60), 8, seed=43), _request(cfg, (84, 56), 11, seed=44)]
    host, _ = batch_generate_ids(model, [r[0].reshape(-1) for r in reqs], [torch.from_numpy(r[2]) for r in reqs],
                                 [r[3] for r in reqs], max_tokens=8)
    devs = [_DEVP([r[1]]) for r in reqs]
    got, _ = batch_generate_ids(model, [r[0].reshape(-1) for r in reqs], [d["pixel_values"] for d in devs],
                                [d["image_grid_thw"] for d in devs], max_tokens=8)
    assert got == host and all(len(t) == 8 for t in got)


def test_batch_generator_admits_device_pixel_values(tiny):
    """the continuous generator runs the ViT of an admission on its side stream, which it gates on an event of the stream that
    calls next(): pixel_values made on that stream (the processor's current stream) are complete before the tower reads them"""
    from mlx_vlm_amd.batch import generate_batch_continuous

    cfg, model = tiny
    reqs = [_request(cfg, (40, 60), 8, seed=45), _request(cfg, (84, 56), 11, seed=46), _request(cfg, (56, 56), 6, seed=47)]
    ids = [r[0].reshape(-1) for r in reqs]
    host, _ = generate_batch_continuous(model, ids, [torch.from_numpy(r[2]) for r in reqs], [r[3] for r in reqs], max_tokens=6,
                                        batch_size=2)
    devs = [_DEVP([r[1]]) for r in reqs]
    got, _ = generate_batch_continuous(model, ids, [d["pixel_values"] for d in devs], [d["image_grid_thw"] for d in devs],
                                       max_tokens=6, batch_size=2)
    assert got == host and all(len(t) == 6 for t in got)


# ------------------------------------------------------------------------------------------------ bad arguments
def test_bad_arguments_return_an_error_and_launch_nothing():
    H, W, rh, rw = 40, 60, 56, 84
    img = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (H, W, 3), dtype=np.uint8)).to(DEV)
    th, tv = image_ops.device_tables(W, rw, "bicubic", DEV), image_ops.device_tables(H, rh, "bicubic", DEV)
    lut = _DEVP._device_lut(DEV)
    n = (rh // 14) * (rw // 14)
    out = torch.full((n, PATCH_K), 3.0, dtype=BF, device=DEV)
    frame = torch.full((rh, rw, 3), 7, dtype=torch.uint8, device=DEV)
    tmp = torch.full((H, rw, 3), 7, dtype=torch.uint8, device=DEV)
    L = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(ld_dst=PATCH_K, cols=PATCH_DIM, rows=n, dst_offset=0, **over):
        kw = dict(src=img.data_ptr(), height=H, width=W, src_stride=W * 3, resized_height=rh, resized_width=rw,
                  coeffs_h=th[0].data_ptr(), bounds_h=th[1].data_ptr(), ksize_h=th[2], coeffs_v=tv[0].data_ptr(),
                  bounds_v=tv[1].data_ptr(), ksize_v=tv[2], tmp_h=tmp.data_ptr(), frame=frame.data_ptr(), lut=lut.data_ptr(),
                  patch=14, merge=2, temporal=2, row_offset=0)
        kw.update(over)
        a = _lib.ImagePatchArgs(**kw)
        return L.vlm_cast_f32_bf16_pad(C.cast(C.pointer(a), C.c_void_p), C.c_void_p(out.data_ptr() + dst_offset), rows, cols,
                                       _lib.CAST_PAD_IMAGE_MODE, ld_dst, stream)

    ARG, SHAPE = 1, 2
    assert call(frame=None) == ARG and call(tmp_h=None) == ARG                  # null workspaces
    assert call(resized_width=rw + 14) == SHAPE                                 # rw is no multiple of patch * merge
    assert call(ld_dst=PATCH_DIM - 8) == ARG                                    # ld_dst < 1176
    assert call(ld_dst=PATCH_DIM + 4) == SHAPE                                  # rows would not be 16-byte aligned
    assert call(cols=PATCH_DIM - 1) == SHAPE and call(lut=None) == ARG and call(src=None) == ARG
    assert call(coeffs_h=None) == SHAPE                                         # a skipped pass must keep the size
    assert call(row_offset=1) == ARG and call(rows=n - 1) == ARG                # the image does not fit dst
    assert call(dst_offset=2) == ARG                                            # dst is not 16-byte aligned
    assert call(src_stride=W * 3 - 1) == ARG and call(bounds_v=None) == ARG and call(ksize_h=0) == ARG
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((frame == 7).all()) and bool((tmp == 7).all())   # nothing ran
    # the same arguments, unbroken, run
    assert call() == 0
    torch.cuda.synchronize()
    ref, _ = _host_matrix([np.ascontiguousarray(np.transpose(img.cpu().numpy(), (2, 0, 1)))])
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
    with pytest.raises(ValueError):
        ops.image_patches(img.to(torch.float32), rh, rw)
    with pytest.raises(_lib.VlmHipError):
        ops.image_patches(img.cpu(), rh, rw)
