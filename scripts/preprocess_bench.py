"""What the device image path saves (profiles/device_preprocess.txt).  Two measurements, to be taken inside ONE GPU session
(box-to-box spread is 1.5x, docs/HISTORY.md); the yardstick of both is the host path on the same machine in the same run.

    python scripts/preprocess_bench.py matrix [--reps N]
        milliseconds from "uint8 ndarray [3, H, W] in host memory" to "the ViT's bf16 [N, patch_k] patch matrix on the device,
        stream synchronised", at 336x336, 480x640, 768x1024 and 1080x1920 (seeded random bytes), for
          host    Qwen2VLImageProcessor() (PIL resize, numpy patchify), the pinned upload of the fp32 rows and ops.cast_pad:
                  what VisionModel.__call__ does ahead of the patch GEMM
          device  Qwen2VLImageProcessor(device="cuda"): the pinned upload of the bytes, the cached tables, the HIP kernels
        alternating in one process, warmed, median of N >= 20 repetitions and min .. max.  The device path's kernels are also
        timed alone with device events (the bytes already uploaded).  Each size runs in two memory layouts of the [3, H, W]
        array: "decoded" - the transposed view of an [H, W, 3] array, which is what load_image returns for a PIL-decoded
        picture (both paths take the HWC bytes without a copy) - and "planar", a C-contiguous [3, H, W] array (both paths
        pay a strided copy to HWC first: PIL.Image.fromarray on the host path, the staging of the upload on the device path).

    python scripts/preprocess_bench.py ttft [--reps N]
        time to the first token of generate_step at Qwen2-VL-2B dimensions (synthetic weights) for a 768x1024 image and a
        16-token text, measured from the ndarray: processor, ViT, prefill, the first sampled token on the host.  It is
        generate_step that is timed, on pre-tokenised ids (no tokenizer or checkpoint is needed): what `generate` adds in
        front of it, the chat template and the tokenizer, is the same work on both paths and is not in the figure.
"""
import argparse
import os
import sys
import time

SIZES = ((336, 336), (480, 640), (768, 1024), (1080, 1920))


def _stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def matrix_table(reps):
    import numpy as np
    import torch
    from mlx_vlm_amd import _lib, image_ops, ops
    from mlx_vlm_amd.models.qwen2_vl.processing_qwen2_vl import Qwen2VLImageProcessor, smart_resize

    dev = "cuda"
    host_p, dev_p = Qwen2VLImageProcessor(), Qwen2VLImageProcessor(device=dev)
    patch_k = image_ops.patch_k_for(1176)

    def host(img):
        out = host_p([img])
        x = ops.cast_pad(_lib.h2d(out["pixel_values"], dev), patch_k)
        torch.cuda.synchronize()
        return x

    def device(img):
        x = image_ops.patch_matrix_of(dev_p([img])["pixel_values"], 1176, patch_k)
        torch.cuda.synchronize()
        return x

    print(f"ndarray -> bf16 [N, {patch_k}] on the device, ms (median of {reps}, alternating; min .. max)")
    for H, W, layout in [(h, w, l) for h, w in SIZES for l in ("decoded", "planar")]:
        img = np.transpose(np.random.default_rng(H).integers(0, 256, (H, W, 3), dtype=np.uint8), (2, 0, 1))
        if layout == "planar":
            img = np.ascontiguousarray(img)
        rh, rw = smart_resize(H, W)
        for _ in range(3):
            a, b = host(img), device(img)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), "the two paths must agree bit for bit"
        th, td = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            host(img)
            t1 = time.perf_counter()
            device(img)
            t2 = time.perf_counter()
            th.append((t1 - t0) * 1e3)
            td.append((t2 - t1) * 1e3)
        # the kernels alone: bytes resident, tables cached
        hwc = torch.from_numpy(np.ascontiguousarray(np.transpose(img, (1, 2, 0)))).to(dev)
        lut = dev_p._device_lut(dev)
        out = torch.empty((rh // 14) * (rw // 14), patch_k, dtype=torch.bfloat16, device=dev)
        tk = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.image_patches(hwc, rh, rw, "bicubic", lut, patch_k, out=out)
            e1.record()
            e1.synchronize()
            tk.append(e0.elapsed_time(e1))
        (mh, lh, hh), (md, ld, hd), (mk, lk, hk) = _stats(th), _stats(td), _stats(tk)
        print(f"  {H:4d} x {W:4d} -> {rh:4d} x {rw:4d}  {layout:<7s}  N = {out.shape[0]:5d}   host {mh:8.2f}  ({lh:.2f} .. {hh:.2f})   "
              f"device {md:7.3f}  ({ld:.3f} .. {hd:.3f})   host / device {mh / md:6.1f}   kernels alone {mk * 1e3:7.1f} us  "
              f"({lk * 1e3:.1f} .. {hk * 1e3:.1f})", flush=True)


def ttft_table(reps):
    import numpy as np
    import torch
    from mlx_vlm_amd import synthetic
    from mlx_vlm_amd.generate import generate_step
    from mlx_vlm_amd.models import qwen2_vl
    from mlx_vlm_amd.models.qwen2_vl.processing_qwen2_vl import Qwen2VLImageProcessor

    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = qwen2_vl.ModelConfig.from_dict(dict(synthetic.QWEN2_VL_2B))
    W = synthetic.random_weights(cfg, seed=0, device=dev)
    model = qwen2_vl.Model(cfg, device=dev, kv_pool_tokens=16384, max_seqs=4)
    model.load_weights(W)
    del W
    H, Wd = 768, 1024
    img = np.transpose(np.random.default_rng(H).integers(0, 256, (H, Wd, 3), dtype=np.uint8), (2, 0, 1))   # as load_image returns it
    procs = {"host": Qwen2VLImageProcessor(), "device": Qwen2VLImageProcessor(device="cuda")}
    n_img = procs["host"].num_image_tokens(H, Wd)
    text = np.random.default_rng(1).integers(0, 151643, 16)
    ids = np.concatenate([[cfg.vision_start_token_id], np.full(n_img, cfg.image_token_id), [cfg.vision_start_token_id + 1],
                          text]).astype(np.int64)[None]

    def first_token(path):
        t0 = time.perf_counter()
        out = procs[path]([img])
        pv = out["pixel_values"]
        gen = generate_step(ids, model, torch.from_numpy(pv) if isinstance(pv, np.ndarray) else pv, None, max_tokens=2,
                            temperature=0.0, image_grid_thw=out["image_grid_thw"], return_logprobs=False)
        tok, _ = next(gen)
        tok = int(tok)
        dt = (time.perf_counter() - t0) * 1e3
        for _ in gen:
            pass
        return tok, dt

    for _ in range(2):
        ta, tb = first_token("host")[0], first_token("device")[0]
    assert ta == tb, (ta, tb)
    res = {"host": [], "device": []}
    for _ in range(reps):
        for path in ("host", "device"):
            res[path].append(first_token(path)[1])
    print(f"time to first token of generate_step, Qwen2-VL-2B dimensions, {H} x {Wd} image ({n_img} image tokens) + 16 text tokens, from the "
          f"ndarray, ms (median of {reps}, alternating; min .. max)")
    for path in ("host", "device"):
        m, lo, hi = _stats(res[path])
        print(f"  {path:<7s} {m:8.2f}  ({lo:.2f} .. {hi:.2f})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["matrix", "ttft"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps: at least 20 repetitions")
    sys.path.insert(0, os.path.abspath(args.root))
    t0 = time.perf_counter()
    if args.what == "matrix":
        matrix_table(args.reps)
    else:
        ttft_table(args.reps)
    print(f"  ({time.perf_counter() - t0:.0f} s)", flush=True)


if __name__ == "__main__":
    main()
