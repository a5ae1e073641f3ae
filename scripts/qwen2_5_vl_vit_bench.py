"""Qwen2.5-VL vision tower: the window blocks' attention on the one-tile kernel (csrc/attn_window.hip) against the general varlen
kernel (vlm_attn_prefill over the same window table - the kernel every other tower uses), and the whole tower both ways.

    python scripts/qwen2_5_vl_vit_bench.py [--out profiles/qwen2_5_vl_window_attn.txt] [--depth 32] [--repeats 7]

Real tower widths (1280 / 16 heads / 3420 / out 2048, depth 32, fullatt [7, 15, 23, 31]), seeded weights; one 448 x 448 image
(grid 32 x 32: N = 1024 patch rows, 16 windows of 64) and 16 of them.  Every figure is the median over `--repeats` timed windows
of device-event time, the two sides ALTERNATING inside one process, each window long enough to be far above the event clock;
the spread printed next to it is (max - min) / median over the same windows.  The attention launch is timed as a captured graph
of 100 launches (a Python loop of single launches measures the ~12 us enqueue, not a kernel of a few us; its figure is printed
too, labelled); the whole tower is timed as a user runs it, one eager call after the other.  The rule is evaluated on the
graph-replayed launch and on the eager tower.  Outputs of the two routes are compared on the timed inputs before anything is
timed.  Needs a GPU: there is no fallback.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

E, H, D, INTER, OUT = 1280, 16, 80, 3420, 2048
FULLATT = [7, 15, 23, 31]


def seeded_tower(depth, seed=0):
    from mlx_vlm_amd.models.qwen2_5_vl import VisionConfig, VisionModel

    full = [i for i in FULLATT if i < depth] or [depth - 1]
    cfg = VisionConfig(depth=depth, hidden_size=E, intermediate_size=INTER, out_hidden_size=OUT, num_heads=H,
                       fullatt_block_indexes=full)
    g = torch.Generator().manual_seed(seed)
    bf = torch.bfloat16

    def rn(*shape, s=0.02):
        return (torch.randn(*shape, generator=g) * s).to(bf)

    W = {"patch_embed.proj.weight": rn(E, 2, 14, 14, 3)}
    for i in range(depth):
        p = f"blocks.{i}."
        W[p + "norm1.weight"], W[p + "norm2.weight"] = (1 + rn(E, s=0.05).float()).to(bf), (1 + rn(E, s=0.05).float()).to(bf)
        W[p + "attn.qkv.weight"], W[p + "attn.qkv.bias"] = rn(3 * E, E), rn(3 * E)
        W[p + "attn.proj.weight"], W[p + "attn.proj.bias"] = rn(E, E), rn(E)
        for n in ("gate_proj", "up_proj"):
            W[p + f"mlp.{n}.weight"], W[p + f"mlp.{n}.bias"] = rn(INTER, E), rn(INTER)
        W[p + "mlp.down_proj.weight"], W[p + "mlp.down_proj.bias"] = rn(E, INTER), rn(E)
    W["merger.ln_q.weight"] = (1 + rn(E, s=0.05).float()).to(bf)
    W["merger.mlp.0.weight"], W["merger.mlp.0.bias"] = rn(4 * E, 4 * E), rn(4 * E)
    W["merger.mlp.2.weight"], W["merger.mlp.2.bias"] = rn(OUT, 4 * E), rn(OUT)
    vm = VisionModel(cfg)
    vm.load_weights(W)
    return vm


def timed(fn, iters):
    """device-event milliseconds of `iters` back-to-back calls"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def graphed(fn, n):
    """fn() n times as ONE captured graph -> its replay (launch boundaries inside a graph instead of host enqueues)"""
    fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            for _ in range(n):
                fn()
    torch.cuda.current_stream().wait_stream(side)
    g.replay()
    torch.cuda.synchronize()
    return g


def alternate(sides, iters, repeats):
    """sides: name -> callable.  -> name -> list of per-call microseconds, one per repeat, the sides taking turns"""
    for fn in sides.values():                 # warm every shape
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res = {n: [] for n in sides}
    for _ in range(repeats):
        for n, fn in sides.items():
            res[n].append(timed(fn, iters) * 1e3 / iters)
    return res


def line(name, xs):
    med = statistics.median(xs)
    return med, f"{name:34s} median {med:9.2f} us   min {min(xs):9.2f}   max {max(xs):9.2f}   spread {(max(xs) - min(xs)) / med * 100:5.1f} %"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qwen2_5_vl_window_attn.txt"))
    ap.add_argument("--depth", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs an MI355X"
    from mlx_vlm_amd import ops
    from mlx_vlm_amd.models.qwen2_5_vl.vision import host_tables

    arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "")
    out = [f"Qwen2.5-VL window attention: one-tile kernel vs the general varlen kernel ({torch.cuda.get_device_name(0)}, {arch})",
           f"tower 1280 / 16 heads of 80 / intermediate 3420 (3456 padded) / out 2048, depth {args.depth}, seeded weights",
           "times: device events, per call, median of %d alternating windows; spread = (max - min) / median" % args.repeats, ""]
    vm = seeded_tower(args.depth)
    verdict = []
    for n_img in (1, 16):
        grids = np.array([[1, 32, 32]] * n_img)
        N = int(grids.prod(axis=1).sum())
        t = host_tables(grids, 112, 2, 14)
        lens = np.diff(t["cu_window"])
        assert lens.max() == 64 and lens.min() == 64 and len(lens) == 16 * n_img
        cu = torch.from_numpy(t["cu_window"]).cuda()
        nqb = int(sum((int(l) + 127) // 128 for l in lens))
        qkv = (torch.randn(N, 3 * E, generator=torch.Generator().manual_seed(n_img)) * 1.0).to(torch.bfloat16).cuda()
        o1, o2 = torch.empty(N, E, dtype=torch.bfloat16, device="cuda"), torch.empty(N, E, dtype=torch.bfloat16, device="cuda")
        general = lambda: ops.attn_prefill(qkv, qkv[:, E:], qkv[:, 2 * E:], cu, nqb, H, H, D, D ** -0.5, False, out=o1)   # noqa: E731
        window = lambda: ops.attn_prefill(qkv, qkv[:, E:], qkv[:, 2 * E:], cu, None, H, H, D, D ** -0.5, False, out=o2,    # noqa: E731
                                          one_tile_max_seg=64)
        general(); window(); torch.cuda.synchronize()
        rel = float((o1.float() - o2.float()).pow(2).mean().sqrt() / o1.float().pow(2).mean().sqrt())
        out.append(f"--- {n_img} x 448^2 (N = {N}, {len(lens)} windows of 64, {len(lens) * H} (segment, head) pairs)")
        out.append(f"outputs of the two kernels on these inputs: rel-rms {rel:.2e}")
        r = alternate({"general": general, "one_tile": window}, iters=400, repeats=args.repeats)
        _, lg = line("eager loop (enqueue-bound), general", r["general"])
        _, lw = line("eager loop (enqueue-bound), one-tile", r["one_tile"])
        out += [lg, lw]
        gg, gw = graphed(general, 100), graphed(window, 100)
        r = alternate({"general": gg.replay, "one_tile": gw.replay}, iters=20, repeats=args.repeats)
        r = {k: [x / 100 for x in v] for k, v in r.items()}
        mg, lg = line("attention launch, general kernel", r["general"])
        mw, lw = line("attention launch, one-tile kernel", r["one_tile"])
        out += [lg, lw, f"  one-tile / general = {mw / mg:.3f}"]
        sg = (max(r["general"]) - min(r["general"])) / mg
        attn_faster = mw < mg * (1 - sg)
        # whole tower, both ways (the knob is read at call time)
        pix = (torch.rand(N, 1176, generator=torch.Generator().manual_seed(7)) * 2 - 1).cuda()

        def tower(v):
            def f():
                os.environ["VLM_VIT_WINDOW_ATTN"] = v
                return vm(pix, grids)
            return f

        a, b = tower("0")().float(), tower("1")().float()
        torch.cuda.synchronize()
        out.append(f"tower outputs of the two routes: rel-rms {float((a - b).pow(2).mean().sqrt() / a.pow(2).mean().sqrt()):.2e}")
        r = alternate({"general": tower("0"), "one_tile": tower("1")}, iters=60 if n_img == 1 else 10, repeats=args.repeats)
        tg, l1 = line("whole tower, general kernel", r["general"])
        tw, l2 = line("whole tower, one-tile kernel", r["one_tile"])
        out += [l1, l2, f"  one-tile / general = {tw / tg:.3f}", ""]
        stg = (max(r["general"]) - min(r["general"])) / tg
        tower_faster, tower_slower = tw < tg * (1 - stg), tw > tg * (1 + stg)
        verdict.append(attn_faster and not tower_slower)
        out.append(f"  beyond the baseline's spread: attention launch faster {attn_faster}; whole tower faster {tower_faster}, "
                   f"slower {tower_slower}")
        out.append("")
    os.environ.pop("VLM_VIT_WINDOW_ATTN", None)
    out.append("rule: the one-tile kernel is the tower's default only if its launch is faster than the general kernel's at BOTH "
               "shapes by more than the run-to-run spread of that baseline (and the whole tower is at no shape slower beyond its "
               "spread); the whole-tower lines say what of it a user sees")
    out.append(f"result: one-tile kernel as default = {all(verdict)}")
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
