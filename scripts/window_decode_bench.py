"""Decode speed of generate_step(max_kv_size=) with a FULL window, Qwen2-VL-2B dimensions (synthetic weights), one sequence,
greedy - three arms:

  parent     generate_step(max_kv_size=M) of ANOTHER checkout of this repository (--parent-tree: the commit before the
             device-resident window, whose bounded generation runs the eager loop: a host plan, an upload, a move launch, an
             un-captured forward and an .item() per token);
  window     this tree's generate_step(max_kv_size=M): captured window steps (include/vlm_hip.h VLM_DECODE_WINDOW);
  unbounded  this tree's captured decode without a bound at a context that ends at M tokens (so both captured arms take the same
             attention decomposition: nsplit = 1).

The window arms get a text prompt LONGER than M (the L > M start state); every arm generates --tokens tokens and reports
(tokens - 1) / (time from the first to the last yield).  One worker process per tree holds its model; the driver alternates the
arms inside every one of --repeats repeats (a warm-up generation per arm first) and reports median [min .. max] tok/s.

    python scripts/window_decode_bench.py [--parent-tree DIR] [--out FILE]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def worker(tree, M, n_tokens):
    sys.path.insert(0, tree)
    import numpy as np
    import torch

    from mlx_vlm_amd import _lib, synthetic
    from mlx_vlm_amd.generate import generate_step
    from mlx_vlm_amd.models import qwen2_vl

    torch.cuda.set_device(0)
    cfg = qwen2_vl.ModelConfig.from_dict(dict(synthetic.QWEN2_VL_2B))
    W = synthetic.random_weights(cfg, seed=0, device="cuda")
    model = qwen2_vl.Model(cfg, device="cuda", kv_pool_tokens=8192, max_seqs=4)
    model.load_weights(W)
    del W
    rng = np.random.default_rng(7)
    long_ids = rng.integers(1000, 100000, (1, M + M // 8))
    short_ids = long_ids[:, : M - n_tokens - 2]
    print("ready", flush=True)
    for line in sys.stdin:
        arm = line.strip()
        if not arm:
            break
        kw = dict(max_tokens=n_tokens, temperature=0.0, return_logprobs=False, prefill_step_size=None)
        ids = short_ids if arm == "unbounded" else long_ids
        if arm != "unbounded":
            kw["max_kv_size"] = M
        stamps = []
        for _ in generate_step(ids, model, None, None, **kw):
            stamps.append(time.perf_counter())
        launches = _lib.lib().vlm_llm_decode_launches(model.language_model._handle)
        print(f"{(len(stamps) - 1) / (stamps[-1] - stamps[0]):.3f} {launches}", flush=True)


class Worker:
    def __init__(self, tree, M, n_tokens):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree, "--window", str(M),
                                   "--tokens", str(n_tokens)], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        assert self.p.stdout.readline().strip() == "ready", "worker did not start"

    def run(self, arm):
        self.p.stdin.write(arm + "\n")
        self.p.stdin.flush()
        rate, launches = self.p.stdout.readline().split()
        return float(rate), int(launches)

    def close(self):
        self.p.stdin.close()
        self.p.wait(timeout=60)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(HERE))
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--window", type=int, default=2048)
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args.tree, args.window, args.tokens)
    arms = []
    here = Worker(args.tree, args.window, args.tokens)
    parent = Worker(args.parent_tree, args.window, args.tokens) if args.parent_tree else None
    if parent:
        arms.append(("parent", parent, "window"))
    arms += [("window", here, "window"), ("unbounded", here, "unbounded")]
    try:
        launches = {}
        for name, w, arm in arms:               # warm-up: graph capture, allocator, first-touch
            launches[name] = w.run(arm)[1]
        t = {name: [] for name, _, _ in arms}
        for _ in range(args.repeats):
            for name, w, arm in arms:
                t[name].append(w.run(arm)[0])
    finally:
        here.close()
        if parent:
            parent.close()
    lines = [f"Qwen2-VL-2B dimensions, one sequence, greedy, max_kv_size = {args.window}, prompt {args.window + args.window // 8} tokens "
             f"(unbounded arm: {args.window - args.tokens - 2}), {args.tokens} tokens per generation; tok/s from the first to the last "
             f"yield, median [min .. max] of {args.repeats} repeats, arms alternated in every repeat"]
    med = {}
    for name, _, _ in arms:
        v = t[name]
        med[name] = statistics.median(v)
        lines.append(f"{name:10s} {med[name]:9.1f} tok/s [{min(v):9.1f} .. {max(v):9.1f}]  spread {(max(v) - min(v)) / med[name] * 100:5.1f} %  "
                     f"launches in the last step enqueued {launches[name]}")
    if "parent" in med:
        lines.append(f"window / parent = {med['window'] / med['parent']:.2f} x")
    lines.append(f"window / unbounded = {med['window'] / med['unbounded']:.3f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
