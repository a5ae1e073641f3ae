"""What each kernel of the one-row decode step does between its entry point and its first loads (CPU only).

    python scripts/kernarg_entry_report.py [--csrc DIR] [--no-preload] [--keep DIR]

Compiles the decode translation units to gfx950 assembly with the flags of mlx-vlm_amd/build.py and, for every kernel
of the one-row step, prints
  * the kernel-argument preload length (dwords delivered in SGPRs at wave start), VGPRs and waves per SIMD,
  * the kernel-argument scalar loads and the lgkmcnt waits that come
      (a) ahead of the first vector load,
      (b) ahead of the first weight load (non-temporal), or - in a kernel that has none - ahead of the last vector load
          of its first batch (the loads issued before the first wait on vmcnt).
A wait counts only while a kernel-argument load is outstanding.  With a preload length > 0 the walk starts at the
preload entry point (256-byte aligned, behind the compatibility prologue that firmware without the preload runs).

--csrc DIR     sources to compile (default: mlx-vlm_amd/csrc): point it at another checkout's csrc to compare
--no-preload   the same sources without -amdgpu-kernarg-preload-count (what VLM_NO_KERNARG_PRELOAD=1 builds)
Output of parent and branch: profiles/kernarg_preload.txt; with the attention's grid-z forms: profiles/latency_launches_ab.txt.
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (label, translation unit, regex on the mangled symbol) - the launches of a one-row greedy step, in step order
KERNELS = [
    ("qkv       gemv_rowwave_kernel<2,3,1,1,3072>  (bit 6, scalar entry)", "gemv_bf16", r"gemv_rowwave_kernelILi2ELi3ELi1ELi1ELi3072EE"),
    ("attention attn_decode_pagesplit_dz_kernel<6,true,4>", "attn_decode", r"attn_decode_pagesplit_dz_kernelILi6ELb1ELi4EE"),
    ("o_proj    gemv_rowwave_kernel<2,3,1,3,8>", "gemv_bf16", r"gemv_rowwave_kernelILi2ELi3ELi1ELi3ELi8EE"),
    ("gate/up   gemv_rowwave_kernel<2,3,1,1,16>", "gemv_bf16", r"gemv_rowwave_kernelILi2ELi3ELi1ELi1ELi16EE"),
    ("down      gemv_splitk_kernel<6,5,1,8>", "gemv_bf16", r"gemv_splitk_kernelILi6ELi5ELi1ELi8EE"),
    ("head      gemv_rowwave_kernel<2,3,1,1,0>", "gemv_bf16", r"gemv_rowwave_kernelILi2ELi3ELi1ELi1ELi0EE"),
    ("lse       lse_partial_kernel_regs  (bit 13)", "sample", r"lse_partial_kernel_regsE?PKt"),
    ("tail      logprob_argmax_tail_kernel", "sample", r"logprob_argmax_tail_kernelE?PKt"),
]
# the forms the attention launch takes under the other settings of bits 8, 9 of VLM_TUNE_GEMV_VARIANT; listed, not counted
ALTERNATES = [
    ("attention attn_decode_pagesplit_kernel<6,true,false>  (bits 8, 9 off)", "attn_decode", r"attn_decode_pagesplit_kernelILi6ELb1ELb0EE"),
    ("attention attn_decode_pagesplit_dz_kernel<6,true,2>  (bit 8)", "attn_decode", r"attn_decode_pagesplit_dz_kernelILi6ELb1ELi2EE"),
    # the forms the o_proj launch takes under bits 11, 12: a class of 4, and exactly S splits (PRO_ATTN_PS_BASE + S; an even
    # and an odd count - the odd one loads a pair it never uses)
    ("o_proj    gemv_rowwave_kernel<2,3,1,6,8>  (bit 11, 8 slots)", "gemv_bf16", r"gemv_rowwave_kernelILi2ELi3ELi1ELi6ELi8EE"),
    ("o_proj    gemv_rowwave_kernel<2,3,1,24,8>  (bit 12, 8 splits)", "gemv_bf16", r"gemv_rowwave_kernelILi2ELi3ELi1ELi24ELi8EE"),
    ("o_proj    gemv_rowwave_kernel<2,3,1,25,8>  (bit 12, 9 splits)", "gemv_bf16", r"gemv_rowwave_kernelILi2ELi3ELi1ELi25ELi8EE"),
    # bit 6 off: the qkv entry that waits for RopeKvArgs (more than one row, wide heads); bit 13 off: the two-pass lse; bit 14:
    # the greedy tail with its logits loads ahead of the partials'
    ("qkv       gemv_rowwave_kernel<2,3,1,1,1024>  (bit 6 off)", "gemv_bf16", r"gemv_rowwave_kernelILi2ELi3ELi1ELi1ELi1024EE"),
    ("lse       lse_partial_kernel  (bit 13 off)", "sample", r"lse_partial_kernelE?PKt"),
    ("tail      logprob_argmax_tail_kernel_lean  (bit 14)", "sample", r"logprob_argmax_tail_kernel_leanE?PKt"),
]


def load_build(no_preload: bool):
    if no_preload:
        os.environ["VLM_NO_KERNARG_PRELOAD"] = "1"
    spec = importlib.util.spec_from_file_location("vlm_build", os.path.join(ROOT, "mlx-vlm_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_asm(hipcc, flags, src, out):
    r = subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", src, "-o", out], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr}")
    return out


def function_text(lines, pat):
    """-> (symbol, body lines, descriptor lines) of the first kernel whose symbol matches."""
    rx = re.compile(r"^(_Z\w*" + pat + r"\w*):")
    for i, ln in enumerate(lines):
        m = rx.match(ln)
        if not m:
            continue
        sym = m.group(1)
        d0 = next(j for j in range(i, len(lines)) if lines[j].strip() == ".amdhsa_kernel " + sym)
        d1 = next(j for j in range(d0, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        return sym, lines[i + 1:d0], lines[d0:d1 + 40]      # (+ the compiler's summary comments behind the descriptor)
    return None, [], []


def descriptor(desc, key):
    for ln in desc:
        t = ln.replace(";", " ").replace(":", " ").split()
        if len(t) >= 2 and t[0] == key:
            return int(t[1], 0)
    return 0


def entry_walk(body, preload):
    """Scalar loads of kernel arguments (base s[0:1]) and effective lgkmcnt waits up to (a) and (b)."""
    ins = [ln.strip() for ln in body if ln.startswith("\t") and not ln.strip().startswith((";", "."))]
    if preload:      # skip the compatibility prologue: it ends with s_branch to the aligned preload entry
        k = next((j for j, t in enumerate(ins) if t.startswith("s_branch")), -1)
        ins = ins[k + 1:]
    def vload(t):
        return re.match(r"(global|buffer|flat)_load", t) is not None

    # (a) = the first vector load; (b) = the first non-temporal one, else the last load ahead of the first vmcnt wait
    first = next((j for j, t in enumerate(ins) if vload(t)), len(ins))
    nt = next((j for j, t in enumerate(ins) if vload(t) and re.search(r"\bnt\b", t)), None)
    if nt is None:
        wait = next((j for j in range(first, len(ins)) if ins[j].startswith("s_waitcnt") and "vmcnt" in ins[j]), len(ins))
        last = max((j for j in range(first, wait) if vload(ins[j])), default=first)
    else:
        last = nt
    ev_a, ev_b, pending = [], [], 0
    for j, t in enumerate(ins[:last]):
        op = t.split()[0]
        cur = ev_a if j < first else ev_b
        if op.startswith("s_load") and re.search(r"s\[0:1\]", t):
            cur.append(f"{op.replace('s_load_', 'load ')} @{t.split(',')[-1].strip()}")
            pending += 1
        elif op == "s_waitcnt" and "lgkmcnt(0)" in t and pending:
            cur.append(f"WAIT ({pending} outstanding)")
            pending = 0
    return ev_a, ev_b, nt is not None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(ROOT, "mlx-vlm_amd", "csrc"))
    ap.add_argument("--no-preload", action="store_true")
    ap.add_argument("--keep", default=None, help="keep the .s files in this directory")
    a = ap.parse_args()
    build = load_build(a.no_preload)
    hipcc, flags = build.HIPCC, build.flags_for("gemv_bf16.hip")      # (the three units share one set of flags)
    assert all(build.flags_for(t + ".hip") == flags for _, t, _ in KERNELS)
    out = a.keep or tempfile.mkdtemp(prefix="kernarg_entry_")
    os.makedirs(out, exist_ok=True)
    tus = sorted({k[1] for k in KERNELS})
    with ThreadPoolExecutor(max_workers=len(tus)) as ex:
        asm = dict(zip(tus, ex.map(lambda t: compile_asm(hipcc, flags, os.path.join(a.csrc, t + ".hip"),
                                                         os.path.join(out, t + ".s")), tus)))
    text = {t: open(p).read().split("\n") for t, p in asm.items()}
    print("flags: " + " ".join(f for f in flags if not f.startswith("-W")))
    bad = 0
    for label, tu, pat in KERNELS + ALTERNATES:
        counted = (label, tu, pat) in KERNELS
        sym, body, desc = function_text(text[tu], pat)
        if sym is None:
            print(f"{label}\n    NOT FOUND in {tu}.s")
            bad += counted
            continue
        preload = descriptor(desc, ".amdhsa_user_sgpr_kernarg_preload_length")
        vgpr, waves = descriptor(desc, "TotalNumVgprs"), descriptor(desc, "Occupancy")
        ev_a, ev_b, has_nt = entry_walk(body, preload)
        print(f"{label}\n    preload {preload:2d} dwords   {vgpr:3d} VGPRs   {waves} waves/SIMD")
        print("    (a) ahead of the first vector load:  " + (", ".join(ev_a) or "nothing"))
        print(f"    (b) then, ahead of the {'weight stream' if has_nt else 'last load of the first batch'}:  "
              + (", ".join(ev_b) or "nothing"))
        bad += counted and any(e.startswith("WAIT") for e in ev_a + ev_b)
    print(f"kernels with a kernel-argument wait ahead of their first loads: {bad} of {len(KERNELS)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
