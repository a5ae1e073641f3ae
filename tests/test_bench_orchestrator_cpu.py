"""bench.py's single-GPU orchestrator on the host (no GPU): a headline child that dies is re-run and reported, a dying extras child
costs only the extras it had not finished, and exactly ONE JSON line reaches stdout (BENCH_r04 was a GPU memory
fault that erased the whole line)."""
import argparse
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _args(**over):
    d = dict(gpus=1, steps=2, warmup=1, max_tokens=256, lookahead=8, vit_batch=64, no_cpu_baseline=True, no_cpu_hf=True, no_extras=False,
             no_configs=True, stage="")
    d.update(over)
    return argparse.Namespace(**d)


HEAD = {"metric": "decode tokens/sec + vision-prefill images/sec, Qwen2-VL-2B", "value": 1100.0, "unit": "tokens/s", "n_gpus": 1,
        "roofline": {"bound": "hbm", "frac": 0.43}, "_traffic_gate_up": 55e6, "decode_nan_rows": 0}
EXTRAS = {"kernels": {"gemv_gate_up_swiglu": {"GBps": 5200.0, "bytes_per_launch": 55050240, "us_per_launch": 10.5}},
          "vit336": (1240.0, 0.0516), "vit448": (210.0, 0.00476), "vit336_sweep": {"16": {"images_per_s": 1150.0}},
          "batch8": {"generation_tps": 5800.0}}


def test_headline_child_is_retried_and_one_line_is_printed(monkeypatch, capsys):
    import bench

    calls = []

    def fake_child(args, stage, timeout_s):
        calls.append(stage)
        if stage == "headline":
            if calls.count("headline") == 1:
                return None, -6, "Memory access fault by GPU node-2"
            return dict(HEAD), 0, ""
        return dict(EXTRAS), 0, ""

    monkeypatch.setattr(bench, "_child", fake_child)
    bench.orchestrate(_args())
    out, err = capsys.readouterr()
    lines = [ln for ln in out.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and calls == ["headline", "headline", "extras"]
    d = json.loads(lines[0])
    assert d["value"] == 1100.0 and "_traffic_gate_up" not in d
    assert d["headline_attempts"]["succeeded_on"] == 2 and d["headline_attempts"]["failed"][0]["rc"] == -6
    assert "Memory access fault" in d["headline_attempts"]["failed"][0]["stderr_tail"]
    assert d["roofline_kernel"]["traffic"] == 55e6 and d["roofline_vit"]["workload"].startswith("64 x 336x336")
    assert abs(d["roofline_vit"]["frac"] - 1240.0 * bench.VIT_TFLOP_336 / 2500.0) < 1e-12
    # the images/s half of the metric inside `roofline` (what the driver's record keeps whole), and a retry impossible to miss
    assert d["roofline"]["vit"]["batch"] == 64 and abs(d["roofline"]["vit"]["frac"] - d["roofline_vit"]["frac"]) < 1e-12
    assert d["roofline"]["vit_16"]["batch"] == 16 and abs(d["roofline"]["vit_16"]["images_per_s"] - 1150.0) < 1e-9
    assert d["roofline"]["vit_single_448"]["batch"] == 1 and d["roofline"]["vit_single_448"]["images_per_s"] == 210.0
    assert d["config"]["headline_retries"] == 1 and d["config"]["vit_batch"] == 64
    assert d["batch8_decode"] == {"generation_tps": 5800.0} and d["wide64_decode"] is None
    assert "[bench] headline: {" in err and "headline attempt 1 failed" in err


def test_extras_fault_keeps_the_headline_and_the_finished_extras(monkeypatch, capsys):
    import bench

    def fake_child(args, stage, timeout_s):
        if stage == "headline":
            return dict(HEAD), 0, ""
        return {"kernels": EXTRAS["kernels"]}, -6, "Memory access fault"         # died after the first extra

    monkeypatch.setattr(bench, "_child", fake_child)
    bench.orchestrate(_args())
    d = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert d["value"] == 1100.0 and "headline_attempts" not in d
    assert d["kernel_rooflines"] == EXTRAS["kernels"] and "roofline_vit" not in d and "extras stage rc -6" in d["extras_error"]


def test_three_dead_headline_children_end_the_run(monkeypatch):
    import bench

    monkeypatch.setattr(bench, "_child", lambda args, stage, timeout_s: (None, -11, "boom"))
    with pytest.raises(SystemExit) as e:
        bench.orchestrate(_args(no_extras=True))
    assert "failed 3 times" in str(e.value)


def test_clock_sampler_reads_the_starred_level_and_degrades_without_sysfs(tmp_path):
    """bench.ClockSampler: the current level of an amdgpu `pp_dpm_*` table is the line that ends with `*`; without the tables
    (this container) the summary says so instead of raising."""
    import time

    import bench

    sclk = tmp_path / "pp_dpm_sclk"
    sclk.write_text("S: 95Mhz\n0: 500Mhz\n1: 2100Mhz *\n2: 2400Mhz\n")
    mclk = tmp_path / "pp_dpm_mclk"
    mclk.write_text("0: 900Mhz\n1: 2000Mhz *\n")
    assert bench.ClockSampler._current_mhz(str(sclk)) == 2100
    c = bench.ClockSampler(period_s=0.01)
    c.paths = {"sclk": str(sclk), "mclk": str(mclk)}
    with c:
        time.sleep(0.05)
    s = c.summary()
    assert s["sclk_mhz"]["median"] == 2100 and s["mclk_mhz"]["max"] == 2000 and s["sclk_mhz"]["n"] >= 1
    d = bench.ClockSampler()
    d.paths = {}
    with d:
        pass
    assert "before" in d.summary() and "after" in d.summary()


def test_dump_outputs_and_steps_arguments(monkeypatch, tmp_path):
    """--dump-outputs reaches the headline child (an absolute path) and no other; --steps 0 and a dump of another workload
    are refused before anything runs."""
    import subprocess

    import bench

    cmds = []

    def fake_run(cmd, **kw):
        cmds.append(cmd)
        return subprocess.CompletedProcess(cmd, 0, stdout=json.dumps(HEAD) + "\n", stderr="")

    monkeypatch.setattr(subprocess, "run", fake_run)
    dump = str(tmp_path / "dump")
    bench._child(_args(dump_outputs=dump), "headline", 10)
    bench._child(_args(dump_outputs=dump), "extras", 10)
    assert cmds[0][cmds[0].index("--dump-outputs") + 1] == dump and "--dump-outputs" not in cmds[1]
    monkeypatch.undo()
    for extra in (["--steps", "0"], ["--dump-outputs", dump, "--workload", "nanollava"], ["--dump-outputs", dump, "--dry-run"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "error:" in r.stderr, (extra, r.stderr[-500:])
    assert not os.path.exists(dump)


def test_plain_run_times_the_headline_in_process_and_full_runs_the_orchestrator(monkeypatch, capsys):
    """`bench.py --gpus 1 --steps K --warmup W` runs the timed region in its own process and prints its line with nothing else
    started (no child, no extras, no CPU baseline, no other configs); `--full` hands the same arguments to the orchestrator,
    whose --no-* options still narrow it."""
    import bench

    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    seen = []

    def fake_headline(args, rank, ws, local):
        seen.append(("headline", args))
        return dict(HEAD)

    def refuse(*a, **kw):
        raise AssertionError("a plain run started more than its timed region")

    monkeypatch.setattr(bench, "stage_headline", fake_headline)
    monkeypatch.setattr(bench, "orchestrate", lambda args: seen.append(("orchestrate", args)))
    for name in ("_child", "stage_extras", "cpu_baseline", "other_configs"):
        monkeypatch.setattr(bench, name, refuse)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "2"])
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and [s[0] for s in seen] == ["headline"]
    d = json.loads(lines[0])
    assert d["value"] == 1100.0 and "_traffic_gate_up" not in d
    a = seen[0][1]
    assert (a.steps, a.warmup, a.max_tokens, a.full) == (4, 2, 256, False)
    assert a.no_extras and a.no_cpu_baseline and a.no_configs

    seen.clear()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "2", "--full", "--no-configs"])
    bench.main()
    assert [s[0] for s in seen] == ["orchestrate"] and capsys.readouterr().out == ""
    a = seen[0][1]
    assert (a.steps, a.warmup, a.max_tokens, a.full) == (4, 2, 256, True)
    assert not a.no_extras and not a.no_cpu_baseline and a.no_configs
