"""Per-request samplers of the continuous batch, host side: the row-table lines the scheduler keeps (written at admission with
count 0 for the first token and 1 for the row's steps, moved with the row at compaction, zeroed when the row leaves), the
line a `Sampler` turns into, and the C ABI the mode is carried by - driven by the mock engine of
tests/test_batch_scheduler_cpu.py."""
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

from mlx_vlm_amd.sample_utils import make_sampler
from tests.test_batch_scheduler_cpu import MockEngineGenerator, make_pool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bf16_round(x: float) -> float:
    """double -> float32 -> bf16 (nearest even), as a float: the conversion csrc/sample.hip makes of a scalar call's 1 - top_p
    and log(min_p)"""
    u = struct.unpack("<I", struct.pack("<f", x))[0]
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return struct.unpack("<f", struct.pack("<I", u))[0]


def fields(line):
    line = np.asarray(line, dtype=np.int32)
    f = line.view(np.float32)
    return dict(temperature=float(f[0]), top_p=float(f[1]), min_p=float(f[2]), top_k=int(line[3]),
                seed=int(line.view(np.uint32)[4]), count=int(line.view(np.uint32)[5]), thr_top_p=float(f[6]), log_min_p=float(f[7]))


@pytest.mark.parametrize("kw", [dict(temp=0.7, top_p=0.9, min_p=0.05, top_k=40, seed=7), dict(temp=1.3, seed=0xFFFFFFFF),
                                dict(temp=0.5, top_p=0.37, seed=1), dict(temp=1.0, min_p=1e-3, top_k=3, seed=2),
                                dict(temp=1.0, top_p=1.0, seed=3), dict(temp=1.0, top_p=0.0, seed=4)])
def test_a_line_holds_engine_args_after_the_documented_roundings(kw):
    s = make_sampler(**kw)
    a = s.engine_args()
    got = fields(s.row_line(count=5))
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    assert got["temperature"] == f32(a["temperature"]) and got["top_p"] == f32(a["top_p"]) and got["min_p"] == f32(a["min_p"])
    assert got["top_k"] == a["top_k"] and got["seed"] == a["seed"] and got["count"] == 5
    assert got["thr_top_p"] == bf16_round(1.0 - a["top_p"])
    assert got["log_min_p"] == (bf16_round(math.log(a["min_p"])) if a["min_p"] else 0.0)
    # a filter that is off in engine_args is off in the line: top_p outside (0, 1), min_p 0, top_k 0
    assert (0 < got["top_p"] < 1) == (0 < s.top_p < 1)


def test_a_greedy_line_is_all_zero_and_extended_samplers_have_none():
    assert make_sampler().row_line().tolist() == [0] * 8
    assert make_sampler(min_p=0.1).row_line(3).tolist() == [0, 0, 0, 0, 0, 3, 0, 0]      # temp 0: greedy whatever else is set
    for kw in (dict(typical_p=0.5), dict(top_n_sigma=1.0), dict(p_less=True), dict(min_tokens_to_keep=2), dict(xtc_probability=0.5)):
        with pytest.raises(NotImplementedError):
            make_sampler(temp=1.0, **kw).row_line()


# ------------------------------------------------------------------------------------------ scheduler
def _ids(n, base=0):
    return [np.arange(3 + base + i, 3 + base + i + 4 + i) for i in range(n)]


def _lines(gen):
    return gen._sampler_lines().clone()


def _line_of(s, count):
    return s.row_line(count).tolist()


def test_lines_follow_the_rows():
    smps = [make_sampler(temp=0.5 + 0.1 * i, top_p=0.9, top_k=10 + i, seed=100 + i) for i in range(6)]
    default = make_sampler(temp=0.9, min_p=0.1, seed=9)
    gen = MockEngineGenerator(make_pool(), max_tokens=64, completion_batch_size=4, prefill_batch_size=4, async_prefill=False,
                              sampler=default)
    # 6 requests, 4 rows; request 2 takes the generator's sampler; different lengths: rows finish at different rounds
    max_tokens = [3, 9, 5, 7, 6, 4]
    given = smps[:2] + [None] + smps[3:]
    uids = gen.insert(_ids(6), max_tokens, samplers=given)
    by_uid = {u: (s or default) for u, s in zip(uids, given)}
    assert gen._row_sampling
    seen_compaction = False
    rounds = 0
    while gen.has_work:
        before = [row.uid for row in gen._rows]
        gen.next()
        rounds += 1
        assert rounds < 200
        after = [row.uid for row in gen._rows]
        lines = _lines(gen)
        # (the mock step does not advance the counts: a line holds what the scheduler wrote - count 1 at the join - wherever
        # its row has moved since)
        for r, u in enumerate(after):
            assert lines[r].tolist() == _line_of(by_uid[u], 1), (rounds, r, u)
        assert not lines[len(after):].any()             # rows past the live ones: zero = greedy
        kept = [u for u in before if u in after]
        if kept and [after.index(u) for u in kept] != [before.index(u) for u in kept]:
            seen_compaction = True
    assert seen_compaction
    assert not _lines(gen).any()
    gen.close()


def test_remove_zeroes_the_line_and_none_takes_the_generators():
    default = make_sampler(temp=0.7, top_k=5, seed=3)
    own = make_sampler(temp=1.1, top_p=0.8, seed=4)
    gen = MockEngineGenerator(make_pool(), max_tokens=50, completion_batch_size=4, prefill_batch_size=4, async_prefill=False,
                              sampler=default)
    u0, u1, u2 = gen.insert(_ids(3), 50, samplers=[None, own, None])
    gen.next()
    order = [row.uid for row in gen._rows]
    lines = _lines(gen)
    for r, u in enumerate(order):
        assert lines[r].tolist() == _line_of(own if u == u1 else default, 1)
    # the first row leaves: the last row takes its place with its line, the vacated line is zero
    assert gen.remove(order[0])
    lines = _lines(gen)
    assert [row.uid for row in gen._rows] == [order[2], order[1]]
    assert lines[0].tolist() == _line_of(own if order[2] == u1 else default, 1)
    assert lines[1].tolist() == _line_of(own if order[1] == u1 else default, 1)
    assert not lines[2:].any()
    gen.close()


def test_rows_already_running_get_the_generators_line_when_the_mode_begins():
    default = make_sampler(temp=0.6, seed=8)
    gen = MockEngineGenerator(make_pool(), max_tokens=50, completion_batch_size=4, prefill_batch_size=4, async_prefill=False,
                              sampler=default)
    gen.insert(_ids(2), 50)
    gen.next()
    assert not gen._row_sampling and getattr(gen, "_host_lines", None) is None      # a generator that never hears of samplers
    own = make_sampler(temp=1.0, top_k=2, seed=5)
    gen.insert(_ids(1, base=50), 50, samplers=[own])
    assert gen._row_sampling
    assert _lines(gen)[:2].tolist() == [_line_of(default, 0)] * 2
    gen.next()
    assert _lines(gen)[2].tolist() == _line_of(own, 1)
    gen.close()


def test_insert_checks_samplers():
    gen = MockEngineGenerator(make_pool(), max_tokens=8, completion_batch_size=2)
    with pytest.raises(ValueError, match="one entry per prompt"):
        gen.insert(_ids(2), 4, samplers=[make_sampler()])
    for bad in (make_sampler(temp=1.0, typical_p=0.4), make_sampler(temp=1.0, min_tokens_to_keep=3), lambda lp: lp.argmax(-1)):
        with pytest.raises(NotImplementedError, match="top_p, min_p .* top_k"):
            gen.insert(_ids(1), 4, samplers=[bad])
    assert not gen.unprocessed_prompts and not gen._row_sampling
    gen.close()
    eager = MockEngineGenerator(make_pool(), max_tokens=8, completion_batch_size=2, sampler=lambda lp: lp.argmax(-1))
    with pytest.raises(NotImplementedError):
        eager.insert(_ids(1), 4, samplers=[make_sampler(temp=1.0)])
    eager.insert(_ids(1), 4, samplers=[None])            # all None: nothing changes
    assert not eager._row_sampling
    eager.close()


# ------------------------------------------------------------------------------------------ header and ABI
def test_the_mode_rides_in_abi_v8():
    from mlx_vlm_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "vlm_hip.h")).read()
    assert len(set(re.findall(r"\b(vlm_[a-z0-9_]+)\s*\(", hdr))) == 60 == len(_lib.SIGNATURES)
    defs = dict(re.findall(r"#define (VLM_[A-Z_]+) (\(1 << \d+\)|\d+)", hdr))
    assert eval(defs["VLM_DECODE_ROW_SAMPLER"]) == _lib.DECODE_ROW_SAMPLER == 1 << 11
    assert int(defs["VLM_SAMPLE_ROW_TABLE"]) == _lib.SAMPLE_MODE_ROW_TABLE == 4
    assert int(defs["VLM_SAMPLE_ROW_STRIDE_WORDS"]) == _lib.SAMPLE_ROW_STRIDE_WORDS
    assert int(defs["VLM_SAMPLE_ROW_LINE_WORD"]) == _lib.SAMPLE_ROW_LINE_WORD
    # the line of every row lies inside the workspace as it was sized before the mode existed: 256 bytes + one block per row
    stride, word = _lib.SAMPLE_ROW_STRIDE_WORDS, _lib.SAMPLE_ROW_LINE_WORD
    assert 64 <= word and word + 8 <= 64 + stride and (4 * word) % 32 == 0 and (4 * stride) % 32 == 0
    # the documentation sits where a caller looks: at the parameter block and at the flag
    doc = hdr[hdr.index("VLM_SAMPLE_ROW_TABLE"):hdr.index("} vlm_sampler_params;")]
    for word_ in ("temperature f32", "count u32", "greedy", "(seed, count, 0, index)", "VLM_ERR_ARG"):
        assert word_ in doc.replace("GREEDY", "greedy"), word_
    flag = hdr[hdr.index("#define VLM_DECODE_ROW_SAMPLER"):]
    assert "VLM_DECODE_WINDOW" in flag[:1200] and "argument error" in flag[:1200]
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.lib()
        assert L.vlm_abi_version() == 8
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert len([ln for ln in out.splitlines() if " T vlm_" in ln]) == 60
        assert L.vlm_sample_workspace_bytes(3) == 256 + 3 * 4 * stride


def test_sample_row_table_is_a_view_of_the_workspace():
    from mlx_vlm_amd import _lib, ops

    ws = torch.zeros(256 + 3 * 4 * _lib.SAMPLE_ROW_STRIDE_WORDS, dtype=torch.uint8)
    lines = ops.sample_row_table(ws)
    assert tuple(lines.shape) == (3, 8)
    lines[2].copy_(torch.from_numpy(make_sampler(temp=1.0, seed=77).row_line(6)))
    words = ws.view(torch.int32)
    at = _lib.SAMPLE_ROW_LINE_WORD + 2 * _lib.SAMPLE_ROW_STRIDE_WORDS
    assert words[at + 4].item() == 77 and words[at + 5].item() == 6
    assert int((words != 0).sum()) == 4                  # temperature, top_p = 1 (off), seed, count (T(1 - 1.0) = 0, no min-p)
