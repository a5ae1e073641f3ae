"""convert() on the host: the public surface, the C ABI it must not widen, the no-quantize path (MLX layout, shards, index,
config, sidecar files), the table of what gets quantized for the four families, every refusal, and the host-side bit
operations of models/quantized.py.  The quantizer kernel itself: tests/test_convert_gpu.py."""
from __future__ import annotations

import glob
import inspect
import json
import os
import re

import pytest
import torch

from oracle import idefics2 as oi
from oracle import llava_bunny as ob
from oracle import phi3_v as op3
from oracle import quant as Q
from oracle import qwen2_vl as oq
from tests.convert_helpers import assert_same_tensors, read_metadata, read_tensors, write_tiny_checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16

SIGNATURE = [("hf_path", inspect.Parameter.empty), ("mlx_path", "mlx_model"), ("quantize", False), ("q_group_size", 64),
             ("q_bits", 4), ("q_mode", "affine"), ("quant_method", "rtn"), ("calibration", "text"), ("calibration_data", None),
             ("dtype", None), ("upload_repo", None), ("revision", None), ("dequantize", False), ("trust_remote_code", True),
             ("quant_predicate", None), ("mtp", False), ("mtp_output", None)]


@pytest.fixture(scope="module")
def tiny_src(tmp_path_factory):
    """(cfg, W, directory): the tiny Qwen2-VL of the engine tests in the HF layout, written once and never changed"""
    cfg = oq.tiny_cfg()
    W = oq.random_weights(cfg, seed=4321, dtype=BF, std=0.05, embed_std=0.2)
    d = tmp_path_factory.mktemp("tiny_hf")
    write_tiny_checkpoint(str(d), cfg, W, tokenizer=False)
    (d / "tokenizer_config.json").write_text('{"tokenizer_class": "PreTrainedTokenizerFast"}')
    (d / "chat_template.jinja").write_text("{{ messages }}")
    (d / "modeling_remote.py").write_text("# remote code of the checkpoint\n")
    (d / "merges.txt").write_text("a b\n")
    (d / "extra").mkdir()
    (d / "extra" / "note.txt").write_text("kept")
    (d / "model.safetensors.index.json").write_text('{"metadata": {}, "weight_map": {"stale": "model.safetensors"}}')
    return cfg, W, str(d)


def test_convert_is_exported_with_the_reference_signature():
    from mlx_vlm_amd import convert

    sig = inspect.signature(convert)
    assert [(p.name, p.default) for p in sig.parameters.values()] == SIGNATURE
    import mlx_vlm_amd.convert as module          # the name is the module AND the function, in either import order
    from mlx_vlm_amd import convert as again

    assert callable(again) and [(p.name, p.default) for p in inspect.signature(again).parameters.values()] == SIGNATURE
    assert module.convert.__module__ == "mlx_vlm_amd.convert"


def test_c_abi_is_still_60_symbols_at_v8():
    hdr = open(os.path.join(ROOT, "include", "vlm_hip.h")).read()
    assert len(set(re.findall(r"\b(vlm_[a-z0-9_]+)\s*\(", hdr))) == 60
    assert "n_table_rows == -1" in hdr                       # the quantise direction is documented at its carrier
    srcs = "".join(open(f).read() for f in glob.glob(os.path.join(ROOT, "mlx-vlm_amd", "csrc", "*.hip")))
    m = re.search(r"int\s+vlm_abi_version\s*\(\s*(?:void)?\s*\)\s*\{\s*return\s+(\d+)\s*;", srcs)
    assert m and int(m.group(1)) == 8


def test_no_quantize_path_writes_mlx_layout_config_and_sidecars(tiny_src, tmp_path):
    from mlx_vlm_amd import convert

    cfg, W, src = tiny_src
    out = str(tmp_path / "mlx")
    convert(src, out)
    assert sorted(os.path.basename(f) for f in glob.glob(out + "/*.safetensors")) == ["model.safetensors"]
    assert read_metadata(out + "/model.safetensors") == {"format": "mlx"}
    assert_same_tensors(read_tensors(out), W)               # sanitized names, conv weight back in (O,T,H,W,C)
    raw = open(out + "/config.json").read()
    conf = json.loads(raw)
    assert list(conf) == sorted(conf) and raw == json.dumps(conf, indent=4)
    assert "torch_dtype" not in conf and "_name_or_path" not in conf and "quantization" not in conf
    src_conf = json.load(open(src + "/config.json"))
    assert conf == {k: v for k, v in src_conf.items() if k not in ("torch_dtype", "_name_or_path")}
    for name in ("tokenizer_config.json", "chat_template.jinja", "modeling_remote.py", "merges.txt", "preprocessor_config.json",
                 os.path.join("extra", "note.txt")):
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(src, name), "rb").read(), name
    index = json.load(open(out + "/model.safetensors.index.json"))
    assert "stale" not in index["weight_map"] and set(index["weight_map"].values()) == {"model.safetensors"}
    # an MLX-layout source passes through unchanged
    again = str(tmp_path / "mlx2")
    convert(out, again)
    assert_same_tensors(read_tensors(again), W)


def test_shards_index_and_total_size(tiny_src, tmp_path, monkeypatch):
    import mlx_vlm_amd.convert as C

    cfg, W, src = tiny_src
    limit = 96 * 1024
    monkeypatch.setattr(C, "_MAX_SHARD_BYTES", limit)
    out = str(tmp_path / "sharded")
    C.convert(src, out)
    files = sorted(os.path.basename(f) for f in glob.glob(out + "/*.safetensors"))
    n = len(files)
    assert n > 2 and files == [f"model-{i + 1:05d}-of-{n:05d}.safetensors" for i in range(n)]
    from safetensors.torch import load_file

    index = json.load(open(out + "/model.safetensors.index.json"))
    wm = index["weight_map"]
    assert list(wm) == sorted(wm) and set(wm) == set(W)
    assert index["metadata"]["total_size"] == sum(v.nbytes for v in W.values())
    order = []
    for f in files:
        shard = load_file(os.path.join(out, f))
        assert read_metadata(os.path.join(out, f)) == {"format": "mlx"}
        assert all(wm[k] == f for k in shard)
        size = sum(v.nbytes for v in shard.values())
        assert size <= limit or len(shard) == 1             # a tensor above the limit sits alone
        order.append(size)
    # greedy in insertion order: no two neighbouring shards would have fitted in one
    assert all(a + b > limit for a, b in zip(order, order[1:]))
    assert_same_tensors(read_tensors(out), W)
    # the rule itself: insertion order, a new shard when the next tensor would pass the limit
    t = {n: torch.zeros(s, dtype=torch.uint8) for n, s in (("a", 40), ("b", 50), ("c", 20), ("d", 200), ("e", 10), ("f", 90))}
    assert [list(s) for s in C.make_shards(t, 100)] == [["a", "b"], ["c"], ["d"], ["e", "f"]]


def _families():
    cq, cb, cp, ci = oq.tiny_cfg(), ob.tiny_cfg(), op3.tiny_cfg(), oi.tiny_cfg()
    return {"qwen2_vl": oq.random_weights(cq, seed=1, dtype=BF), "llava_bunny": ob.random_weights(cb, seed=1, dtype=BF),
            "phi3_v": op3.random_weights(cp, seed=1, dtype=BF), "idefics2": oi.random_weights(ci, seed=1, dtype=BF)}


def test_predicate_table_of_the_four_families():
    """The paths chosen = the 2-D `.weight`s with a last dimension % 64 == 0 under the prefixes the docstring of convert.py
    lists as quantized; nothing under a vision tower / vision_model, nothing whose last dimension is no multiple of 64."""
    import mlx_vlm_amd.convert as C

    for family, W in _families().items():
        W = dict(W)
        qp, bp = C.QUANTIZED_PREFIXES[family], C.BF16_PREFIXES[family]
        for p in qp + bp:
            assert p.rstrip(".") in C.__doc__, (family, p)
        odd = qp[0].rstrip(".") + "_odd"                    # under a quantized prefix, but 2-D with K % 64 != 0
        W[odd + ".weight"] = torch.zeros(8, 96, dtype=BF)
        chosen = C.quantized_paths(W)
        want = [k[:-len(".weight")] for k, v in W.items() if k.endswith(".weight") and v.dim() == 2 and v.shape[-1] % 64 == 0
                and k.startswith(qp)]
        assert chosen == want and len(chosen) > 4, (family, sorted(set(chosen) ^ set(want)))
        assert odd not in chosen
        assert not [p for p in chosen if "vision_tower" in p or "vision_model" in p or p.startswith(bp)]
        # every tensor is accounted for: quantized prefix, bf16 prefix, or no 2-D `.weight` at all
        for k, v in W.items():
            assert k.startswith(qp + bp) or not (k.endswith(".weight") and v.dim() == 2) or v.shape[-1] % 64, (family, k)
        tower = next(k for k in W if k.startswith(bp) and k.endswith(".weight") and W[k].dim() == 2)
        W2 = {**W, tower: torch.zeros(64, 128, dtype=BF)}      # a tower Linear of a width the rule would take elsewhere
        assert C.quantized_paths(W2) == want
        # the same choice as the oracle's quantize_checkpoint under this predicate
        ck, _ = Q.quantize_checkpoint(W, predicate=lambda p, v: not C.skip_multimodal_module(p))
        assert chosen == [k[:-len(".scales")] for k in ck if k.endswith(".scales")]
        # a callable predicate narrows the rule, a dict answer is refused
        assert C.quantized_paths(W, lambda p, t: "embed_tokens" not in p) == [p for p in want if "embed_tokens" not in p]
        with pytest.raises(NotImplementedError):
            C.quantized_paths(W, lambda p, t: {"bits": 8, "group_size": 64})


REFUSALS = [
    (dict(q_bits=8), NotImplementedError), (dict(q_bits=3, quantize=True), NotImplementedError),
    (dict(q_group_size=32), NotImplementedError), (dict(q_group_size=128, quantize=True), NotImplementedError),
    (dict(q_mode="mxfp4"), NotImplementedError), (dict(quant_method="awq", quantize=True), NotImplementedError),
    (dict(quant_predicate="mixed_3_6", quantize=True), NotImplementedError), (dict(mtp=True), NotImplementedError),
    (dict(upload_repo="someone/model"), NotImplementedError),
    (dict(quantize=True, quant_predicate=lambda p, t: {"bits": 4, "group_size": 64}), NotImplementedError),
    (dict(quantize=True, dtype="float16"), NotImplementedError), (dict(quantize=True, dtype="float32"), NotImplementedError),
    (dict(quantize=True, dequantize=True), ValueError),
]


@pytest.mark.parametrize("kw,exc", REFUSALS, ids=[",".join(k) for k, _ in REFUSALS])
def test_refusals_raise_before_anything_is_written(tiny_src, tmp_path, kw, exc):
    from mlx_vlm_amd import convert

    out = str(tmp_path / "never")
    with pytest.raises(exc):
        convert(tiny_src[2], out, **kw)
    assert not os.path.exists(out)


def test_refusals_that_depend_on_the_source(tiny_src, tmp_path):
    from mlx_vlm_amd import convert

    cfg, W, src = tiny_src
    out = str(tmp_path / "never")
    # a family outside the four
    other = tmp_path / "other"
    write_tiny_checkpoint(str(other), cfg, W, tokenizer=False, config_extra={"model_type": "paligemma"})
    with pytest.raises(NotImplementedError):
        convert(str(other), out)
    # quantize=True on a source that already holds .scales
    ck, _ = Q.quantize_checkpoint(W, predicate=lambda p, v: p.startswith("language_model."))
    quant = tmp_path / "quant"
    write_tiny_checkpoint(str(quant), cfg, ck, hf_layout=False, tokenizer=False,
                          config_extra={"quantization": {"group_size": 64, "bits": 4}})
    with pytest.raises(ValueError):
        convert(str(quant), out, quantize=True)
    # a source in another mode than the loader runs
    quant8 = tmp_path / "quant8"
    write_tiny_checkpoint(str(quant8), cfg, ck, hf_layout=False, tokenizer=False,
                          config_extra={"quantization": {"group_size": 32, "bits": 8}})
    with pytest.raises(NotImplementedError):
        convert(str(quant8), out)
    # no dtype anywhere and fp32 weights: the kernel reads bf16, the caller is told to pass dtype="bfloat16"
    f32 = tmp_path / "f32"
    write_tiny_checkpoint(str(f32), cfg, {k: v.float() for k, v in W.items()}, tokenizer=False)
    conf = json.load(open(f32 / "config.json"))
    del conf["torch_dtype"]
    (f32 / "config.json").write_text(json.dumps(conf))
    with pytest.raises(NotImplementedError, match="bfloat16"):
        convert(str(f32), out, quantize=True)
    with pytest.raises(FileNotFoundError):
        convert(str(tmp_path / "missing"), out)
    assert not os.path.exists(out)
    # ... while the dtype cast alone runs on the host: fp32 source -> bf16 output, bit-identical to the bf16 weights
    convert(str(f32), out, dtype="bfloat16")
    assert_same_tensors(read_tensors(out), W)
    # a quantized MLX-layout source passes through (nothing to dequantize on the host, nothing asked for)
    again = str(tmp_path / "pass")
    convert(str(quant), again)
    assert_same_tensors(read_tensors(again), ck)
    assert json.load(open(again + "/config.json"))["quantization"] == {"group_size": 64, "bits": 4}


def test_cli_parser_has_the_reference_flag_names():
    import mlx_vlm_amd.convert as C

    a = C.configure_parser().parse_args(["--hf-path", "a", "--mlx-path", "b", "-q", "--q-group-size", "64", "--q-bits", "4",
                                         "--q-mode", "affine", "--dtype", "bfloat16"])
    assert vars(a) == dict(hf_path="a", mlx_path="b", quantize=True, q_group_size=64, q_bits=4, q_mode="affine",
                           dtype="bfloat16", dequantize=False)
    d = C.configure_parser().parse_args(["--hf-path", "a", "-d"])
    assert d.dequantize and not d.quantize and d.mlx_path == "mlx_model" and d.q_bits is None and d.q_group_size is None
    assert set(vars(a)) <= {n for n, _ in SIGNATURE}


def test_split_sb_inverts_take():
    from mlx_vlm_amd.models import quantized as Qz

    g = torch.Generator().manual_seed(5)
    w = (torch.randn(37, 256, generator=g) * 0.3).to(BF)
    wq, s, b = Q.quantize_affine(w, 64, 4)
    s[0, 0], b[0, 1] = -0.0, float("inf")                    # bit patterns, not values: sign of zero and the top exponent survive
    q = Qz.take({"p.weight": wq, "p.scales": s, "p.biases": b}, "p")
    s2, b2 = Qz.split_sb(q)
    assert s2.dtype == BF and b2.dtype == BF and s2.shape == (37, 4)
    assert torch.equal(s2.view(torch.int16), s.view(torch.int16)) and torch.equal(b2.view(torch.int16), b.view(torch.int16))
    back = Qz.take({"p.weight": q.wq, "p.scales": s2, "p.biases": b2}, "p")
    assert torch.equal(back.sb, q.sb) and torch.equal(back.wq, wq)


def test_quantize_w4_has_no_cpu_fallback():
    from mlx_vlm_amd import _lib, ops

    with pytest.raises(_lib.VlmHipError):
        ops.quantize_w4(torch.zeros(4, 64, dtype=BF))
