"""Qwen3-VL language model on MI355X - host mirror of the reference's mlx_vlm/models/qwen3_vl/language.py (LanguageModel: same
call contract, get_rope_index, rope-delta position rule, DeepStack inputs) on the native engine of models/qwen2_vl.

What the reference's file changes against its qwen2_vl/language.py, and where it lands here:
  * q / k / v / o without bias, an explicit head_dim (40-57)            -> QKV_BIAS, TextConfig.head_dim
  * q_norm / k_norm = RMSNorm(head_dim) per head before the rope (84-89) -> the engine's VLM_MODE_QWEN3: the qkv step is the
    projection and then the QK-norm form of the rotary + KV-write launch (csrc/rope.hip), in the prefill and in every decode step
  * the interleaved M-RoPE selector (19-37, rope_utils.py:511-516)       -> the same mode
  * DeepStack (231-283, 528-558): the rows at image-token positions get the tower's tap features added behind the first
    decoder layers, prefill only, cut to the window of a chunked prefill  -> vlm_prefill_args.ds_* / ops.add_rows_
  * get_rope_index (299-485) gives the positions of qwen2_vl's for text and images (video is out of scope here as there)
"""
from __future__ import annotations

import torch

from ... import _lib, ops
from ..._lib import check
from ..qwen2_vl.language import DecodeState, LanguageModel as _Qwen2VLLanguageModel, _to_np
from .config import ModelConfig, TextConfig


class LanguageModel(_Qwen2VLLanguageModel):
    DEEPSTACK = True

    def __init__(self, args: TextConfig, config: ModelConfig, device="cuda", **engine_kwargs):
        super().__init__(args, config, device=device, **engine_kwargs)
        self.mrope_section = list((args.rope_scaling or {}).get("mrope_section", [24, 20, 20]))
        self.QKV_BIAS = bool(getattr(args, "attention_bias", False))
        if self.head_dim != 128:
            raise NotImplementedError(f"head_dim = {self.head_dim}: the QK-norm rotary kernel and the decode attention are built "
                                      "for 128-wide heads (every dense Qwen3-VL)")
        if len(self.mrope_section) != 3 or sum(self.mrope_section) != self.head_dim // 2 or self.mrope_section[0] <= 0:
            raise ValueError(f"mrope_section {self.mrope_section} must have three entries that sum to head_dim / 2")
        if not getattr(args, "use_final_norm", True):
            raise NotImplementedError("use_final_norm = False is not built")
        self._qkn_tables = {}

    def _set_engine_modes(self):
        check(_lib.lib().vlm_llm_set_tuning(self._handle, _lib.MODE_QWEN3, 1), "llm_set_tuning")

    def _layer_extra(self, i, prefix, W):
        """q_norm / k_norm as the engine reads them: fp32 [head_dim] (the bf16 weights widened)"""
        qn = self.arena.put(W[prefix + "self_attn.q_norm.weight"].to(device=self.device, dtype=torch.bfloat16).float())
        kn = self.arena.put(W[prefix + "self_attn.k_norm.weight"].to(device=self.device, dtype=torch.bfloat16).float())
        self._w[f"{i}.qn"], self._w[f"{i}.kn"] = qn, kn
        return qn.data_ptr(), kn.data_ptr()

    def _rope_kvwrite(self, i, qkv, pos_d, inv_tab, new_seq_d, new_slot_d, bt, kp, vp):
        t = self.args
        tab = self._qkn_tables.get(i)
        if tab is None:
            tab = self._qkn_tables[i] = ops.qknorm_table(inv_tab, t.rms_norm_eps, self._w[f"{i}.qn"], self._w[f"{i}.kn"])
        ops.mrope_qknorm_kvwrite_(qkv, t.num_attention_heads, t.num_key_value_heads, self.head_dim, pos_d[0], pos_d[1], pos_d[2],
                                  tab, self.mrope_section, kv_seq=new_seq_d, kv_slot=new_slot_d, block_table=bt, kpool=kp, vpool=vp)

    def get_rope_index(self, input_ids, image_grid_thw=None, video_grid_thw=None, attention_mask=None):
        """reference language.py:299-485.  For text and images its rules give qwen2_vl's positions (pinned by
        tests/golden/qwen3_vl_tiny_ref.npz); video grids are refused instead of silently taking that rule."""
        if video_grid_thw is not None:
            raise NotImplementedError("video inputs are outside the built hot path")
        return super().get_rope_index(input_ids, image_grid_thw, None, attention_mask)


__all__ = ["DecodeState", "LanguageModel", "_to_np"]
