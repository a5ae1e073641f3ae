"""Shared model dataclasses - same fields and behaviour as the reference's
mlx_vlm/models/base.py:54-118 (LanguageModelOutput, InputEmbeddingsFeatures,
BaseModelConfig), holding torch device tensors instead of mx.arrays."""
from __future__ import annotations

import inspect
from dataclasses import dataclass
from typing import Any, Dict, List, Optional


@dataclass
class LanguageModelOutput:
    logits: Any
    hidden_states: Optional[List[Any]] = None
    cross_attention_states: Optional[List[Any]] = None
    encoder_outputs: Optional[List[Any]] = None
    gdn_states: Optional[List] = None
    shared_kv_states: Optional[Dict[str, tuple]] = None


@dataclass
class InputEmbeddingsFeatures:
    inputs_embeds: Any
    attention_mask_4d: Optional[Any] = None
    visual_pos_masks: Optional[Any] = None
    deepstack_visual_embeds: Optional[Any] = None
    per_layer_inputs: Optional[Any] = None
    cross_attention_states: Optional[Any] = None
    cross_attention_mask: Optional[Any] = None
    full_text_row_masked_out_mask: Optional[Any] = None
    decoder_inputs_embeds: Optional[Any] = None
    attention_mask: Optional[Any] = None
    position_ids: Optional[Any] = None
    pos_hw: Optional[Any] = None
    rope_deltas: Optional[Any] = None

    def to_dict(self):
        return {k: getattr(self, k) for k in self.__dataclass_fields__}


@dataclass
class BaseModelConfig:
    @classmethod
    def from_dict(cls, params):
        if not params:
            return cls()
        return cls(**{k: v for k, v in params.items() if k in inspect.signature(cls).parameters})

    def to_dict(self):
        return {k: v for k, v in self.__dict__.items() if v is not None}


def deepstack_window(visual_pos_masks, deepstack_visual_embeds, start: int, window: int):
    """DeepStack inputs of ONE prefill call over prompt columns [start, start + window) (reference qwen3_vl/language.py:528-558:
    the full-prompt mask and embeds are cut to the model's current window; the embeds of a layer are consumed in row order).
    visual_pos_masks: bool [B, L] (or [L]) over the full prompt; deepstack_visual_embeds: [n_layers, n_visual, D] (tensor or
    list of per-layer tensors).  -> (embeds [n_layers, n_window, D], rows int64 [n_window] into the call's B * window rows), or
    None when there is nothing to add.  A window that cuts the prompt is taken for one sequence, as the reference does."""
    import numpy as np

    if deepstack_visual_embeds is None or visual_pos_masks is None or len(deepstack_visual_embeds) == 0:
        return None
    m = visual_pos_masks.detach().cpu().numpy() if hasattr(visual_pos_masks, "detach") else np.asarray(visual_pos_masks)
    m = m.astype(bool).reshape(1, -1) if m.ndim == 1 else m.astype(bool)
    start, window = int(start), int(window)
    whole = start == 0 and window >= m.shape[1]
    if not whole and m.shape[0] != 1:
        raise NotImplementedError("DeepStack over a window of a batched prompt: one sequence per chunked prefill")
    n_before = int(m[:, :start].sum())
    win = m[:, start:start + window]
    rows = np.nonzero(win.reshape(-1))[0].astype(np.int64)
    if rows.size == 0:
        return None
    e = deepstack_visual_embeds
    if isinstance(e, (list, tuple)):
        import torch

        e = torch.stack(list(e))
    return e[:, n_before:n_before + rows.size], rows
