"""FmlpEngine — flat-buffer training engine for the reference's FMLP (model/fmlp.py) on top of dr4sr_fmlp_* (C ABI)."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from .flat_engine import FlatEngine

_LAYER = [("filterlayer.complex_weight", lambda L, D, F: (1, L // 2 + 1, D, 2)),
          ("filterlayer.LayerNorm.weight", lambda L, D, F: (D,)), ("filterlayer.LayerNorm.bias", lambda L, D, F: (D,)),
          ("intermediate.dense_1.weight", lambda L, D, F: (F, D)), ("intermediate.dense_1.bias", lambda L, D, F: (F,)),
          ("intermediate.dense_2.weight", lambda L, D, F: (D, F)), ("intermediate.dense_2.bias", lambda L, D, F: (D,)),
          ("intermediate.LayerNorm.weight", lambda L, D, F: (D,)), ("intermediate.LayerNorm.bias", lambda L, D, F: (D,))]


def fmlp_param_names(n_layer):
    names = ["item_embedding.weight", "position_embeddings.weight", "LayerNorm.weight", "LayerNorm.bias"]
    for i in range(n_layer):
        names += [f"item_encoder.layer.{i}.{n}" for n, _ in _LAYER]
    return names


def fmlp_param_shapes(n_items, L, D, F, n_layer):
    shapes = [(n_items, D), (L, D), (D,), (D,)]
    for _ in range(n_layer):
        shapes += [fn(L, D, F) for _, fn in _LAYER]
    return shapes


class FmlpEngine(FlatEngine):
    MODEL, PLAN, PREFIX, ADAM_STEP = "FMLP", _lib.FmlpPlan, "dr4sr_fmlp_", "dr4sr_fmlp_adam_step"
    BUILT_FOR = "even L <= 50, D = 64, F = 256"

    def __init__(self, n_items, L=50, D=64, F=256, n_layer=2, ln_eps=1e-12, p_drop=0.5, max_batch=256, device="cuda",
                 seed=2023, lr=1e-3, betas=(0.9, 0.999), adam_eps=1e-8, weight_decay=0.0):
        self.n_items, self.L, self.D, self.F, self.n_layer = n_items, L, D, F, n_layer     # KEPT DIFFERENCE: no H
        self.ln_eps = float(ln_eps)
        # KEPT DIFFERENCE: one query per row, so one negative per row (neg_scratch has max_batch elements)
        super().__init__(fmlp_param_names(n_layer), fmlp_param_shapes(n_items, L, D, F, n_layer), (n_items, L, D, F, n_layer), 1,
                         p_drop, max_batch, device, seed, lr, betas, adam_eps, weight_decay)

    def _fill_shape(self, p):
        p.L, p.D, p.F, p.n_layer, p.n_items, p.ln_eps = self.L, self.D, self.F, self.n_layer, self.n_items, self.ln_eps

    def _shape_text(self):
        return f"FMLP shape L={self.L} D={self.D} F={self.F} layers={self.n_layer}"

    def _check_item_id(self, in_item_id, item_id):
        # KEPT DIFFERENCE: model/fmlp.py:38 keeps ONE query per row (transformer_out[:, -1]); against [B, L] targets the reference's
        # (query * item_embedding(target)).sum(-1) (basemodel.py:182) cannot broadcast
        if item_id.dim() != 1:
            raise _lib.Dr4srError(f"FMLP scores one query per row: item_id must be [rows], got {tuple(item_id.shape)} "
                                  "(use the prefix-row data format: data.prefix_rows / configs/synthetic-toys-prefix.yaml)")

    def make_plan(self, in_item_id, item_id, rows=None, neg_item=None, sample_neg=None, perm_sel=None, loss_log=None):
        return FlatEngine.make_plan(self, in_item_id, item_id, None, rows, neg_item, sample_neg, perm_sel, loss_log)     # KEPT DIFFERENCE: no seqlen

    # KEPT DIFFERENCE: the encoder output is the last position's, [B, D]: no pooling argument
    def encode(self, plan, training: bool, out: Optional[torch.Tensor] = None):
        if out is None:
            out = torch.empty(plan.B, self.D, dtype=torch.float32, device=self.device)
        self._call("dr4sr_fmlp_encode", plan, int(training), _lib.ptr(out))
        return out

    def encode_bwd(self, plan, training: bool, d_out: torch.Tensor):
        self._call("dr4sr_fmlp_encode_bwd", plan, int(training), _lib.ptr(d_out.contiguous()))
