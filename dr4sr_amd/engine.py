"""SasrecEngine — the FlatEngine (flat_engine.py) of SASRec: dr4sr_sasrec_* of the C ABI (include/dr4sr_hip.h), plus what only
SASRec has: workspace slots, the expected_tokens regime hint and the data-parallel entry points.

Replaces, on the device: one iteration of BaseModel.training_epoch
(/root/reference model/basemodel.py:193-199) for model = SASRec (model/sasrec.py:39-75).
"""
from __future__ import annotations

import logging
import ctypes as C

import torch

from . import _lib
from .flat_engine import FlatEngine

_LAYER_TENSORS = [  # order of include/dr4sr_hip.h "Flat parameter layout"
    ("self_attn.in_proj_weight", lambda D, F: (3 * D, D)),
    ("self_attn.in_proj_bias", lambda D, F: (3 * D,)),
    ("self_attn.out_proj.weight", lambda D, F: (D, D)),
    ("self_attn.out_proj.bias", lambda D, F: (D,)),
    ("linear1.weight", lambda D, F: (F, D)),
    ("linear1.bias", lambda D, F: (F,)),
    ("linear2.weight", lambda D, F: (D, F)),
    ("linear2.bias", lambda D, F: (D,)),
    ("norm1.weight", lambda D, F: (D,)),
    ("norm1.bias", lambda D, F: (D,)),
    ("norm2.weight", lambda D, F: (D,)),
    ("norm2.bias", lambda D, F: (D,)),
]


def param_names(n_layer: int):
    names = ["item_embedding.weight", "query_encoder.position_emb.weight"]
    for i in range(n_layer):
        names += [f"query_encoder.transformer_layer.layers.{i}.{n}" for n, _ in _LAYER_TENSORS]
    return names


def param_shapes(n_items, L, D, F, n_layer):
    shapes = [(n_items, D), (L, D)]
    for _ in range(n_layer):
        shapes += [fn(D, F) for _, fn in _LAYER_TENSORS]
    return shapes


class SasrecEngine(FlatEngine):
    MODEL, PLAN, PREFIX, ADAM_STEP = "SASRec", _lib.SasrecPlan, "dr4sr_sasrec_", "dr4sr_adam_step"
    BUILT_FOR = "L <= 64, (D, F) in {(64, 128), (64, 256), (128, 128)}, head_dim 32 or 64"
    POOLED = (_lib.POOL_LAST, _lib.POOL_MEAN)
    train_steps = FlatEngine._train_steps

    def __init__(self, n_items: int, L: int, D: int, H: int, F: int, n_layer: int, ln_eps: float = 1e-12,
                 p_drop: float = 0.0, max_batch: int = 256, device="cuda", seed: int = 2023, lr: float = 1e-3,
                 betas=(0.9, 0.999), adam_eps: float = 1e-8, weight_decay: float = 0.0, n_slots: int = 1):
        self.n_items, self.L, self.D, self.H, self.F, self.n_layer = n_items, L, D, H, F, n_layer
        self.ln_eps = float(ln_eps)
        self.mean_len = None                     # mean valid length of the training split, set by the model (regime hint)
        self._mean_len = {}
        self._n_slots = n_slots
        super().__init__(param_names(n_layer), param_shapes(n_items, L, D, F, n_layer), (n_items, L, D, F, n_layer), L,
                         p_drop, max_batch, device, seed, lr, betas, adam_eps, weight_decay)

    def _fill_shape(self, p):
        p.L, p.D, p.H, p.F, p.n_layer, p.n_items, p.ln_eps = self.L, self.D, self.H, self.F, self.n_layer, self.n_items, self.ln_eps

    def _shape_text(self):
        return f"SASRec encoder shape L={self.L} D={self.D} H={self.H} F={self.F} layers={self.n_layer}"

    def _alloc_workspace(self):
        # KEPT DIFFERENCE: slot = (workspace, state words): several forward passes can be alive before their backward passes (CL4SRec
        # encodes three views per step); slot 0 is the default (`workspace`, `state`) and the one the optimizer's step counter lives in
        dev = self.device
        self.workspaces = [torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev) for _ in range(self._n_slots)]
        self.states = [self.state] + [torch.zeros(_lib.STATE_WORDS, dtype=torch.int32, device=dev) for _ in range(self._n_slots - 1)]
        return self.workspaces[0]

    # ------------------------------------------------------------------------------------------
    def _expected_tokens(self, B, seqlen, dataset_tensor: bool) -> int:
        """regime hint of the plan (include/dr4sr_hip.h: expected_tokens) = B * mean(min(seqlen, L)) when the caller gave none.
        Dataset tensors (batches are rows[] of them; they live as long as the dataset): one device reduction + host read per
        tensor, cached by (address, length, a checksum-free generation = the tensor's _version).  Per-batch tensors are transient —
        the allocator re-uses their memory for batches of other lengths, so they are NEVER cached: `self.mean_len` (the training
        split's mean, set by the model) when known, else measured (one synchronisation; not possible inside a graph capture, where
        the hint stays 0 = capacity rule and a warning says so once)."""
        if seqlen is None:
            return 0
        if dataset_tensor:
            key = (seqlen.data_ptr(), int(seqlen.shape[0]), int(seqlen._version))
            mean = self._mean_len.get(key)
            if mean is None:
                if torch.cuda.is_current_stream_capturing():
                    return 0
                mean = float(seqlen.clamp(0, self.L).float().mean()) if seqlen.numel() else 0.0
                if len(self._mean_len) > 64:
                    self._mean_len.clear()
                self._mean_len[key] = mean
        elif self.mean_len is not None:
            mean = self.mean_len
        elif torch.cuda.is_current_stream_capturing():
            if not getattr(self, "_warned_no_hint", False):
                self._warned_no_hint = True
                logging.getLogger("CDR").warning("dr4sr_amd: no expected_tokens hint for a per-batch plan inside a graph capture "
                                                 "(engine.mean_len unset): launch forms follow the capacity rule")
            return 0
        else:
            mean = float(seqlen.clamp(0, self.L).float().mean()) if seqlen.numel() else 0.0
        return max(1, int(B * mean))

    def make_plan(self, in_item_id, item_id, seqlen, rows=None, neg_item=None, sample_neg=None, perm_sel=None, slot=0, loss_log=None,
                  expected_tokens=None):
        """FlatEngine.make_plan, plus
        expected_tokens: the regime hint, when the caller knows the batch's valid-token count better than the engine's default
        (eval split, augmented views: CL4SRec's crops are much shorter than the training rows)."""
        p = FlatEngine.make_plan(self, in_item_id, item_id, seqlen, rows, neg_item, sample_neg, perm_sel, loss_log)
        if slot:   # KEPT DIFFERENCE: a later slot's workspace and state words, with a dropout stream of its own (slot 0 is what the base
            #        bound: `workspace`, `state`, the unshifted seed; a probe plan, which carries no workspace, never gets here)
            p.workspace, p.state = self.workspaces[slot].data_ptr(), self.states[slot].data_ptr()
            p.seed = (self.seed + 0x9E3779B97F4A7C15 * slot) & 0xFFFFFFFFFFFFFFFF
        # KEPT DIFFERENCE: only dr4sr_sasrec_plan has the hint
        p.expected_tokens = int(expected_tokens) if expected_tokens is not None else self._expected_tokens(p.B, seqlen, rows is not None)
        return p

    # ------------------------------------------------------------------------------------------
    # KEPT DIFFERENCE: only SASRec's encoder takes a per-token input scale (include/dr4sr_hip.h: dr4sr_sasrec_inputs)
    def _check_weight(self, plan, t, what):
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (plan.B, self.L) or t.device != self.params.device:
            raise _lib.Dr4srError(f"SASRec: {what} must be a contiguous fp32 [{plan.B}, {self.L}] tensor on {self.params.device}, got "
                                  f"{t.dtype} {tuple(t.shape)} on {t.device}")

    def encode(self, plan, training: bool, pooling: int, out=None, input_weight=None):
        """input_weight [B, L] (by batch slot): x = dropout(input_weight * (E[id] + P[pos])), sasrec.py:61-64; None = the unweighted call"""
        if input_weight is None:
            return FlatEngine.encode(self, plan, training, pooling, out)
        self._check_weight(plan, input_weight, "input_weight")
        if out is None:
            shape = (plan.B, self.D) if pooling in self.POOLED else (plan.B, self.L, self.D)
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        ins = _lib.SasrecInputs(_lib.ptr(input_weight), None)
        _lib.check(self.lib.dr4sr_sasrec_encode_w(C.byref(plan), C.byref(ins), int(training), pooling, _lib.ptr(out), _lib.cur_stream()),
                   "dr4sr_sasrec_encode_w")
        return out

    def encode_bwd(self, plan, training: bool, pooling: int, d_out: torch.Tensor, input_weight=None, d_input_weight=None):
        """input_weight: the forward's; d_input_weight [B, L]: receives the weight's gradient — written for pos < seqlen, so the caller
        hands a zero-filled buffer (the other positions' gradient is 0)"""
        if input_weight is None and d_input_weight is None:
            return FlatEngine.encode_bwd(self, plan, training, pooling, d_out)
        if input_weight is not None:
            self._check_weight(plan, input_weight, "input_weight")
        if d_input_weight is not None:
            self._check_weight(plan, d_input_weight, "d_input_weight")
        ins = _lib.SasrecInputs(_lib.ptr(input_weight) if input_weight is not None else None,
                                _lib.ptr(d_input_weight) if d_input_weight is not None else None)
        _lib.check(self.lib.dr4sr_sasrec_encode_w_bwd(C.byref(plan), C.byref(ins), int(training), pooling, _lib.ptr(d_out.contiguous()),
                                                      _lib.cur_stream()), "dr4sr_sasrec_encode_w_bwd")

    # ------------------------------------------------------------------------------------------
    # KEPT DIFFERENCE: the data-parallel step in pieces (parallel.py) exists for SASRec only
    def fwd_bwd_prepared(self, plan):
        self._call("dr4sr_sasrec_fwd_bwd_prepared", plan)

    def adam_step_prepare_next(self, plan):
        self._call("dr4sr_adam_step_prepare_next", plan)

    def grad_buckets(self, plan):
        """[(lo, hi), ...] float ranges of self.grads that become final one after the other in a step of this plan: one range
        (everything, tail included) in the latency forms, (item + position table | encoder layers + tail) at scale
        (include/dr4sr_hip.h: dr4sr_sasrec_grad_buckets)"""
        b = (C.c_int64 * 3)()
        n = int(self.lib.dr4sr_sasrec_grad_buckets(C.byref(plan), b))
        if n < 1:
            _lib.check(n, "dr4sr_sasrec_grad_buckets")
        return [(int(b[0]), int(b[1]))] if n == 1 else [(int(b[0]), int(b[1])), (int(b[1]), int(b[2]))]

    def grad_buckets_for(self, rows: int, seqlen=None):
        """grad_buckets of a training plan of `rows` rows drawn from the dataset tensor `seqlen` (a probe plan: no buffers)"""
        keep = self._keep
        probe = self._plan(rows, None, None, None, None, None, False, with_ws=False)
        self._keep = keep                                    # (the probe references nothing)
        probe.expected_tokens = self._expected_tokens(rows, seqlen, True) if seqlen is not None else \
            (max(1, int(rows * self.mean_len)) if self.mean_len is not None else 0)
        return self.grad_buckets(probe)

    def fwd_bwd_phase(self, plan, prepared: bool, phase: int):
        """phase 1: the step up to the launch that completes grad_buckets()[0]; phase 2: the rest (dr4sr_sasrec_fwd_bwd_phase)"""
        self._call("dr4sr_sasrec_fwd_bwd_phase", plan, int(bool(prepared)), int(phase))
