"""FlatEngine — what the SASRec, FMLP and GRU4Rec engines (engine.py, fmlp_engine.py, gru_engine.py) have in common: the flat fp32
buffers (params / grads / Adam moments) and their named views, the workspace and the device state words, the ctypes plan of
include/dr4sr_hip.h filled field by field, and the entry points of the C ABI wrapped in _lib.check.  PyTorch supplies device memory
and the stream only; all arithmetic runs in libdr4sr_hip.so.

A subclass supplies MODEL, PLAN, PREFIX (its symbols are PREFIX + param_layout / workspace_bytes / fwd_bwd / train_step / encode /
encode_bwd, and ADAM_STEP), BUILT_FOR, its own constructor signature, `_fill_shape`, `_shape_text`, and overrides what really
differs; every such place is marked KEPT DIFFERENCE in the subclass.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import Dict, Optional

import torch

from . import _lib


class FlatEngine:
    MODEL = ""               # the model's name in error texts
    PLAN = None              # the ctypes mirror of the model's plan struct
    PREFIX = ""              # "dr4sr_<model>_"
    ADAM_STEP = ""           # the plan-taking optimizer entry
    BUILT_FOR = ""           # the shapes the library accepts, for the error of a refused one
    POOLED = ()              # poolings whose encode() output is [B, D] instead of [B, L, D]

    def __init__(self, names, shapes, layout_args, neg_per_row, p_drop, max_batch, device, seed, lr, betas, adam_eps, weight_decay):
        """names / shapes: the flat parameter layout; layout_args: what PREFIX + param_layout takes in front of the offsets;
        neg_per_row: negatives a row of the batch draws (the size of neg_scratch).  The subclass has set its shape attributes."""
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.Dr4srError(f"{type(self).__name__} needs a GPU device; dr4sr_amd has no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.p_drop, self.seed = float(p_drop), int(seed)
        self.lr, self.betas, self.adam_eps, self.weight_decay = lr, betas, adam_eps, weight_decay
        self.optimizer = _lib.OPT_ADAM             # DR4SR_OPT_* (set_optimizer)
        self.max_batch = max_batch
        off = (C.c_int64 * len(names))()
        self.n_params = int(getattr(self.lib, self.PREFIX + "param_layout")(*layout_args, off))
        self.offsets = list(off)
        dev = self.device
        self.params = torch.zeros(self.n_params, dtype=torch.float32, device=dev)
        self.grads = torch.zeros(self.n_params + _lib.GRAD_TAIL, dtype=torch.float32, device=dev)
        self.adam_m = torch.zeros(self.n_params, dtype=torch.float32, device=dev)
        self.adam_v = torch.zeros(self.n_params, dtype=torch.float32, device=dev)
        self.state = torch.zeros(_lib.STATE_WORDS, dtype=torch.int32, device=dev)
        self.names, self.shapes = names, shapes
        self.views: "OrderedDict[str, torch.Tensor]" = OrderedDict()
        self.grad_views: "OrderedDict[str, torch.Tensor]" = OrderedDict()
        for name, shp, o in zip(self.names, self.shapes, self.offsets):
            n = 1
            for s in shp:
                n *= s
            self.views[name] = self.params[o:o + n].view(shp)
            self.grad_views[name] = self.grads[o:o + n].view(shp)
        # what no plan of this engine changes (the ABI version, the shape fields, the flat buffers, slot 0's state words): filled once,
        # every plan starts as a copy of it
        c = self._const = self.PLAN()
        c.abi_version = _lib.ABI_VERSION
        self._fill_shape(c)
        c.params, c.grads = self.params.data_ptr(), self.grads.data_ptr()
        c.adam_m, c.adam_v, c.n_params = self.adam_m.data_ptr(), self.adam_v.data_ptr(), self.n_params
        c.state = self.state.data_ptr()
        sym = self.PREFIX + "workspace_bytes"
        probe = self._plan(max_batch, None, None, None, None, None, False, with_ws=False)
        self.ws_bytes = int(getattr(self.lib, sym)(C.byref(probe)))
        if self.ws_bytes <= 0:
            raise _lib.Dr4srError(f"{self._shape_text()}: {sym} failed: " + _lib._ERR.get(self.ws_bytes, str(self.ws_bytes))
                                  + " — built for " + self.BUILT_FOR)
        self.workspace = self._alloc_workspace()
        self.neg_scratch = torch.zeros(max_batch * neg_per_row, dtype=torch.int64, device=dev)
        self._keep = []          # tensors referenced by the last plan

    # ---- what a subclass supplies -------------------------------------------------------------------------------------------
    def _fill_shape(self, p):
        """copy the model's shape fields (and ln_eps where it has one) into the plan (called once, for the constant part)"""
        raise NotImplementedError

    def _shape_text(self) -> str:
        """the shape as the error of a refused one names it"""
        raise NotImplementedError

    def _alloc_workspace(self):
        return torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.device)

    def _check_item_id(self, in_item_id, item_id):
        # pooling 'origin' keeps one query per position: (query * item_embedding(target)).sum(-1) (basemodel.py:182) needs [rows, L] targets
        if item_id.shape != in_item_id.shape:
            raise _lib.Dr4srError(f"{self.MODEL} scores one query per position: item_id must be {tuple(in_item_id.shape)}, "
                                  f"got {tuple(item_id.shape)} (prefix-row data is the one-query-per-row models' format)")

    # ---- the plan -------------------------------------------------------------------------------------------------------------
    def _plan(self, B, in_item_id, item_id, seqlen, rows, neg_item, sample_neg, with_ws=True, perm_sel=None, loss_log=None):
        """with_ws=False: a probe plan (no workspace; with no tensors it references nothing)"""
        p = self.PLAN.from_buffer_copy(self._const)
        p.B, p.p_drop, p.seed = B, self.p_drop, self.seed
        for name, t in (("in_item_id", in_item_id), ("item_id", item_id), ("seqlen", seqlen), ("rows", rows), ("neg_item", neg_item)):
            if t is not None:
                assert t.dtype == torch.int64 and t.is_contiguous() and t.device == self.device, name
                setattr(p, name, t.data_ptr())
        p.sample_neg = 1 if sample_neg else 0
        if with_ws:
            p.workspace, p.workspace_bytes = self.workspace.data_ptr(), self.ws_bytes
        p.lr, (p.beta1, p.beta2), p.adam_eps, p.weight_decay = self.lr, self.betas, self.adam_eps, self.weight_decay
        p.optimizer = self.optimizer
        if perm_sel is not None:           # (perm[n], stride, offset, counter[1] int32): rows[] is FILLED by the step's first kernel
            perm, stride, offset, counter = perm_sel
            assert rows is not None and perm.dtype == torch.int64 and counter.dtype == torch.int32
            p.perm, p.n_perm, p.perm_stride, p.perm_offset = perm.data_ptr(), int(perm.shape[0]), int(stride), int(offset)
            p.perm_counter = counter.data_ptr()
        if loss_log is not None:           # float32 device buffer: the step's mean loss lands at [batch index] (include/dr4sr_hip.h)
            assert loss_log.dtype == torch.float32
            p.loss_log = loss_log.data_ptr()
        self._keep = [in_item_id, item_id, seqlen, rows, neg_item, perm_sel, loss_log]
        return p

    def make_plan(self, in_item_id, item_id, seqlen, rows=None, neg_item=None, sample_neg=None, perm_sel=None, loss_log=None):
        """rows=None: the tensors ARE the batch ([B,L]/[B]); else they are dataset tensors indexed by rows[B].
        perm_sel: fused device-side batch selection (include/dr4sr_hip.h: the plan's perm fields)."""
        B = int(rows.shape[0] if rows is not None else in_item_id.shape[0])
        if B > self.max_batch:
            raise _lib.Dr4srError(f"batch {B} > max_batch {self.max_batch}")
        if in_item_id.dim() != 2 or int(in_item_id.shape[1]) != self.L:
            raise _lib.Dr4srError(f"{self.MODEL}: in_item_id must be [rows, {self.L}], got {tuple(in_item_id.shape)}")
        if item_id is not None:
            self._check_item_id(in_item_id, item_id)
        if seqlen is not None and (seqlen.dim() != 1 or seqlen.shape[0] != in_item_id.shape[0]):
            raise _lib.Dr4srError(f"{self.MODEL}: seqlen must be [{int(in_item_id.shape[0])}], got {tuple(seqlen.shape)}")
        if sample_neg is None:
            sample_neg = neg_item is None
        if neg_item is None:
            neg_item = self.neg_scratch
        return self._plan(B, in_item_id, item_id, seqlen, rows, neg_item, sample_neg, perm_sel=perm_sel, loss_log=loss_log)

    # ---- entry points -----------------------------------------------------------------------------------------------------------
    def _call(self, symbol, plan, *args):
        """one plan-taking entry point on the current stream; a return code other than 0 raises a Dr4srError that names the symbol"""
        _lib.check(getattr(self.lib, symbol)(C.byref(plan), *args, _lib.cur_stream()), symbol)

    def fwd_bwd(self, plan):
        self._call(self.PREFIX + "fwd_bwd", plan)

    def train_step(self, plan):
        self._call(self.PREFIX + "train_step", plan)

    def _train_steps(self, plan, n: int):
        """n consecutive steps with one prep launch (the optimizer launches prepare the next step): needs a plan whose batch is selected
        on the device (perm_sel), else every step would train on the same rows.  Bound as `train_steps` by the engines whose library
        has the entry (the trainer asks hasattr)."""
        self._call(self.PREFIX + "train_steps", plan, int(n))

    def adam_step(self, plan=None):
        if plan is not None:               # the plan's optimizer launch: logs the step's loss when the plan carries a loss log
            self._call(self.ADAM_STEP, plan)
            return
        _lib.check(self.lib.dr4sr_optimizer_flat(self.optimizer, _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(self.adam_m),
                                                 _lib.ptr(self.adam_v), self.n_params, _lib.ptr(self.state), self.lr, self.betas[0],
                                                 self.betas[1], self.adam_eps, self.weight_decay, _lib.cur_stream()), "dr4sr_optimizer_flat")

    def encode(self, plan, training: bool, pooling: int, out: Optional[torch.Tensor] = None):
        if out is None:
            shape = (plan.B, self.D) if pooling in self.POOLED else (plan.B, self.L, self.D)
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        self._call(self.PREFIX + "encode", plan, int(training), pooling, _lib.ptr(out))
        return out

    def encode_bwd(self, plan, training: bool, pooling: int, d_out: torch.Tensor):
        self._call(self.PREFIX + "encode_bwd", plan, int(training), pooling, _lib.ptr(d_out.contiguous()))

    # ---- results ------------------------------------------------------------------------------------------------------------------
    def loss_and_count(self):
        """(mean loss, n_valid) of the last fwd_bwd — reads the gradient tail (one host sync)."""
        tail = self.grads[self.n_params:self.n_params + 2].tolist()
        n = tail[0]
        return (tail[1] / n if n > 0 else float("nan")), int(n)

    def normalized_grads(self) -> Dict[str, torch.Tensor]:
        n = self.grads[self.n_params]
        return {k: v / n for k, v in self.grad_views.items()}

    def load_named(self, sd: Dict[str, torch.Tensor]):
        for k, v in self.views.items():
            v.copy_(sd[k].to(self.device, torch.float32))

    def dropout_mask(self, n: int, site: int, step: int, p: Optional[float] = None) -> torch.Tensor:
        n4 = (n + 3) // 4 * 4
        out = torch.empty(n4, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.dr4sr_dropout_mask(_lib.ptr(out), n4, self.p_drop if p is None else p, self.seed, step, site,
                                               _lib.cur_stream()), "dr4sr_dropout_mask")
        return out[:n]
