"""Dataset regeneration — stage 3 of DR4SR (the reference's 3.Hybrid_inference.py) on the GPU.

The pre-trained regenerator (the reference's `Generator`: nn.Transformer d 64, 2 heads, 2 + 2 post-norm layers, FFN 256, erf-GELU,
plus `condition_linear` that turns the encoder memory into K condition memories) greedy-decodes every training sequence under each
condition; the decoded sequences, deduplicated, become new training rows of `train_regen.pth` — what `train_file: '_regen'` reads.

    model = RegenModel.from_state_dict(torch.load("regenerator.pth"), "cuda")
    model.translate([src0, src1, ...], condition=2)            # what the reference's translate() returns, one tensor per source
    hybrid_inference("dataset/amazon-toys/toy/")               # writes train_regen.pth exactly as the reference does

backend="hip" runs csrc/regen.hip through the C ABI (dr4sr_regen_encode / dr4sr_regen_decode: all steps of a chunk of rows on the
device, no host sync per token).  backend="torch" is a batched eager restatement of the same math (padding masks, full prefix
recompute); it runs on CPU or GPU and is the cross-check of the kernels, not a fall-back: nothing switches to it on its own.
It lives in regen_torch.py; this module holds the product path: parameters and the two flat buffers, plans, packing, the HIP calls
and the chunk drivers.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os

import torch

from . import _lib
from .regen_dropout import RegenDropout, eval_mode      # RegenDropout: callers import it from here

D, H, FF, N_LAYER, N_POS, MAX_LEN, LN_EPS = 64, 2, 256, 2, 50, 25, 1e-12
NUM_ITEM = {"toy": 11925, "sport": 18358, "beauty": 12102, "yelp": 20034}     # 3.Hybrid_inference.py:237-242
ROWS_PER_CALL = 16384          # decode rows per HIP call: ~1.3 GB of workspace (csrc/regen.hip, about 77 KB per row)
ROWS_PER_TORCH = 2048          # decode rows per torch batch ([rows, n_rows] logits)
PAIRS_PER_CALL = 4096          # score(): pairs per HIP call (csrc/regen_score.hip keeps K x 2 x Ls x 128 floats per pair: 256 KB at Ls = 50)
SCORE_BWD_PAIRS_PER_CALL = 256 # loss_and_grad(): pairs per HIP call (the backward keeps ~2 MB of records per pair at Ls = 50: ~0.6 GB)
COND_BWD_PAIRS_PER_CALL = 1024 # condition_grad(): pairs per HIP call (csrc/regen_score_bwd.hip keeps ~16 KB per token slot: ~0.5 GB at T = 19)
MAX_SEQ_LEN = 50

_ENC = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
        "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")
_DEC = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
        "multihead_attn.in_proj_weight", "multihead_attn.in_proj_bias", "multihead_attn.out_proj.weight", "multihead_attn.out_proj.bias",
        "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias",
        "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias", "norm3.weight", "norm3.bias")


def param_names():
    """state-dict names in the order of the flat layout (include/dr4sr_hip.h, dr4sr_regen_param_layout)"""
    names = ["item_embedding.weight", "position_embedding.weight"]
    names += [f"transformer.encoder.layers.{i}.{n}" for i in range(N_LAYER) for n in _ENC]
    names += ["transformer.encoder.norm.weight", "transformer.encoder.norm.bias"]
    names += [f"transformer.decoder.layers.{i}.{n}" for i in range(N_LAYER) for n in _DEC]
    names += ["transformer.decoder.norm.weight", "transformer.decoder.norm.bias"]
    names += ["condition_linear.0.weight", "condition_linear.0.bias", "condition_linear.2.weight", "condition_linear.2.bias"]
    return names


def score_param_names():
    """the 98 tensors of dr4sr_regen_score_param_layout: param_names() followed by condition_encoder.*"""
    names = param_names()
    names += [f"condition_encoder.encoder.layers.{i}.{n}" for i in range(N_LAYER) for n in _ENC]
    names += [f"condition_encoder.condition_layer.{i}.{n}" for i in (0, 2) for n in ("weight", "bias")]
    return names


_ENC_SHAPES = [(3 * D, D), (3 * D,), (D, D), (D,), (FF, D), (FF,), (D, FF), (D,), (D,), (D,), (D,), (D,)]      # the shapes of _ENC


def score_param_shapes(n_rows: int, K: int):
    return param_shapes(n_rows, K) + _ENC_SHAPES * N_LAYER + [(D, D), (D,), (K, D), (K,)]


def param_shapes(n_rows: int, K: int):
    dec = [(3 * D, D), (3 * D,), (D, D), (D,), (3 * D, D), (3 * D,), (D, D), (D,), (FF, D), (FF,), (D, FF), (D,)] + [(D,)] * 6
    return ([(n_rows, D), (N_POS, D)] + _ENC_SHAPES * N_LAYER + [(D,), (D,)] + dec * N_LAYER + [(D,), (D,)]
            + [(K * D, D), (K * D,), (K * D, K * D), (K * D,)])


def _chunks(n: int, size: int):
    """(a, b) of the chunks [a, b) of at most `size` rows that cover range(n); none for n = 0"""
    return ((a, min(n, a + size)) for a in range(0, n, size))


def _check_backend(backend):
    if backend not in ("hip", "torch"):
        raise ValueError(f"backend must be 'hip' or 'torch', not {backend!r}")


def _torch():
    """the eager restatement, for the backend="torch" branches (regen_torch.py imports this module, so it is imported at first use)"""
    from . import regen_torch
    return regen_torch


class RegenModel:
    """the reference's Generator at inference (eval mode: dropout off), from its state dict"""

    def __init__(self, params: dict, n_rows: int, K: int, device):
        self.device = torch.device(device)
        self.n_rows, self.K = int(n_rows), int(K)
        self.n_item = self.n_rows - 2
        self.sos, self.eos = self.n_item, self.n_item + 1
        self.p = {k: v.to(self.device, torch.float32).contiguous() for k, v in params.items()}
        self._flat = None
        self._score_flat = None
        self._layouts = {}
        self._cast = {}
        self.has_condition_encoder = "condition_encoder.condition_layer.2.weight" in self.p

    @classmethod
    def from_state_dict(cls, sd: dict, device="cuda", dataset: str | None = None):
        """`sd`: the reference's regenerator.pth as saved (2.Pretrain_regenerator.py:318).  condition_encoder.* is kept when it is
        complete (score() uses it; decoding never does) and dropped otherwise; item_embedding_decoder.weight must be the same table as item_embedding.weight (the reference ties
        them).  N and K come from the tensors; with a known `dataset` name N is checked against the reference's num_item_dict."""
        if "item_embedding.weight" not in sd or "condition_linear.2.weight" not in sd:
            raise ValueError("not a regenerator state dict: item_embedding.weight / condition_linear.2.weight missing")
        E = sd["item_embedding.weight"]
        dec = sd.get("item_embedding_decoder.weight")
        if dec is not None and not torch.equal(dec.cpu(), E.cpu()):
            raise ValueError("item_embedding_decoder.weight differs from item_embedding.weight (the reference ties them)")
        n_rows = int(E.shape[0])
        KD = int(sd["condition_linear.2.weight"].shape[0])
        if KD % D or int(sd["condition_linear.2.weight"].shape[1]) != KD:
            raise ValueError(f"condition_linear.2.weight has shape {tuple(sd['condition_linear.2.weight'].shape)}, expected [64K, 64K]")
        K = KD // D
        if dataset is not None and dataset in NUM_ITEM and NUM_ITEM[dataset] + 2 != n_rows:
            raise ValueError(f"item table has {n_rows} rows; dataset '{dataset}' has {NUM_ITEM[dataset]} items (+ SOS, EOS)")
        params = {}
        for name, shape in zip(param_names(), param_shapes(n_rows, K)):
            if name not in sd:
                raise ValueError(f"state dict lacks {name}")
            if tuple(sd[name].shape) != shape:
                raise ValueError(f"{name}: shape {tuple(sd[name].shape)}, expected {shape}")
            params[name] = sd[name].detach()
        extra = list(zip(score_param_names(), score_param_shapes(n_rows, K)))[len(params):]
        if all(name in sd and tuple(sd[name].shape) == shape for name, shape in extra):     # a complete condition_encoder: kept for score()
            params.update({name: sd[name].detach() for name, _ in extra})
        return cls(params, n_rows, K, device)

    # ------------------------------------------------------------------------------------------------ HIP
    def _layout(self, score: bool):
        """(element count, offsets, names) of dr4sr_regen_param_layout's 70 tensors or, score=True, of the 98 tensors of
        dr4sr_regen_score_param_layout; asked of the library once"""
        if score not in self._layouts:
            fn, names = ("dr4sr_regen_score_param_layout", score_param_names()) if score else ("dr4sr_regen_param_layout", param_names())
            off = (C.c_int64 * len(names))()
            n = getattr(_lib.load(), fn)(self.n_rows, self.K, off)
            if n < 0:
                _lib.check(int(n), fn)
            self._layouts[score] = int(n), list(off), names
        return self._layouts[score]

    def _fill_flat(self, buf, score: bool, only=None):
        """write the named parameters (`only`: those names) into a flat buffer of the 70- or the 98-tensor layout"""
        _, off, names = self._layout(score)
        for o, name in zip(off, names):
            if (only is None or name in only) and (name in self.p or not score):      # only the score layout's condition_encoder.* may be absent
                buf[o:o + self.p[name].numel()] = self.p[name].reshape(-1)
        return buf

    def flat(self):
        """the flat fp32 parameter buffer of dr4sr_regen_param_layout"""
        if self._flat is None:
            self._flat = self._fill_flat(torch.zeros(self._layout(False)[0], dtype=torch.float32, device=self.device), False)
        return self._flat

    def score_flat(self):
        """the flat fp32 parameter buffer of dr4sr_regen_score_param_layout (condition_encoder.* zero when the model has none)"""
        if self._score_flat is None:
            self._score_flat = self._fill_flat(torch.zeros(self._layout(True)[0], dtype=torch.float32, device=self.device), True)
        return self._score_flat

    def adopt_score_flat(self, buf):
        """make `buf` the model's score buffer (a trainer's padded master holds it as a view): score_plan() points at it from now on.
        Its contents are the caller's business; it must be a contiguous fp32 tensor of score_flat()'s length on the model's device"""
        n = self._layout(True)[0]
        same_device = buf.device.type == self.device.type and self.device.index in (None, buf.device.index)
        if buf.numel() != n or buf.dim() != 1 or buf.dtype != torch.float32 or not same_device or not buf.is_contiguous():
            raise ValueError(f"the score buffer must hold {n} contiguous fp32 values on {self.device}")
        self._score_flat = buf

    def score_plan(self):
        return self.plan(self.score_flat())

    def plan(self, flat=None):
        """the plan over flat(), or over the given parameter buffer (score_plan: the 98-tensor one)"""
        p = _lib.RegenPlan()
        p.abi_version = _lib.ABI_VERSION
        p.n_rows, p.K, p.max_len = self.n_rows, self.K, MAX_LEN
        p.D, p.H, p.F, p.n_layer = D, H, FF, N_LAYER
        p.ln_eps = LN_EPS
        flat = self.flat() if flat is None else flat
        p.params = flat.data_ptr()
        p.n_params = flat.numel()
        return p

    def _pack(self, src_list):
        lens = [int(len(s)) for s in src_list]
        if any(n > N_POS for n in lens):
            raise ValueError(f"a source of {max(lens)} ids: the regenerator's position table has {N_POS} rows (the reference fails "
                             f"for len(src) > {N_POS})")
        if any(n < 1 for n in lens):
            raise ValueError("an empty source")
        Ls = max(lens)
        src = torch.full((len(src_list), Ls), self.sos, dtype=torch.int64)
        for i, s in enumerate(src_list):
            src[i, :lens[i]] = torch.as_tensor(s, dtype=torch.int64).reshape(-1).cpu()
        if int(src.min()) < 0 or int(src.max()) >= self.n_rows:
            raise IndexError(f"source ids outside [0, {self.n_rows})")
        return src, torch.tensor(lens, dtype=torch.int64)

    def _decode_hip(self, src, lens, cond0, n_cond):
        """tokens [n_cond * S, MAX_LEN] int64 and len [n_cond * S] int32 (condition-major), on the host"""
        lib = _lib.load()
        plan = self.plan()
        S = src.shape[0]
        src_d, len_d = src.to(self.device).contiguous(), lens.to(self.device).contiguous()
        nb = lib.dr4sr_regen_workspace_bytes(C.byref(plan), S, n_cond)
        if nb < 0:
            _lib.check(int(nb), "dr4sr_regen_workspace_bytes")
        ws = torch.empty(int(nb), dtype=torch.uint8, device=self.device)
        tok = torch.empty(n_cond * S, MAX_LEN, dtype=torch.int64, device=self.device)
        ln = torch.empty(n_cond * S, dtype=torch.int32, device=self.device)
        st = _lib.cur_stream()
        _lib.check(lib.dr4sr_regen_encode(C.byref(plan), _lib.ptr(src_d), _lib.ptr(len_d), S, src.shape[1], cond0, n_cond,
                                          C.c_void_p(ws.data_ptr()), int(nb), st), "dr4sr_regen_encode")
        _lib.check(lib.dr4sr_regen_decode(C.byref(plan), _lib.ptr(src_d), _lib.ptr(len_d), S, src.shape[1], cond0, n_cond,
                                          C.c_void_p(ws.data_ptr()), int(nb), _lib.ptr(tok), _lib.ptr(ln), st), "dr4sr_regen_decode")
        return tok.cpu(), ln.cpu()

    # ------------------------------------------------------------------------------------------------ public
    @torch.no_grad()
    def decode(self, src_list, cond0: int = 0, n_cond: int | None = None, backend: str = "hip"):
        """greedy decode of every source under conditions cond0 .. cond0 + n_cond - 1: a list (condition-major, as the reference
        appends them) of token lists [SOS, ..., EOS or the 24th item]"""
        return self._decode_chunks(src_list, cond0, n_cond, backend)[0]

    def _decode_chunks(self, src_list, cond0, n_cond, backend, gaps=False):
        """decode()'s chunk driver: (token lists,), or with gaps (backend="torch" only) (token lists, gap, top): regen_torch.decode's
        record, [n_cond * S, MAX_LEN - 1] each, in the order of the token lists"""
        n_cond = self.K - cond0 if n_cond is None else int(n_cond)
        if not (0 <= cond0 and n_cond >= 1 and cond0 + n_cond <= self.K):
            raise ValueError(f"conditions {cond0}..{cond0 + n_cond - 1} outside 0..{self.K - 1}")
        _check_backend(backend)
        src, lens = self._pack(src_list)
        S = src.shape[0]
        per = {c: [None] * S for c in range(n_cond)}
        record = tuple(torch.empty(n_cond, S, MAX_LEN - 1) for _ in range(2)) if gaps else ()
        for a, b in _chunks(S, max(1, ROWS_PER_CALL // n_cond) if backend == "hip" else 4 * ROWS_PER_TORCH):
            Lc = int(lens[a:b].max())
            chunk = src[a:b, :Lc].contiguous(), lens[a:b].contiguous(), cond0, n_cond
            tok, ln = self._decode_hip(*chunk) if backend == "hip" else _torch().decode(self, *chunk, record=tuple(r[:, a:b] for r in record))
            tl, nl = tok.tolist(), ln.tolist()
            for c in range(n_cond):
                for j in range(b - a):
                    r = c * (b - a) + j
                    per[c][a + j] = tl[r][:nl[r]]
        return ([per[c][s] for c in range(n_cond) for s in range(S)], *(r.flatten(0, 1) for r in record))

    @torch.no_grad()
    def decode_with_gaps(self, src_list, cond0: int = 0, n_cond: int | None = None):
        """backend="torch" decode that also returns, per row (same order) and step, the gap between the best and the second-best
        ALLOWED logit and the best logit (NaN after the row ended): a step whose gap is within rounding may legitimately differ"""
        return self._decode_chunks(src_list, cond0, n_cond, "torch", gaps=True)

    def translate(self, src_list, condition: int, backend: str = "hip"):
        """the reference's translate(model, src) under set_condition(condition), for every source: one int64 tensor each"""
        return [torch.tensor(t, dtype=torch.int64) for t in self.decode(src_list, condition, 1, backend)]

    # ------------------------------------------------------------------------------------------------ teacher-forced scoring
    def _pack_pairs(self, pairs, width):
        """the padded matrices of 2.Pretrain_regenerator.py:49-64 and :275-282: src [n, Ls], tgt_in / tgt_out [n, T], lengths with
        SOS and EOS counted; Ls and T are the file-wide widths (`width` overrides the ones derived from `pairs`)"""
        srcs = [[self.sos] + [int(v) for v in s] + [self.eos] for s, _ in pairs]
        tgts = [[self.sos] + [int(v) for v in t] + [self.eos] for _, t in pairs]
        Ls = max((len(s) for s in srcs), default=2)
        T = max(20, max((len(t) for t in tgts), default=2)) - 1
        if width is not None:
            wl, wt = int(width[0]), int(width[1])
            need_t = max((len(t) for t in tgts), default=2) - 1
            if wl < Ls or wt < need_t:
                raise ValueError(f"width {tuple(width)} is narrower than the pairs need ({Ls}, {need_t})")
            Ls, T = wl, wt
        if Ls > N_POS or T > N_POS:
            raise ValueError(f"widths ({Ls}, {T}): the regenerator's position table has {N_POS} rows")
        n = len(pairs)
        src = torch.zeros(n, Ls, dtype=torch.int64)
        tgt = torch.zeros(n, T + 1, dtype=torch.int64)
        for i in range(n):
            src[i, :len(srcs[i])] = torch.tensor(srcs[i])
            tgt[i, :len(tgts[i])] = torch.tensor(tgts[i])
        if n and (int(min(src.min(), tgt.min())) < 0 or int(max(src.max(), tgt.max())) >= self.n_rows):
            raise IndexError(f"ids outside [0, {self.n_rows})")
        return (src, torch.tensor([len(s) for s in srcs], dtype=torch.int64), tgt,
                torch.tensor([len(t) for t in tgts], dtype=torch.int64), Ls, T)

    def _params_as(self, dtype, device):
        key = (dtype, str(device))
        if key not in self._cast:
            self._cast[key] = {k: v.to(device=device, dtype=dtype) for k, v in self.p.items()}
        return self._cast[key]

    def _hip(self, name, ws_query, ws_sizes, pre, post, workspace, dropout, pair0, *, backward=False, grad=None, accumulate=False):
        """One call of the scoring family, enqueued on the current stream: name(plan, *pre, workspace, its bytes, *post, stream) in eval
        mode, name_train(..., p, seed, step, pair0, stream) with a RegenDropout.  Tensors in pre / post go in as their pointers.  The
        workspace is checked against ws_query(plan, *ws_sizes) by the library and allocated here when None.  A backward call
        (backward=True) also takes `grad` and `accumulate`: the flat gradient, a new buffer when None, goes in front of `post` and
        `accumulate` behind it, and the buffer is returned"""
        lib = _lib.load()
        plan = self.score_plan()
        nb = getattr(lib, ws_query)(C.byref(plan), *ws_sizes)
        if nb < 0:
            _lib.check(int(nb), ws_query)
        if workspace is None:
            workspace = torch.empty(int(nb), dtype=torch.uint8, device=self.device)
        if backward:
            if grad is None:
                if accumulate:
                    raise ValueError("accumulate=True needs the gradient buffer to add to")
                grad = torch.empty(plan.n_params, dtype=torch.float32, device=self.device)
            if grad.numel() != plan.n_params or grad.dtype != torch.float32:
                raise ValueError(f"grad must hold {plan.n_params} fp32 values")
            post = (grad, *post, int(bool(accumulate)))
        args = [_lib.ptr(v) if isinstance(v, torch.Tensor) else v
                for v in (C.byref(plan), *pre, C.c_void_p(workspace.data_ptr()), workspace.numel(), *post)]
        if eval_mode(dropout):
            _lib.check(getattr(lib, name)(*args, _lib.cur_stream()), name)
        else:
            _lib.check(getattr(lib, name + "_train")(*args, *_drop_args(dropout, pair0), _lib.cur_stream()), name + "_train")
        return grad

    def score_device(self, src, src_len, tgt, tgt_len, w, causal_source=True, workspace=None, dropout=None, pair0=0):
        """the HIP call on device tensors (src [n, Ls], tgt [n, T + 1] int64, w [n_w, n, K] fp32): nll [n_w, n, T] on the device.
        Only enqueues on the current stream (capturable); `workspace` may be reused between calls of the same sizes.  dropout (a
        RegenDropout) scores in train mode; row i then takes the masks of global pair pair0 + i"""
        (n, Ls), T, n_w = src.shape, tgt.shape[1] - 1, w.shape[0]
        nll = torch.empty(n_w, n, T, dtype=torch.float32, device=self.device)
        self._hip("dr4sr_regen_score", "dr4sr_regen_score_workspace_bytes", (n, Ls, T, n_w),
                  (src, src_len, tgt, tgt_len, n, Ls, T, w, n_w, int(bool(causal_source))), (nll,), workspace, dropout, pair0)
        return nll

    def condition_device(self, tgt, tgt_len, workspace=None, dropout=None, pair0=0):
        """condition logits [n, K] of the condition_encoder on device tensors (HIP; only enqueues); dropout / pair0 as score_device"""
        n, T = tgt.shape[0], tgt.shape[1] - 1
        out = torch.empty(n, self.K, dtype=torch.float32, device=self.device)
        self._hip("dr4sr_regen_score_condition", "dr4sr_regen_score_workspace_bytes", (n, 1, T, 1), (tgt, tgt_len, n, T), (out,),
                  workspace, dropout, pair0)
        return out

    # ------------------------------------------------------------------------------------------------ parameters in and out
    def state_dict(self):
        """the model's parameters by their state-dict names (fp32 clones on the model's device); item_embedding_decoder.weight is the
        same table as item_embedding.weight, as the reference ties them"""
        sd = {k: v.clone() for k, v in self.p.items()}
        sd["item_embedding_decoder.weight"] = sd["item_embedding.weight"]
        return sd

    @torch.no_grad()
    def load_params(self, params: dict):
        """overwrite parameters IN PLACE: self.p, the dtype casts and both flat buffers keep their device addresses, so plans, views
        and captured graphs stay valid.  `params` maps state-dict names to tensors of the stored shapes (a subset is allowed)"""
        params = {k: v for k, v in params.items() if k != "item_embedding_decoder.weight"}      # the same table as item_embedding.weight
        for name, v in params.items():
            if name not in self.p:
                raise KeyError(f"{name} is not a parameter of this model")
            if tuple(v.shape) != tuple(self.p[name].shape):
                raise ValueError(f"{name}: shape {tuple(v.shape)}, expected {tuple(self.p[name].shape)}")
        for name, v in params.items():
            self.p[name].copy_(v.detach().to(self.device, torch.float32))
            for cast in self._cast.values():
                cast[name].copy_(self.p[name].to(device=cast[name].device, dtype=cast[name].dtype))
        for buf, score in ((self._flat, False), (self._score_flat, True)):
            if buf is not None:
                self._fill_flat(buf, score, params)

    # ------------------------------------------------------------------------------------------------ gradients
    def grads_from_flat(self, flat):
        """views of a flat gradient buffer in the 98-tensor score layout, by state-dict name (70 names without a condition encoder)"""
        _, off, names = self._layout(True)
        return {name: flat[o:o + math.prod(shape)].view(shape)
                for o, name, shape in zip(off, names, score_param_shapes(self.n_rows, self.K)) if name in self.p}

    def condition_bwd_device(self, tgt, tgt_len, dlogits, grad=None, accumulate=False, workspace=None, dropout=None, pair0=0):
        """the HIP backward of condition_device on device tensors: dlogits [n, K] fp32 -> the flat gradient (98-tensor score layout;
        condition_encoder.* and the two tables receive values).  accumulate=False overwrites every element of `grad` (a new buffer
        when None), True adds to it.  Only enqueues on the current stream (capturable); the same inputs give the same bits"""
        n, T = tgt.shape[0], tgt.shape[1] - 1
        return self._hip("dr4sr_regen_score_condition_bwd", "dr4sr_regen_score_condition_bwd_workspace_bytes", (n, T),
                         (tgt, tgt_len, n, T, dlogits), (), workspace, dropout, pair0, backward=True, grad=grad, accumulate=accumulate)

    def score_bwd_device(self, src, src_len, tgt, tgt_len, w, dnll, causal_source=True, grad=None, accumulate=False, workspace=None,
                         dropout=None, pair0=0):
        """the HIP backward of score_device on device tensors: dnll [n_w, n, T] fp32 -> (flat gradient in the 98-tensor score layout,
        dw [n_w, n, K], nll [n_w, n, T]).  Self-contained (runs the forward it needs); accumulate=False overwrites every element of
        `grad` (a new buffer when None), True adds.  Only enqueues on the current stream; the same inputs give the same bits"""
        (n, Ls), T, n_w = src.shape, tgt.shape[1] - 1, w.shape[0]
        if tuple(dnll.shape) != (n_w, n, T):
            raise ValueError(f"dnll of shape {tuple(dnll.shape)}, expected ({n_w}, {n}, {T})")
        dw = torch.empty(n_w, n, self.K, dtype=torch.float32, device=self.device)
        nll = torch.empty(n_w, n, T, dtype=torch.float32, device=self.device)
        grad = self._hip("dr4sr_regen_score_bwd", "dr4sr_regen_score_bwd_workspace_bytes", (n, Ls, T, n_w),
                         (src, src_len, tgt, tgt_len, n, Ls, T, w, n_w, int(bool(causal_source)), dnll), (dw, nll), workspace, dropout,
                         pair0, backward=True, grad=grad, accumulate=accumulate)
        return grad, dw, nll

    def _loss_and_grad_hip(self, src, src_len, tgt, tgt_len, T, conditions, causal_source, noise, tau, entropy_weight, dropout=None, pair0=0):
        dev = self.device
        n = src.shape[0]
        encoder = isinstance(conditions, str)
        n_tok = max(int((tgt[:, 1:] != 0).sum()), 1)
        flat = None
        loss = torch.zeros((), dtype=torch.float64)
        entropy = torch.zeros((), dtype=torch.float64)
        dws, conds = [], []
        for a, b in _chunks(n, SCORE_BWD_PAIRS_PER_CALL):
            s_d, sl_d = src[a:b].to(dev).contiguous(), src_len[a:b].to(dev).contiguous()
            t_d, tl_d = tgt[a:b].to(dev).contiguous(), tgt_len[a:b].to(dev).contiguous()
            c = self.condition_device(t_d, tl_d, None, dropout, pair0 + a) if self.has_condition_encoder else None
            if encoder:                  # the few [n, K] operations between dw and the condition encoder's backward: torch autograd
                c_leaf = c.detach().requires_grad_(True)
                z = c_leaf if noise is None else c_leaf + torch.as_tensor(noise)[a:b].to(dev, torch.float32)
                w0 = torch.softmax(z / tau, -1)
                ent = -(w0 * torch.log(w0 + 1e-12)).sum(-1).sum() / n
                w = w0.detach()[None].contiguous()
            else:
                w = conditions[:, a:b].to(dev, torch.float32).contiguous()
            dnll = torch.full((w.shape[0], b - a, T), 1.0 / n_tok, dtype=torch.float32, device=dev)
            flat, dw, nll = self.score_bwd_device(s_d, sl_d, t_d, tl_d, w, dnll, causal_source, flat, accumulate=flat is not None,
                                                  dropout=dropout, pair0=pair0 + a)
            loss += float(nll.double().sum()) / n_tok
            if encoder:
                entropy += float(ent.detach())
                (dlog,) = torch.autograd.grad((w0 * dw[0]).sum() + entropy_weight * ent, c_leaf)
                self.condition_bwd_device(t_d, tl_d, dlog.contiguous(), flat, accumulate=True, dropout=dropout, pair0=pair0 + a)
            dws.append(dw)
            if c is not None:
                conds.append(c)
        n_w = 1 if encoder else conditions.shape[0]
        if flat is None:
            flat = torch.zeros(self.score_flat().numel(), dtype=torch.float32, device=dev)
        return GradResult(loss, entropy if encoder else None, self.grads_from_flat(flat),
                          torch.cat(dws, 1) if dws else torch.zeros(n_w, 0, self.K, device=dev), torch.cat(conds) if conds else None)

    def condition_grad(self, pairs, dlogits, width=None, backend: str = "hip", dtype=torch.float32, dropout=None, pair0: int = 0):
        """gradients of sum(cond_logits * dlogits) over the given pairs: state-dict name -> tensor for condition_encoder.* and the
        two tables (the vector-Jacobian product of score()'s cond_logits).  backend="hip" runs csrc/regen_score_bwd.hip, chunked
        with `accumulate`; backend="torch" is autograd through the eager restatement in `dtype`"""
        _check_backend(backend)
        if not self.has_condition_encoder:
            raise ValueError("condition_grad needs condition_encoder.* and this state dict has none")
        _, _, tgt, tgt_len, _, T = self._pack_pairs(pairs, width)
        n = len(pairs)
        dlogits = torch.as_tensor(dlogits)
        if tuple(dlogits.shape) != (n, self.K):
            raise ValueError(f"dlogits of shape {tuple(dlogits.shape)}, expected ({n}, {self.K})")
        dev = self.device
        names = ["item_embedding.weight", "position_embedding.weight"] + [k for k in score_param_names() if k.startswith("condition_encoder.")]
        if backend == "hip":
            flat = None
            # KEPT DIFFERENCE: this loop runs once for n = 0 (an empty call: the all-zero flat buffer the views below need); the
            # other chunk loops do not run at all
            for a, b in list(_chunks(n, COND_BWD_PAIRS_PER_CALL)) or [(0, 0)]:
                flat = self.condition_bwd_device(tgt[a:b].to(dev).contiguous(), tgt_len[a:b].to(dev).contiguous(),
                                                 dlogits[a:b].to(dev, torch.float32).contiguous(), flat, accumulate=flat is not None,
                                                 dropout=dropout, pair0=pair0 + a)
            g = self.grads_from_flat(flat)
            return {k: g[k] for k in names}
        return _torch().condition_grad(self, tgt, tgt_len, dlogits, names, dtype, dropout, pair0)

    def loss_and_grad(self, pairs, conditions, causal_source: bool = True, width=None, backend: str = "hip", dtype=torch.float32,
                      noise=None, tau: float = 1.0, entropy_weight: float = 0.0, dropout=None, pair0: int = 0):
        """The reference's training loss and its gradient with respect to every parameter: in eval mode (dropout=None), or in train
        mode with the masks a RegenDropout names (pair i takes the masks of global pair pair0 + i, whatever the chunking).

        loss: CrossEntropyLoss(ignore_index=0) over ALL given pairs as one batch, per weight vector and summed over them.
        conditions: a [n_w, n, K] tensor (a constant; `dw` is the loss's gradient with respect to it) or "encoder":
        w = softmax((cond_logits + noise) / tau), F.gumbel_softmax's soft sample for recorded noise (zero when None), and the
        differentiated scalar is CE + entropy_weight * (-(w log(w + 1e-12)).sum(-1).mean()); the reference uses weight 1.
        A target id outside its source makes the reference's loss inf: ValueError here.

        backend="hip": csrc/regen_score_bwd.hip, chunked at SCORE_BWD_PAIRS_PER_CALL pairs with `accumulate`; in "encoder" mode the
        few [n, K] operations between dw and the condition encoder's backward run in torch autograd on the device.
        backend="torch": autograd through the eager restatement, fp32 or fp64 (`dtype`): the float64 side of every check."""
        _check_backend(backend)
        src, src_len, tgt, tgt_len, Ls, T = self._pack_pairs(pairs, width)
        n = len(pairs)
        for i in range(n):
            have = set(src[i].tolist())
            if any(int(v) not in have for v in tgt[i, 1:int(tgt_len[i])].tolist()):
                raise ValueError(f"pair {i}: a target id is not in its source (the reference's loss is inf there)")
        encoder = isinstance(conditions, str)
        if encoder:
            if conditions != "encoder":
                raise ValueError(f"conditions must be 'encoder' or a [n_w, n_pair, K] tensor, not {conditions!r}")
            if not self.has_condition_encoder:
                raise ValueError("conditions='encoder' needs condition_encoder.* and this state dict has none")
            if noise is not None and tuple(torch.as_tensor(noise).shape) != (n, self.K):
                raise ValueError(f"noise of shape {tuple(torch.as_tensor(noise).shape)}, expected ({n}, {self.K})")
        else:
            conditions = torch.as_tensor(conditions)
            if conditions.dim() != 3 or tuple(conditions.shape[1:]) != (n, self.K):
                raise ValueError(f"condition weights of shape {tuple(conditions.shape)}, expected [n_w, {n}, {self.K}]")
        if backend == "hip":
            return self._loss_and_grad_hip(src, src_len, tgt, tgt_len, T, conditions, causal_source, noise, tau, entropy_weight, dropout,
                                           int(pair0))
        return _torch().loss_and_grad(self, src, tgt, tgt_len, conditions, causal_source, dtype, noise, tau, entropy_weight, dropout,
                                      int(pair0))

    @torch.no_grad()
    def score(self, pairs, conditions="all", causal_source: bool = True, width=None, backend: str = "hip", dtype=torch.float32,
              dropout=None, pair0: int = 0):
        """Teacher-forced per-token NLL of every (sequence, pattern) pair — the forward and loss of 2.Pretrain_regenerator.py's
        train_epoch in eval mode.  conditions: "all" (each of the K one-hot condition weights, the memory slices stage 3 decodes
        with), "encoder" (softmax of the condition_encoder's logits: training's weights without the Gumbel noise, tau = 1) or a
        [n_w, n_pair, K] tensor used as is.  causal_source=False scores with the bidirectional source encoder of stage 3.
        width=(Ls, T) scores at those matrix widths (a slice of a file scores as inside the file).  `dtype` applies to
        backend="torch" only.  dropout (a RegenDropout) scores in train mode: pair i takes the masks of global pair pair0 + i."""
        _check_backend(backend)
        src, src_len, tgt, tgt_len, Ls, T = self._pack_pairs(pairs, width)
        n = len(pairs)
        pair0 = int(pair0)
        if isinstance(conditions, str):
            if conditions not in ("all", "encoder"):
                raise ValueError(f"conditions must be 'all', 'encoder' or a [n_w, n_pair, K] tensor, not {conditions!r}")
            if conditions == "encoder" and not self.has_condition_encoder:
                raise ValueError("conditions='encoder' needs condition_encoder.* and this state dict has none")
            w = torch.eye(self.K)[:, None, :].expand(self.K, n, self.K) if conditions == "all" else None
        else:
            w = torch.as_tensor(conditions)
            if tuple(w.shape[1:]) != (n, self.K) or w.dim() != 3:
                raise ValueError(f"condition weights of shape {tuple(w.shape)}, expected [n_w, {n}, {self.K}]")
        dev = self.device
        if backend == "torch":
            nll, cond = _torch().score(self, src, tgt, tgt_len, w, causal_source, dtype, dropout, pair0)
        else:
            dtype = torch.float32
            nll, cond = [], []
            for a, b in _chunks(n, PAIRS_PER_CALL):
                s_d, sl_d = src[a:b].to(dev).contiguous(), src_len[a:b].to(dev).contiguous()
                t_d, tl_d = tgt[a:b].to(dev).contiguous(), tgt_len[a:b].to(dev).contiguous()
                c = self.condition_device(t_d, tl_d, None, dropout, pair0 + a) if self.has_condition_encoder else None
                wc = torch.softmax(c, -1)[None] if w is None else w[:, a:b]
                nll.append(self.score_device(s_d, sl_d, t_d, tl_d, wc.to(dev, torch.float32).contiguous(), causal_source, None, dropout,
                                             pair0 + a).cpu())
                if c is not None:
                    cond.append(c.cpu())
        n_w = 1 if w is None else w.shape[0]
        nll = torch.cat(nll, 1) if nll else torch.zeros(n_w, 0, T, dtype=dtype)
        return ScoreResult(nll, (tgt[:, 1:] != 0).sum(1), torch.cat(cond) if cond else None, Ls, T)


def _drop_args(dropout, pair0):
    if int(pair0) < 0:
        raise ValueError("pair0 must not be negative")
    return C.c_float(dropout.p), C.c_uint64(dropout.seed), C.c_uint32(dropout.step), C.c_int64(int(pair0))


class GradResult:
    """RegenModel.loss_and_grad's result: loss (float64 scalar: the cross entropy summed over the weight vectors), entropy (float64
    scalar, the mean condition entropy; None for constant weights), grads (state-dict name -> tensor), dw [n_w, n_pair, K] (the
    gradient with respect to the condition weights) and cond_logits [n_pair, K] or None"""

    def __init__(self, loss, entropy, grads, dw, cond_logits):
        self.loss, self.entropy, self.grads, self.dw, self.cond_logits = loss, entropy, grads, dw, cond_logits


class ScoreResult:
    """RegenModel.score's result: nll [n_w, n_pair, T] (0 where tgt_out is PAD, +inf where the target id is not in the source),
    n_tok [n_pair], cond_logits [n_pair, K] or None, and the widths (Ls, T) the pairs were scored at"""

    def __init__(self, nll, n_tok, cond_logits, Ls, T):
        self.nll, self.n_tok, self.cond_logits, self.width = nll, n_tok, cond_logits, (Ls, T)

    def per_pair(self):
        """[n_w, n_pair] float64: each pair's summed NLL (its negative log-likelihood under each condition weight)"""
        return self.nll.double().sum(-1)

    def loss(self):
        """[n_w] float64: nn.CrossEntropyLoss(ignore_index=0) of the reference over ALL given pairs as one batch (sum of the token
        NLLs over the token count), summed in float64 on the host"""
        return self.per_pair().sum(-1) / max(int(self.n_tok.sum()), 1)


def random_state_dict(n_item: int = NUM_ITEM["toy"], K: int = 5, seed: int = 0, std: float = 0.1, condition_encoder: bool = False):
    """a seeded random regenerator state dict in the reference's names (normal weights, LayerNorm weight 1 / bias 0): the
    measurement's worst case (no row stops early) and the synthetic cross-checks' model"""
    g = torch.Generator().manual_seed(seed)
    names, shapes = (score_param_names(), score_param_shapes(n_item + 2, K)) if condition_encoder else (param_names(), param_shapes(n_item + 2, K))
    sd = {}
    for name, shape in zip(names, shapes):     # condition_encoder.* is drawn after everything else: the other tensors do not depend on the flag
        if name.split(".")[-2].startswith("norm"):
            sd[name] = torch.ones(shape) if name.endswith("weight") else torch.zeros(shape)
        else:
            sd[name] = std * torch.randn(shape, generator=g)
    sd["item_embedding_decoder.weight"] = sd["item_embedding.weight"]
    return sd


def source_rows(original_data):
    """3.Hybrid_inference.py:250-254: [SOS] + hist[:seqlen] + [target[seqlen - 1]] + [EOS] per train row, without SOS / EOS"""
    return [list(r[1][:r[3]]) + [r[2][r[3] - 1]] for r in original_data]


def regen_rows(token_lists, max_seq_len: int = MAX_SEQ_LEN):
    """3.Hybrid_inference.py:265-290: decoded token lists (condition-major) -> the new training rows, in the reference's order"""
    train_set = set()
    for toks in token_lists:
        train_set.add(tuple(int(v) for v in toks[1:-1]))

    def truncate_or_pad(seq):
        return seq[-max_seq_len:] if len(seq) > max_seq_len else seq + [0] * (max_seq_len - len(seq))

    rows = []
    for t in train_set:
        seq = list(t)
        seq_len = sum(a != 0 for a in seq[:-1])
        if seq_len == 0:
            continue
        rows.append([1, truncate_or_pad(seq[:-1]), truncate_or_pad(seq[1:]), seq_len, [1] * max_seq_len, [0] * max_seq_len])
    return rows


def hybrid_inference(root_path: str, ckpt_name: str = "regenerator.pth", begin: int = 0, end: int = 1000000, backend: str = "hip",
                     device="cuda", out_name: str = "train_regen.pth"):
    """3.Hybrid_inference.py's __main__: reads train.pth, patterns.pth and the regenerator under root_path, decodes rows
    begin*5000 : end*5000 under every condition, writes original_rows + patterns + new_rows to train_regen.pth; returns the path"""
    parts = root_path.split("/")
    dataset = parts[-2] if len(parts) >= 2 else None        # e.g. 'toy' in './dataset/amazon-toys/toy/' (:236)
    sd = torch.load(os.path.join(root_path, ckpt_name), map_location="cpu")
    model = RegenModel.from_state_dict(sd, device, dataset=dataset)
    original_data = torch.load(os.path.join(root_path, "train.pth"))
    ori_pattern = torch.load(os.path.join(root_path, "patterns.pth"))
    seqs = source_rows(original_data)[begin * 5000:end * 5000]
    src = [[model.sos] + s + [model.eos] for s in seqs]
    tokens = model.decode(src, 0, model.K, backend) if src else []
    out_path = os.path.join(root_path, out_name)
    torch.save(original_data + ori_pattern + regen_rows(tokens), out_path)
    return out_path


def score_file(root_path: str, pairs_file: str = "seq-pat-pair.pth", ckpt_name: str = "regenerator.pth", begin: int = 0, end: int = 1000000,
               causal_source: bool = True, backend: str = "hip", device="cuda"):
    """the --score report: teacher-forced loss of the pairs begin*5000 : end*5000 of a pairs file, scored at the widths of the whole
    file, under each one-hot condition and under the condition_encoder's own softmax"""
    parts = root_path.split("/")
    dataset = parts[-2] if len(parts) >= 2 else None
    model = RegenModel.from_state_dict(torch.load(os.path.join(root_path, ckpt_name), map_location="cpu"), device, dataset=dataset)
    pairs = torch.load(os.path.join(root_path, pairs_file))
    width = model._pack_pairs(pairs, None)[4:]
    pairs = pairs[begin * 5000:end * 5000]
    res = model.score(pairs, "all", causal_source, width, backend)
    per = res.per_pair()                                         # [K, n]
    n_tok = max(int(res.n_tok.sum()), 1)
    best = per.argmin(0)
    rep = {"pairs": len(pairs), "tokens": int(res.n_tok.sum()), "width": list(width), "causal_source": bool(causal_source),
           "inf_tokens": int(torch.isinf(res.nll).sum()),
           "loss_encoder": None, "loss_best_condition": float(per.min(0).values.sum() / n_tok),
           "nll_per_condition": [float(v) for v in res.loss()],
           "argmin_hist": torch.bincount(best, minlength=model.K).tolist(),
           "encoder_argmax_hist": None, "agreement": None}
    if model.has_condition_encoder and res.cond_logits is not None:
        rep["loss_encoder"] = float(model.score(pairs, "encoder", causal_source, width, backend).loss()[0])
        top = res.cond_logits.argmax(-1)
        rep["encoder_argmax_hist"] = torch.bincount(top, minlength=model.K).tolist()
        rep["agreement"] = float((top == best).double().mean()) if len(pairs) else None
    return rep


def main(argv=None):
    ap = argparse.ArgumentParser(description="DR4SR stage 3: regenerate train_regen.pth with the pre-trained regenerator; "
                                             "--score: teacher-forced loss of a regenerator on a pairs file instead")
    ap.add_argument("--root_path", type=str, default="./dataset/amazon-toys/toy/", help="The path to the dataset.")
    ap.add_argument("--ckpt_name", type=str, default="regenerator.pth", help="The name of pretrained regenerator")
    ap.add_argument("--begin", "-b", type=int, default=0, help="Used for multi-processing. Beginning of the inference.")
    ap.add_argument("--end", "-e", type=int, default=1000000, help="Used for multi-processing. End of the inference.")
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--score", action="store_true", help="print one JSON line of teacher-forced losses instead of decoding")
    ap.add_argument("--pairs_file", type=str, default="seq-pat-pair.pth", help="--score: the pairs file under root_path")
    ap.add_argument("--bidirectional_source", action="store_true", help="--score: stage 3's source encoder mask instead of stage 2's")
    ap.add_argument("--backend", choices=("hip", "torch"), default="hip", help="--score: 'torch' is the eager cross-check (runs on --device)")
    ap.add_argument("--device", type=str, default=None, help="--score with --backend torch: e.g. cpu")
    a = ap.parse_args(argv)
    if a.score:
        dev = a.device or f"cuda:{a.gpu}"
        if a.backend == "hip" or dev.startswith("cuda"):
            torch.cuda.set_device(a.gpu)
        print(json.dumps(score_file(a.root_path, a.pairs_file, a.ckpt_name, a.begin, a.end, not a.bidirectional_source, a.backend, dev)))
        return
    torch.cuda.set_device(a.gpu)
    path = hybrid_inference(a.root_path, a.ckpt_name, a.begin, a.end, "hip", torch.device("cuda", a.gpu))
    print(path)


if __name__ == "__main__":
    main()
