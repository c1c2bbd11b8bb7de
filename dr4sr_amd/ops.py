"""PyTorch custom-op registration of the dense C-ABI entry points: `torch.ops.dr4sr_hip.*`.

SURVEY.md §8(b) / BASELINE north_star describe the native layer as "PyTorch-ROCm custom ops".  The compute library itself stays a
torch-free C ABI (include/dr4sr_hip.h — that is what makes it bindable from anything); this module registers the stateless,
tensor-in / tensor-out subset of it with the torch dispatcher through `torch.library`, so that the ops are visible as
`torch.ops.dr4sr_hip.<name>`, carry schemas, fake (meta) kernels for shape inference and autograd formulas, and can be called from
a reference-style model written against plain torch ops:

    embed_gather_posadd(E, P, idx) -> x                       model/sasrec.py:43-46,:64   (bit-exact with torch)
    score_bce(query, E, target, neg) -> (loss_pos, stats)     model/basemodel.py:204-214 + loss_func.py:9-38  (autograd: d query, d E)
    score_bpr(query, E, target, neg) -> (loss_pos, stats)     ... + loss_func.py:40-48
    loss_from_scores(pos, neg, kind) -> (loss_pos, stats)     model/loss_func.py on score tensors (autograd: d pos, d neg)
    neg_sample(n, n_items, seed, step) -> ids                 model/basemodel.py:50-61
    full_score_topk(q, E, hist, item_blocked, k) -> (score, ids)   model/basemodel.py:354-365
    target_rank(q, E, target, hist, item_blocked) -> rank int32 [B]   the target's position in that top-k order, without the top-k
    fused_adam_(params, grads, m, v, state, lr, b1, b2, eps, wd)   torch.optim.Adam on flat buffers (in place)
    sasrec_layer(x, key_padding_mask?, causal, <12 layer tensors>, n_head, eps, p_drop, seed, step, layer) -> (y, saved)
                                                              one TransformerEncoderLayer of model/sasrec.py:21-30,:68 on dense [B, L, D]
                                                              (autograd: d x and the 12 weight gradients, bit-reproducible)
    sasrec_layer_packed(x, seqlen, causal, <12 layer tensors>, n_head, eps, p_drop, seed, step, layer) -> (y, saved)
                                                              the same layer on post-padded rows: keys at pos >= seqlen[b] are padded, y is
                                                              0 there; short sequences share a 64-row tile (csrc/layer_packed.hip)
    seq_pool(x, seqlen, pooling) -> out                       module/layers.py:41-73 'origin' | 'last', module/functional.py:50-55 'mean'
    dropout(x, p_drop, seed, step, site) -> out               model/sasrec.py:66 with the library's Philox masks (DR4SR_SITE_EMB)
    fmlp_layer(x, complex_weight, filter_ln_w, filter_ln_b, dense_1_w, dense_1_b, dense_2_w, dense_2_b, inter_ln_w, inter_ln_b,
               eps, p_drop, seed, step, layer) -> (y, saved)  one FMLP Layer (FilterLayer + Intermediate) of module/layers.py:740-791 on dense
                                                              [B, L, 64] (autograd: d x and the 9 weight gradients, bit-reproducible)
    layer_norm(x, weight, bias, eps) -> y                     nn.LayerNorm over the last dimension: model/fmlp.py:25 (autograd: d x, d w, d b)
    gru_layer(x, weight_ih, weight_hh, seqlen?) -> (y, saved)   one layer of nn.GRU(bias=False, batch_first=True), module/layers.py:117-136, on
                                                              dense [B, L, I]; seqlen skips the steps behind each length (autograd: d x,
                                                              d weight_ih, d weight_hh, bit-reproducible)
    (+ embed_gather_posadd_backward, sasrec_layer_backward, sasrec_layer_packed_backward, seq_pool_backward, fmlp_layer_backward, layer_norm_backward,
     gru_layer_backward: the autograd formulas, ops themselves)

Every implementation only enqueues HIP kernels of libdr4sr_hip.so on the current stream; there is no CPU kernel (the ops raise on
CPU tensors).  The encoder LAYER is a dispatcher op: stateless, dense tensors in and out, its dropout keyed by explicit (seed, step,
layer) arguments — dr4sr_amd/module/layers.py SASRecQueryEncoderOps is the reference's query encoder written on these ops, FMLPOps /
FMLPEncoderOps the reference's FMLP on fmlp_layer and layer_norm.  What stays
outside the dispatcher are the plan-based entry points (whole fused training steps, the packed encoders with their workspaces), driven by
the engines (dr4sr_amd/engine.py ...): they own device state (workspace, RNG step, Adam step).
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import os

import torch

from . import _lib

NS = "dr4sr_hip"


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.Dr4srError("torch.ops.dr4sr_hip.* run on the GPU only (libdr4sr_hip.so has no CPU path)")


# ------------------------------------------------------------------------------------------------ embed_gather_posadd
@torch.library.custom_op(f"{NS}::embed_gather_posadd", mutates_args=())
def embed_gather_posadd(E: torch.Tensor, P: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    _need_cuda(E, P, idx)
    lib = _lib.load()
    B, L = idx.shape
    N, D = E.shape
    E, P, idx = E.contiguous(), P.contiguous(), idx.contiguous()
    # nn.Embedding's IndexError (the kernel itself clamps).  The check is an extra launch + a blocking device-to-host read: skipped
    # inside a stream capture (a synchronisation there raises) and under DR4SR_NO_ID_CHECK — check the id tensor once up front then
    # (BaseModel._check_dataset_ids does so for every split's resident tensors)
    if not torch.cuda.is_current_stream_capturing() and not os.environ.get("DR4SR_NO_ID_CHECK"):
        _lib.check_ids(idx, N, "embed_gather_posadd")
    out = torch.empty(B, L, D, dtype=torch.float32, device=E.device)
    _lib.check(lib.dr4sr_embed_gather_posadd(_lib.ptr(E), _lib.ptr(P), _lib.ptr(idx), _lib.ptr(out), B, L, D, N, _lib.cur_stream()),
               "dr4sr_embed_gather_posadd")
    return out


@embed_gather_posadd.register_fake
def _(E, P, idx):
    return E.new_empty(idx.shape[0], idx.shape[1], E.shape[1])


@torch.library.custom_op(f"{NS}::embed_gather_posadd_backward", mutates_args=())
def embed_gather_posadd_backward(g_x: torch.Tensor, idx: torch.Tensor, n_items: int, n_pos: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (dE [n_items, D], dP [n_pos, D]); the PAD row of dE is exactly 0 (nn.Embedding(padding_idx=0), model/basemodel.py:42)"""
    _need_cuda(g_x, idx)
    lib = _lib.load()
    B, L, D = (int(s) for s in g_x.shape)
    g, ic = g_x.contiguous().float(), idx.contiguous()
    dE = torch.empty(n_items, D, dtype=torch.float32, device=g.device)
    dP = torch.empty(n_pos, D, dtype=torch.float32, device=g.device)
    _lib.check(lib.dr4sr_embed_gather_posadd_bwd(_lib.ptr(g), _lib.ptr(ic), B, L, D, n_items, n_pos, _lib.ptr(dE), _lib.ptr(dP),
                                                 _lib.cur_stream()), "dr4sr_embed_gather_posadd_bwd")
    return dE, dP


@embed_gather_posadd_backward.register_fake
def _(g_x, idx, n_items, n_pos):
    return g_x.new_empty(n_items, g_x.shape[2]), g_x.new_empty(n_pos, g_x.shape[2])


def _egp_setup(ctx, inputs, output):
    E, P, idx = inputs
    ctx.n_items, ctx.n_pos = E.shape[0], P.shape[0]
    ctx.save_for_backward(idx)


def _egp_backward(ctx, g):
    dE, dP = embed_gather_posadd_backward(g, ctx.saved_tensors[0], ctx.n_items, ctx.n_pos)
    return dE, dP, None


embed_gather_posadd.register_autograd(_egp_backward, setup_context=_egp_setup)


# ------------------------------------------------------------------------------------------------ scorer + loss
def _score_fwd(kind: int, query, E, target, neg):
    _need_cuda(query, E, target, neg)
    lib = _lib.load()
    B = int(target.shape[0])
    L = int(target.shape[1]) if target.dim() == 2 else 1
    D = int(E.shape[1])
    q, Ec, tg, ng = query.contiguous(), E.contiguous(), target.contiguous(), neg.contiguous()
    lp = torch.empty(B * L, dtype=torch.float32, device=q.device)
    stats = torch.zeros(2, dtype=torch.float32, device=q.device)
    fn = lib.dr4sr_score_bpr_fwd if kind else lib.dr4sr_score_bce_fwd
    _lib.check(fn(_lib.ptr(q), _lib.ptr(Ec), _lib.ptr(tg), _lib.ptr(ng), None, None, _lib.ptr(lp), _lib.ptr(stats), B, L, D,
                  _lib.cur_stream()), "dr4sr_score_fwd")
    return lp.view(target.shape), stats


def _score_bwd(kind: int, query, E, target, neg, g_loss_pos):
    lib = _lib.load()
    B = int(target.shape[0])
    L = int(target.shape[1]) if target.dim() == 2 else 1
    D = int(E.shape[1])
    q, Ec, tg, ng = query.contiguous(), E.contiguous(), target.contiguous(), neg.contiguous()
    w = g_loss_pos.contiguous().view(-1).float()
    dq = torch.empty_like(q)
    dE = torch.zeros_like(Ec)
    fn = lib.dr4sr_score_bpr_bwd if kind else lib.dr4sr_score_bce_bwd
    _lib.check(fn(_lib.ptr(q), _lib.ptr(Ec), _lib.ptr(tg), _lib.ptr(ng), _lib.ptr(w), None, _lib.ptr(dq), _lib.ptr(dE), B, L, D,
                  _lib.cur_stream()), "dr4sr_score_bwd")
    return dq.view(query.shape), dE


def _make_scorer(name: str, kind: int):
    @torch.library.custom_op(f"{NS}::{name}", mutates_args=())
    def fwd(query: torch.Tensor, E: torch.Tensor, target: torch.Tensor, neg: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        return _score_fwd(kind, query, E, target, neg)

    @fwd.register_fake
    def _(query, E, target, neg):
        return query.new_empty(target.shape), query.new_empty(2)

    @torch.library.custom_op(f"{NS}::{name}_backward", mutates_args=())
    def bwd(query: torch.Tensor, E: torch.Tensor, target: torch.Tensor, neg: torch.Tensor,
            g_loss_pos: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        return _score_bwd(kind, query, E, target, neg, g_loss_pos)

    @bwd.register_fake
    def _(query, E, target, neg, g_loss_pos):
        return torch.empty_like(query), torch.empty_like(E)

    def setup(ctx, inputs, output):
        ctx.save_for_backward(*inputs)

    def backward(ctx, g_lp, g_stats):
        query, E, target, neg = ctx.saved_tensors
        dq, dE = bwd(query, E, target, neg, g_lp)
        return dq, dE, None, None

    fwd.register_autograd(backward, setup_context=setup)
    return fwd, bwd


score_bce, score_bce_backward = _make_scorer("score_bce", 0)
score_bpr, score_bpr_backward = _make_scorer("score_bpr", 1)


@torch.library.custom_op(f"{NS}::loss_from_scores", mutates_args=())
def loss_from_scores(pos: torch.Tensor, neg: torch.Tensor, kind: int) -> Tuple[torch.Tensor, torch.Tensor]:
    _need_cuda(pos, neg)
    lib = _lib.load()
    p, ng = pos.contiguous().float(), neg.contiguous().float()
    n, K = p.numel(), int(ng.shape[-1])
    lp = torch.empty(n, dtype=torch.float32, device=p.device)
    stats = torch.zeros(2, dtype=torch.float32, device=p.device)
    _lib.check(lib.dr4sr_loss_from_scores_fwd(_lib.ptr(p), _lib.ptr(ng), n, K, kind, _lib.ptr(lp), _lib.ptr(stats), _lib.cur_stream()),
               "dr4sr_loss_from_scores_fwd")
    return lp.view(pos.shape), stats


@loss_from_scores.register_fake
def _(pos, neg, kind):
    return pos.new_empty(pos.shape), pos.new_empty(2)


@torch.library.custom_op(f"{NS}::loss_from_scores_backward", mutates_args=())
def loss_from_scores_backward(pos: torch.Tensor, neg: torch.Tensor, kind: int, g_loss_pos: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    lib = _lib.load()
    p, ng = pos.contiguous().float(), neg.contiguous().float()
    n, K = p.numel(), int(ng.shape[-1])
    dp, dn = torch.empty_like(p), torch.empty_like(ng)
    g = g_loss_pos.contiguous().view(-1).float()
    _lib.check(lib.dr4sr_loss_from_scores_bwd(_lib.ptr(p), _lib.ptr(ng), n, K, kind, _lib.ptr(g), None, _lib.ptr(dp), _lib.ptr(dn),
                                              _lib.cur_stream()), "dr4sr_loss_from_scores_bwd")
    return dp.view(pos.shape), dn.view(neg.shape)


@loss_from_scores_backward.register_fake
def _(pos, neg, kind, g_loss_pos):
    return torch.empty_like(pos), torch.empty_like(neg)


def _lfs_setup(ctx, inputs, output):
    pos, neg, kind = inputs
    ctx.kind = kind
    ctx.save_for_backward(pos, neg)


def _lfs_backward(ctx, g_lp, g_stats):
    pos, neg = ctx.saved_tensors
    dp, dn = loss_from_scores_backward(pos, neg, ctx.kind, g_lp)
    return dp, dn, None


loss_from_scores.register_autograd(_lfs_backward, setup_context=_lfs_setup)


# ------------------------------------------------------------------------------------------------ neg_sample / topk / adam
@torch.library.custom_op(f"{NS}::neg_sample", mutates_args=(), device_types="cuda")
def neg_sample(n: int, n_items: int, seed: int, step: int, like: torch.Tensor) -> torch.Tensor:
    """`like` only supplies the device (custom ops need a tensor input to dispatch on)"""
    lib = _lib.load()
    out = torch.empty(n, dtype=torch.int64, device=like.device)
    _lib.check(lib.dr4sr_neg_sample(_lib.ptr(out), n, n_items, seed & 0xFFFFFFFFFFFFFFFF, step & 0xFFFFFFFF, _lib.cur_stream()), "dr4sr_neg_sample")
    return out


@neg_sample.register_fake
def _(n, n_items, seed, step, like):
    return like.new_empty(n, dtype=torch.int64)


@torch.library.custom_op(f"{NS}::full_score_topk", mutates_args=())
def full_score_topk(q: torch.Tensor, E: torch.Tensor, hist: Optional[torch.Tensor], item_blocked: Optional[torch.Tensor],
                    k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    _need_cuda(q, E, hist, item_blocked)
    lib = _lib.load()
    B, D = q.shape
    N = int(E.shape[0])
    qc, Ec = q.contiguous(), E.contiguous()
    hc = hist.contiguous() if hist is not None else None
    bc = item_blocked.contiguous() if item_blocked is not None else None
    score = torch.empty(B, k, dtype=torch.float32, device=q.device)
    ids = torch.empty(B, k, dtype=torch.int64, device=q.device)
    nb = int(lib.dr4sr_full_score_topk_workspace_bytes(B, N))
    ws = torch.empty(max(nb // 4, 1), dtype=torch.float32, device=q.device)
    _lib.check(lib.dr4sr_full_score_topk_masked_ws(_lib.ptr(qc), _lib.ptr(Ec), _lib.ptr(hc), _lib.ptr(bc), _lib.ptr(score), _lib.ptr(ids), B, D,
                                                   N, int(hc.shape[1]) if hc is not None else 0, k, _lib.ptr(ws), nb, _lib.cur_stream()),
               "dr4sr_full_score_topk_masked_ws")
    return score, ids


@full_score_topk.register_fake
def _(q, E, hist, item_blocked, k):
    return q.new_empty(q.shape[0], k), q.new_empty(q.shape[0], k, dtype=torch.int64)


@torch.library.custom_op(f"{NS}::target_rank", mutates_args=())
def target_rank(q: torch.Tensor, E: torch.Tensor, target: torch.Tensor, hist: Optional[torch.Tensor],
                item_blocked: Optional[torch.Tensor]) -> torch.Tensor:
    """int32 [B]: how many valid items precede target[b] in (score descending, id ascending) order; _lib.RANK_NONE for a target that
    is not a valid item (PAD, out of range, blocked, in the row's own history)"""
    _need_cuda(q, E, target, hist, item_blocked)
    lib = _lib.load()
    B, D = q.shape
    N = int(E.shape[0])
    qc, Ec, tc = q.contiguous(), E.contiguous(), target.contiguous().view(-1)
    hc = hist.contiguous() if hist is not None else None
    bc = item_blocked.contiguous() if item_blocked is not None else None
    rank = torch.empty(B, dtype=torch.int32, device=q.device)
    nb = int(lib.dr4sr_target_rank_workspace_bytes(B))
    ws = torch.empty(max(nb // 4, 1), dtype=torch.float32, device=q.device)
    _lib.check(lib.dr4sr_target_rank(_lib.ptr(qc), _lib.ptr(Ec), _lib.ptr(tc), _lib.ptr(hc), _lib.ptr(bc), _lib.ptr(rank), B, D, N,
                                     int(hc.shape[1]) if hc is not None else 0, _lib.ptr(ws), nb, _lib.cur_stream()), "dr4sr_target_rank")
    return rank


@target_rank.register_fake
def _(q, E, target, hist, item_blocked):
    return q.new_empty(q.shape[0], dtype=torch.int32)


@torch.library.custom_op(f"{NS}::fused_adam_",mutates_args=("params", "adam_m", "adam_v", "state"))
def fused_adam_(params: torch.Tensor, grads: torch.Tensor, adam_m: torch.Tensor, adam_v: torch.Tensor, state: torch.Tensor,
                lr: float, beta1: float, beta2: float, eps: float, weight_decay: float) -> None:
    """torch.optim.Adam on flat fp32 buffers; grads has n + 4 floats, grads[n] = the normaliser the gradient is divided by
    (include/dr4sr_hip.h: dr4sr_adam_flat); state = the engine's int32 device words (state[0] = step counter)"""
    _need_cuda(params, grads, adam_m, adam_v, state)
    lib = _lib.load()
    _lib.check(lib.dr4sr_adam_flat(_lib.ptr(params), _lib.ptr(grads), _lib.ptr(adam_m), _lib.ptr(adam_v), params.numel(), _lib.ptr(state),
                                   lr, beta1, beta2, eps, weight_decay, _lib.cur_stream()), "dr4sr_adam_flat")


# ------------------------------------------------------------------------------------------------ encoder layer / pooling / dropout
def _layer_dims(x, in_proj_weight, linear1_weight, n_head):
    if x.dim() != 3 or x.dtype != torch.float32:
        raise _lib.Dr4srError("sasrec_layer: x must be a [B, L, D] float32 tensor")
    B, L, D = (int(s) for s in x.shape)
    return B, L, D, int(n_head), int(linear1_weight.shape[0])


def _saved_floats(B, L, D, F):
    return B * ((L * (6 * D + F) + 2 * L * L + 3) // 4 * 4)           # dr4sr_sasrec_layer_saved_floats for a supported shape


def _mask_u8(m):
    if m is None:
        return None
    m = m.contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m.to(torch.uint8)


def _layer_struct(cls, tensors):
    return cls(*[_lib.ptr(t) for t in tensors])


@torch.library.custom_op(f"{NS}::sasrec_layer", mutates_args=())
def sasrec_layer(x: torch.Tensor, key_padding_mask: Optional[torch.Tensor], causal: bool, in_proj_weight: torch.Tensor,
                 in_proj_bias: torch.Tensor, out_proj_weight: torch.Tensor, out_proj_bias: torch.Tensor, linear1_weight: torch.Tensor,
                 linear1_bias: torch.Tensor, linear2_weight: torch.Tensor, linear2_bias: torch.Tensor, norm1_weight: torch.Tensor,
                 norm1_bias: torch.Tensor, norm2_weight: torch.Tensor, norm2_bias: torch.Tensor, n_head: int, eps: float, p_drop: float,
                 seed: int, step: int, layer: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """one post-norm TransformerEncoderLayer (model/sasrec.py:21-30) on x [B, L, D]; key_padding_mask [B, L] (True / non-zero: padded)
    or None, causal adds triu(1); a query with no admissible key gets a zero attention context (include/dr4sr_hip.h).  `saved` is the
    opaque buffer the backward reads"""
    ws_ = (in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias, linear1_weight, linear1_bias, linear2_weight, linear2_bias,
           norm1_weight, norm1_bias, norm2_weight, norm2_bias)
    _need_cuda(x, key_padding_mask, *ws_)
    lib = _lib.load()
    B, L, D, H, F = _layer_dims(x, in_proj_weight, linear1_weight, n_head)
    n = int(lib.dr4sr_sasrec_layer_saved_floats(B, L, D, H, F))
    _lib.check(min(n, 0), "dr4sr_sasrec_layer_saved_floats")
    xc, kp = x.contiguous(), _mask_u8(key_padding_mask)
    wc = [t.contiguous() for t in ws_]
    y = torch.empty_like(xc)
    saved = torch.empty(max(n, 1), dtype=torch.float32, device=x.device)
    w = _layer_struct(_lib.LayerWeights, wc)
    _lib.check(lib.dr4sr_sasrec_layer_fwd(_lib.ptr(xc), _lib.ptr(kp), int(causal), w, B, L, D, H, F, eps, p_drop, seed & 0xFFFFFFFFFFFFFFFF,
                                          step & 0xFFFFFFFF, layer, _lib.ptr(y), _lib.ptr(saved), _lib.cur_stream()), "dr4sr_sasrec_layer_fwd")
    return y, saved


@sasrec_layer.register_fake
def _(x, key_padding_mask, causal, in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias, linear1_weight, linear1_bias, linear2_weight,
      linear2_bias, norm1_weight, norm1_bias, norm2_weight, norm2_bias, n_head, eps, p_drop, seed, step, layer):
    B, L, D = x.shape
    return torch.empty_like(x), x.new_empty(max(_saved_floats(B, L, D, linear1_weight.shape[0]), 1))


@torch.library.custom_op(f"{NS}::sasrec_layer_backward", mutates_args=())
def sasrec_layer_backward(x: torch.Tensor, key_padding_mask: Optional[torch.Tensor], causal: bool, in_proj_weight: torch.Tensor,
                          in_proj_bias: torch.Tensor, out_proj_weight: torch.Tensor, out_proj_bias: torch.Tensor,
                          linear1_weight: torch.Tensor, linear1_bias: torch.Tensor, linear2_weight: torch.Tensor, linear2_bias: torch.Tensor,
                          norm1_weight: torch.Tensor, norm1_bias: torch.Tensor, norm2_weight: torch.Tensor, norm2_bias: torch.Tensor,
                          n_head: int, eps: float, p_drop: float, seed: int, step: int, layer: int, saved: torch.Tensor,
                          dy: torch.Tensor) -> List[torch.Tensor]:
    """-> [dx, the 12 weight gradients in the argument order]; written, not accumulated; bit-reproducible"""
    ws_ = (in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias, linear1_weight, linear1_bias, linear2_weight, linear2_bias,
           norm1_weight, norm1_bias, norm2_weight, norm2_bias)
    _need_cuda(x, key_padding_mask, saved, dy, *ws_)
    lib = _lib.load()
    B, L, D, H, F = _layer_dims(x, in_proj_weight, linear1_weight, n_head)
    nb = int(lib.dr4sr_sasrec_layer_workspace_bytes(B, L, D, H, F))
    _lib.check(min(nb, 0), "dr4sr_sasrec_layer_workspace_bytes")
    xc, kp, dyc, sc = x.contiguous(), _mask_u8(key_padding_mask), dy.contiguous().float(), saved.contiguous()
    wc = [t.contiguous() for t in ws_]
    dx = torch.empty_like(xc)
    dws = [torch.empty_like(t) for t in wc]
    ws = torch.empty(max(nb // 4, 1), dtype=torch.float32, device=x.device)
    w, g = _layer_struct(_lib.LayerWeights, wc), _layer_struct(_lib.LayerGrads, dws)
    _lib.check(lib.dr4sr_sasrec_layer_bwd(_lib.ptr(xc), _lib.ptr(kp), int(causal), w, B, L, D, H, F, eps, p_drop, seed & 0xFFFFFFFFFFFFFFFF,
                                          step & 0xFFFFFFFF, layer, _lib.ptr(sc), _lib.ptr(dyc), _lib.ptr(dx), g, _lib.ptr(ws), nb,
                                          _lib.cur_stream()), "dr4sr_sasrec_layer_bwd")
    return [dx] + dws


@sasrec_layer_backward.register_fake
def _(x, key_padding_mask, causal, in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias, linear1_weight, linear1_bias, linear2_weight,
      linear2_bias, norm1_weight, norm1_bias, norm2_weight, norm2_bias, n_head, eps, p_drop, seed, step, layer, saved, dy):
    return [torch.empty_like(t) for t in (x, in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias, linear1_weight, linear1_bias,
                                          linear2_weight, linear2_bias, norm1_weight, norm1_bias, norm2_weight, norm2_bias)]


def _layer_setup(ctx, inputs, output):
    ctx.rest = inputs[1:3] + inputs[15:]                    # mask, causal, n_head, eps, p_drop, seed, step, layer
    ctx.save_for_backward(inputs[0], *inputs[3:15], output[1])
    ctx.mark_non_differentiable(output[1])


def _layer_backward(ctx, g_y, g_saved):
    x, *w, saved = ctx.saved_tensors
    mask, causal = ctx.rest[:2]
    out = sasrec_layer_backward(x, mask, causal, *w, *ctx.rest[2:], saved, g_y)
    return (out[0], None, None, *out[1:], None, None, None, None, None, None)


sasrec_layer.register_autograd(_layer_backward, setup_context=_layer_setup)


# ------------------------------------------------------------------------------------------------ encoder layer with sequence lengths
_W_NAMES = ("in_proj_weight", "in_proj_bias", "out_proj_weight", "out_proj_bias", "linear1_weight", "linear1_bias", "linear2_weight",
            "linear2_bias", "norm1_weight", "norm1_bias", "norm2_weight", "norm2_bias")


def _packed_saved_floats(B, L, D, F):
    return B * (L * (6 * D + F) + 2 * L * L)                         # dr4sr_sasrec_layer_packed_saved_floats for a supported shape


def _packed_args(what, x, seqlen, ws_, n_head, backward, extra=()):
    """(B, L, D, H, F, saved floats, workspace bytes) of a sasrec_layer_packed call; every refusal (device, dtype, contiguity, shape) is
    raised here, before a launch.  Nothing is converted or copied: the op takes the tensors as they are or not at all"""
    named = (("x", x),) + tuple(zip(_W_NAMES, ws_)) + tuple(extra)
    _need_cuda(seqlen, *[t for _, t in named])
    for name, t in named:
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != x.device:
            raise _lib.Dr4srError(f"{what}: {name} must be a contiguous float32 tensor on x's device")
    if x.dim() != 3:
        raise _lib.Dr4srError(f"{what}: x must be [B, L, D]")
    B, L, D = (int(v) for v in x.shape)
    if seqlen.dtype != torch.int64 or seqlen.dim() != 1 or seqlen.shape[0] != B or not seqlen.is_contiguous() or seqlen.device != x.device:
        raise _lib.Dr4srError(f"{what}: seqlen must be a contiguous int64 tensor [B] = [{B}] on x's device")
    H, F = int(n_head), int(ws_[4].shape[0]) if ws_[4].dim() == 2 else 0
    shapes = ((3 * D, D), (3 * D,), (D, D), (D,), (F, D), (F,), (D, F), (D,), (D,), (D,), (D,), (D,))
    for name, t, shp in zip(_W_NAMES, ws_, shapes):
        if tuple(t.shape) != shp:
            raise _lib.Dr4srError(f"{what}: {name} must be {shp} for x [B, L, {D}], got {tuple(t.shape)}")
    lib = _lib.load()
    n = int(lib.dr4sr_sasrec_layer_packed_saved_floats(B, L, D, H, F))          # the shape refusals (DR4SR_E_SHAPE)
    _lib.check(min(n, 0), "dr4sr_sasrec_layer_packed_saved_floats")
    nb = int(lib.dr4sr_sasrec_layer_packed_workspace_bytes(B, L, D, H, F, backward))
    _lib.check(min(nb, 0), "dr4sr_sasrec_layer_packed_workspace_bytes")
    return B, L, D, H, F, n, nb


@torch.library.custom_op(f"{NS}::sasrec_layer_packed", mutates_args=())
def sasrec_layer_packed(x: torch.Tensor, seqlen: torch.Tensor, causal: bool, in_proj_weight: torch.Tensor, in_proj_bias: torch.Tensor,
                        out_proj_weight: torch.Tensor, out_proj_bias: torch.Tensor, linear1_weight: torch.Tensor,
                        linear1_bias: torch.Tensor, linear2_weight: torch.Tensor, linear2_bias: torch.Tensor, norm1_weight: torch.Tensor,
                        norm1_bias: torch.Tensor, norm2_weight: torch.Tensor, norm2_bias: torch.Tensor, n_head: int, eps: float,
                        p_drop: float, seed: int, step: int, layer: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """sasrec_layer on post-padded rows: sequence b has clamp(seqlen[b], 0, L) valid positions from 0, its keys behind them are padded;
    y is exactly 0 there and x there is never read.  Short sequences share a 64-row tile (csrc/layer_packed.hip); the dropout masks are
    sasrec_layer's.  `saved` is the opaque buffer the backward reads"""
    ws_ = (in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias, linear1_weight, linear1_bias, linear2_weight, linear2_bias,
           norm1_weight, norm1_bias, norm2_weight, norm2_bias)
    B, L, D, H, F, n, nb = _packed_args("sasrec_layer_packed", x, seqlen, ws_, n_head, 0)
    lib = _lib.load()
    y = torch.empty_like(x)
    saved = torch.empty(max(n, 1), dtype=torch.float32, device=x.device)
    ws = torch.empty(max(nb // 4, 1), dtype=torch.int32, device=x.device)
    w = _layer_struct(_lib.LayerWeights, ws_)
    _lib.check(lib.dr4sr_sasrec_layer_packed_fwd(_lib.ptr(x), _lib.ptr(seqlen), int(causal), w, B, L, D, H, F, eps, p_drop,
                                                 seed & 0xFFFFFFFFFFFFFFFF, step & 0xFFFFFFFF, layer, _lib.ptr(y), _lib.ptr(saved),
                                                 _lib.ptr(ws), nb, _lib.cur_stream()), "dr4sr_sasrec_layer_packed_fwd")
    return y, saved


@sasrec_layer_packed.register_fake
def _(x, seqlen, causal, in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias, linear1_weight, linear1_bias, linear2_weight,
      linear2_bias, norm1_weight, norm1_bias, norm2_weight, norm2_bias, n_head, eps, p_drop, seed, step, layer):
    B, L, D = x.shape
    return torch.empty_like(x), x.new_empty(max(_packed_saved_floats(B, L, D, linear1_weight.shape[0]), 1))


@torch.library.custom_op(f"{NS}::sasrec_layer_packed_backward", mutates_args=())
def sasrec_layer_packed_backward(x: torch.Tensor, seqlen: torch.Tensor, causal: bool, in_proj_weight: torch.Tensor,
                                 in_proj_bias: torch.Tensor, out_proj_weight: torch.Tensor, out_proj_bias: torch.Tensor,
                                 linear1_weight: torch.Tensor, linear1_bias: torch.Tensor, linear2_weight: torch.Tensor,
                                 linear2_bias: torch.Tensor, norm1_weight: torch.Tensor, norm1_bias: torch.Tensor,
                                 norm2_weight: torch.Tensor, norm2_bias: torch.Tensor, n_head: int, eps: float, p_drop: float, seed: int,
                                 step: int, layer: int, saved: torch.Tensor, dy: torch.Tensor) -> List[torch.Tensor]:
    """-> [dx, the 12 weight gradients in the argument order]; written, not accumulated; bit-reproducible.  dx is exactly 0 at and
    behind each length, dy there is never read"""
    ws_ = (in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias, linear1_weight, linear1_bias, linear2_weight, linear2_bias,
           norm1_weight, norm1_bias, norm2_weight, norm2_bias)
    B, L, D, H, F, n, nb = _packed_args("sasrec_layer_packed_backward", x, seqlen, ws_, n_head, 1, (("saved", saved), ("dy", dy)))
    if dy.shape != x.shape or saved.numel() < n:
        raise _lib.Dr4srError("sasrec_layer_packed_backward: dy must be [B, L, D], saved the forward's")
    lib = _lib.load()
    dx = torch.empty_like(x)
    dws = [torch.empty_like(t) for t in ws_]
    ws = torch.empty(max(nb // 4, 1), dtype=torch.int32, device=x.device)
    w, g = _layer_struct(_lib.LayerWeights, ws_), _layer_struct(_lib.LayerGrads, dws)
    _lib.check(lib.dr4sr_sasrec_layer_packed_bwd(_lib.ptr(x), _lib.ptr(seqlen), int(causal), w, B, L, D, H, F, eps, p_drop,
                                                 seed & 0xFFFFFFFFFFFFFFFF, step & 0xFFFFFFFF, layer, _lib.ptr(saved), _lib.ptr(dy),
                                                 _lib.ptr(dx), g, _lib.ptr(ws), nb, _lib.cur_stream()), "dr4sr_sasrec_layer_packed_bwd")
    return [dx] + dws


@sasrec_layer_packed_backward.register_fake
def _(x, seqlen, causal, in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias, linear1_weight, linear1_bias, linear2_weight,
      linear2_bias, norm1_weight, norm1_bias, norm2_weight, norm2_bias, n_head, eps, p_drop, seed, step, layer, saved, dy):
    return [torch.empty_like(t) for t in (x, in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias, linear1_weight, linear1_bias,
                                          linear2_weight, linear2_bias, norm1_weight, norm1_bias, norm2_weight, norm2_bias)]


def _packed_setup(ctx, inputs, output):
    ctx.rest = inputs[2:3] + inputs[15:]                    # causal, n_head, eps, p_drop, seed, step, layer
    ctx.save_for_backward(*inputs[:2], *inputs[3:15], output[1])
    ctx.mark_non_differentiable(output[1])


def _packed_backward(ctx, g_y, g_saved):
    x, seqlen, *w, saved = ctx.saved_tensors
    out = sasrec_layer_packed_backward(x, seqlen, ctx.rest[0], *w, *ctx.rest[1:], saved, g_y.contiguous())
    return (out[0], None, None, *out[1:], None, None, None, None, None, None)


sasrec_layer_packed.register_autograd(_packed_backward, setup_context=_packed_setup)


def _pool_shape(x, pooling):
    return x.shape if pooling == _lib.POOL_ORIGIN else (x.shape[0], x.shape[2])


@torch.library.custom_op(f"{NS}::seq_pool", mutates_args=())
def seq_pool(x: torch.Tensor, seqlen: torch.Tensor, pooling: int) -> torch.Tensor:
    """SeqPoolingLayer on x [B, L, D]: pooling = POOL_ORIGIN (1, zero rows >= seqlen -> [B, L, D]), POOL_LAST (2, row seqlen - 1 -> [B, D])
    or POOL_MEAN (3, mean of the rows < seqlen -> [B, D]); a row with seqlen 0 pools to zeros"""
    _need_cuda(x, seqlen)
    lib = _lib.load()
    B, L, D = (int(s) for s in x.shape)
    xc, sl = x.contiguous().float(), seqlen.contiguous().view(-1).to(torch.int64)
    out = torch.empty(_pool_shape(xc, pooling), dtype=torch.float32, device=x.device)
    _lib.check(lib.dr4sr_seq_pool_fwd(_lib.ptr(xc), _lib.ptr(sl), pooling, B, L, D, _lib.ptr(out), _lib.cur_stream()), "dr4sr_seq_pool_fwd")
    return out


@seq_pool.register_fake
def _(x, seqlen, pooling):
    return x.new_empty(_pool_shape(x, pooling))


@torch.library.custom_op(f"{NS}::seq_pool_backward", mutates_args=())
def seq_pool_backward(g_out: torch.Tensor, seqlen: torch.Tensor, pooling: int, L: int) -> torch.Tensor:
    _need_cuda(g_out, seqlen)
    lib = _lib.load()
    B, D = int(g_out.shape[0]), int(g_out.shape[-1])
    g, sl = g_out.contiguous().float(), seqlen.contiguous().view(-1).to(torch.int64)
    dx = torch.empty(B, L, D, dtype=torch.float32, device=g.device)
    _lib.check(lib.dr4sr_seq_pool_bwd(_lib.ptr(g), _lib.ptr(sl), pooling, B, L, D, _lib.ptr(dx), _lib.cur_stream()), "dr4sr_seq_pool_bwd")
    return dx


@seq_pool_backward.register_fake
def _(g_out, seqlen, pooling, L):
    return g_out.new_empty(g_out.shape[0], L, g_out.shape[-1])


def _pool_setup(ctx, inputs, output):
    x, seqlen, pooling = inputs
    ctx.pooling, ctx.L = pooling, x.shape[1]
    ctx.save_for_backward(seqlen)


def _pool_backward(ctx, g):
    return seq_pool_backward(g, ctx.saved_tensors[0], ctx.pooling, ctx.L), None, None


seq_pool.register_autograd(_pool_backward, setup_context=_pool_setup)


@torch.library.custom_op(f"{NS}::dropout", mutates_args=())
def dropout(x: torch.Tensor, p_drop: float, seed: int, step: int, site: int) -> torch.Tensor:
    """x * keep / (1 - p) with the library's Philox decisions of stream (seed, step, site), element order = x's memory order (the embedding
    dropout of a model written on the ops: site SITE_EMB); numel a multiple of 4.  Its backward is the same op on the gradient"""
    _need_cuda(x)
    lib = _lib.load()
    xc = x.contiguous().float()
    out = torch.empty_like(xc)
    _lib.check(lib.dr4sr_dropout_apply(_lib.ptr(xc), xc.numel(), p_drop, seed & 0xFFFFFFFFFFFFFFFF, step & 0xFFFFFFFF, site, _lib.ptr(out),
                                       _lib.cur_stream()), "dr4sr_dropout_apply")
    return out


@dropout.register_fake
def _(x, p_drop, seed, step, site):
    return torch.empty_like(x)


def _drop_setup(ctx, inputs, output):
    ctx.rest = inputs[1:]


def _drop_backward(ctx, g):
    return dropout(g, *ctx.rest), None, None, None, None


dropout.register_autograd(_drop_backward, setup_context=_drop_setup)


# ------------------------------------------------------------------------------------------------ FMLP layer / LayerNorm
def _fmlp_dims(x, complex_weight, dense_1_weight):
    if x.dim() != 3 or x.dtype != torch.float32:
        raise _lib.Dr4srError("fmlp_layer: x must be a [B, L, D] float32 tensor")
    B, L, D = (int(s) for s in x.shape)
    F = int(dense_1_weight.shape[0])
    n = int(_lib.load().dr4sr_fmlp_layer_saved_floats(B, L, D, F))          # the shape refusals (DR4SR_E_SHAPE), before any launch
    _lib.check(min(n, 0), "dr4sr_fmlp_layer_saved_floats")
    if tuple(complex_weight.shape) != (1, L // 2 + 1, D, 2):
        raise _lib.Dr4srError(f"fmlp_layer: complex_weight must be [1, L/2 + 1, D, 2] = {(1, L // 2 + 1, D, 2)}, got {tuple(complex_weight.shape)}")
    return B, L, D, F, n


def _fmlp_ws(lib, B, L, D, F, backward, device):
    nb = int(lib.dr4sr_fmlp_layer_workspace_bytes(B, L, D, F, backward))
    _lib.check(min(nb, 0), "dr4sr_fmlp_layer_workspace_bytes")
    return torch.empty(max(nb // 4, 1), dtype=torch.float32, device=device), nb


@torch.library.custom_op(f"{NS}::fmlp_layer", mutates_args=())
def fmlp_layer(x: torch.Tensor, complex_weight: torch.Tensor, filter_ln_weight: torch.Tensor, filter_ln_bias: torch.Tensor,
               dense_1_weight: torch.Tensor, dense_1_bias: torch.Tensor, dense_2_weight: torch.Tensor, dense_2_bias: torch.Tensor,
               inter_ln_weight: torch.Tensor, inter_ln_bias: torch.Tensor, eps: float, p_drop: float, seed: int, step: int,
               layer: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """one FMLP Layer (module/layers.py:781-791) on x [B, L, 64], L even and <= 64; complex_weight [1, L/2 + 1, 64, 2] as the reference
    holds it.  Dropout sites 1 + 2 layer (filter) and 2 + 2 layer (FFN) of stream (seed, step).  `saved` is the opaque buffer the backward
    reads"""
    ws_ = (complex_weight, filter_ln_weight, filter_ln_bias, dense_1_weight, dense_1_bias, dense_2_weight, dense_2_bias, inter_ln_weight,
           inter_ln_bias)
    _need_cuda(x, *ws_)
    lib = _lib.load()
    B, L, D, F, n = _fmlp_dims(x, complex_weight, dense_1_weight)
    xc = x.contiguous()
    wc = [t.contiguous() for t in ws_]
    y = torch.empty_like(xc)
    saved = torch.empty(max(n, 1), dtype=torch.float32, device=x.device)
    ws, nb = _fmlp_ws(lib, B, L, D, F, 0, x.device)
    w = _layer_struct(_lib.FmlpLayerWeights, wc)
    _lib.check(lib.dr4sr_fmlp_layer_fwd(_lib.ptr(xc), w, B, L, D, F, eps, p_drop, seed & 0xFFFFFFFFFFFFFFFF, step & 0xFFFFFFFF, layer,
                                        _lib.ptr(y), _lib.ptr(saved), _lib.ptr(ws), nb, _lib.cur_stream()), "dr4sr_fmlp_layer_fwd")
    return y, saved


@fmlp_layer.register_fake
def _(x, complex_weight, filter_ln_weight, filter_ln_bias, dense_1_weight, dense_1_bias, dense_2_weight, dense_2_bias, inter_ln_weight,
      inter_ln_bias, eps, p_drop, seed, step, layer):
    B, L, D = x.shape
    return torch.empty_like(x), x.new_empty(max(B * L * (2 * D + dense_1_weight.shape[0]), 1))


@torch.library.custom_op(f"{NS}::fmlp_layer_backward", mutates_args=())
def fmlp_layer_backward(x: torch.Tensor, complex_weight: torch.Tensor, filter_ln_weight: torch.Tensor, filter_ln_bias: torch.Tensor,
                        dense_1_weight: torch.Tensor, dense_1_bias: torch.Tensor, dense_2_weight: torch.Tensor, dense_2_bias: torch.Tensor,
                        inter_ln_weight: torch.Tensor, inter_ln_bias: torch.Tensor, eps: float, p_drop: float, seed: int, step: int,
                        layer: int, saved: torch.Tensor, dy: torch.Tensor) -> List[torch.Tensor]:
    """-> [dx, the 9 weight gradients in the argument order]; written, not accumulated; bit-reproducible"""
    ws_ = (complex_weight, filter_ln_weight, filter_ln_bias, dense_1_weight, dense_1_bias, dense_2_weight, dense_2_bias, inter_ln_weight,
           inter_ln_bias)
    _need_cuda(x, saved, dy, *ws_)
    lib = _lib.load()
    B, L, D, F, _ = _fmlp_dims(x, complex_weight, dense_1_weight)
    xc, dyc, sc = x.contiguous(), dy.contiguous().float(), saved.contiguous()
    wc = [t.contiguous() for t in ws_]
    dx = torch.empty_like(xc)
    dws = [torch.empty_like(t) for t in wc]
    ws, nb = _fmlp_ws(lib, B, L, D, F, 1, x.device)
    w, g = _layer_struct(_lib.FmlpLayerWeights, wc), _layer_struct(_lib.FmlpLayerGrads, dws)
    _lib.check(lib.dr4sr_fmlp_layer_bwd(_lib.ptr(xc), w, B, L, D, F, eps, p_drop, seed & 0xFFFFFFFFFFFFFFFF, step & 0xFFFFFFFF, layer,
                                        _lib.ptr(sc), _lib.ptr(dyc), _lib.ptr(dx), g, _lib.ptr(ws), nb, _lib.cur_stream()),
               "dr4sr_fmlp_layer_bwd")
    return [dx] + dws


@fmlp_layer_backward.register_fake
def _(x, complex_weight, filter_ln_weight, filter_ln_bias, dense_1_weight, dense_1_bias, dense_2_weight, dense_2_bias, inter_ln_weight,
      inter_ln_bias, eps, p_drop, seed, step, layer, saved, dy):
    return [torch.empty_like(t) for t in (x, complex_weight, filter_ln_weight, filter_ln_bias, dense_1_weight, dense_1_bias, dense_2_weight,
                                          dense_2_bias, inter_ln_weight, inter_ln_bias)]


def _fmlp_setup(ctx, inputs, output):
    ctx.rest = inputs[10:]                                  # eps, p_drop, seed, step, layer
    ctx.save_for_backward(*inputs[:10], output[1])
    ctx.mark_non_differentiable(output[1])


def _fmlp_backward(ctx, g_y, g_saved):
    x, *w, saved = ctx.saved_tensors
    out = fmlp_layer_backward(x, *w, *ctx.rest, saved, g_y)
    return (*out, None, None, None, None, None)


fmlp_layer.register_autograd(_fmlp_backward, setup_context=_fmlp_setup)


def _ln_dims(x, weight):
    if x.dim() < 1 or x.dtype != torch.float32 or x.shape[-1] != weight.shape[0]:
        raise _lib.Dr4srError("layer_norm: x must be a float32 tensor whose last dimension is the weight's")
    D = int(x.shape[-1])
    return x.numel() // max(D, 1), D


@torch.library.custom_op(f"{NS}::layer_norm", mutates_args=())
def layer_norm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float) -> torch.Tensor:
    """torch.nn.LayerNorm over the last dimension (a multiple of 4 up to 1024): FMLP's embedding LayerNorm, model/fmlp.py:25"""
    _need_cuda(x, weight, bias)
    lib = _lib.load()
    n, D = _ln_dims(x, weight)
    xc = x.contiguous()
    y = torch.empty_like(xc)
    _lib.check(lib.dr4sr_layer_norm_fwd(_lib.ptr(xc), _lib.ptr(weight.contiguous()), _lib.ptr(bias.contiguous()), n, D, eps, _lib.ptr(y),
                                        _lib.cur_stream()), "dr4sr_layer_norm_fwd")
    return y


@layer_norm.register_fake
def _(x, weight, bias, eps):
    return torch.empty_like(x)


@torch.library.custom_op(f"{NS}::layer_norm_backward", mutates_args=())
def layer_norm_backward(x: torch.Tensor, weight: torch.Tensor, eps: float, dy: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (dx, d weight, d bias); written, not accumulated; bit-reproducible"""
    _need_cuda(x, weight, dy)
    lib = _lib.load()
    n, D = _ln_dims(x, weight)
    nb = int(lib.dr4sr_layer_norm_workspace_bytes(n, D))
    _lib.check(min(nb, 0), "dr4sr_layer_norm_workspace_bytes")
    xc, wc, dyc = x.contiguous(), weight.contiguous(), dy.contiguous().float()
    dx, dw, db = torch.empty_like(xc), torch.empty_like(wc), torch.empty_like(wc)
    ws = torch.empty(max(nb // 4, 1), dtype=torch.float32, device=x.device)
    _lib.check(lib.dr4sr_layer_norm_bwd(_lib.ptr(xc), _lib.ptr(wc), n, D, eps, _lib.ptr(dyc), _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(db),
                                        _lib.ptr(ws), nb, _lib.cur_stream()), "dr4sr_layer_norm_bwd")
    return dx, dw, db


@layer_norm_backward.register_fake
def _(x, weight, eps, dy):
    return torch.empty_like(x), torch.empty_like(weight), torch.empty_like(weight)


def _ln_setup(ctx, inputs, output):
    x, weight, _, eps = inputs
    ctx.eps = eps
    ctx.save_for_backward(x, weight)


def _ln_backward(ctx, g):
    x, weight = ctx.saved_tensors
    dx, dw, db = layer_norm_backward(x, weight, ctx.eps, g)
    return dx, dw, db, None


layer_norm.register_autograd(_ln_backward, setup_context=_ln_setup)


# ------------------------------------------------------------------------------------------------ GRU layer
def _gru_dims(x, weight_ih, weight_hh, seqlen, *more):
    """(B, L, I, H, saved floats) of a gru_layer call; every refusal (device, dtype, contiguity, shape) is raised here, before a launch"""
    _need_cuda(x, weight_ih, weight_hh, seqlen, *more)
    for name, t in (("x", x), ("weight_ih", weight_ih), ("weight_hh", weight_hh)) + tuple(("tensor", m) for m in more):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.Dr4srError(f"gru_layer: {name} must be a contiguous float32 tensor")
    if x.dim() != 3 or weight_ih.dim() != 2 or weight_hh.dim() != 2:
        raise _lib.Dr4srError("gru_layer: x must be [B, L, I], weight_ih [3H, I] and weight_hh [3H, H]")
    B, L, I = (int(s) for s in x.shape)
    H = int(weight_hh.shape[1])
    if tuple(weight_ih.shape) != (3 * H, I) or tuple(weight_hh.shape) != (3 * H, H):
        raise _lib.Dr4srError(f"gru_layer: weight_ih must be [3H, I] = {(3 * H, I)} and weight_hh [3H, H] = {(3 * H, H)}, got "
                              f"{tuple(weight_ih.shape)} and {tuple(weight_hh.shape)}")
    if seqlen is not None and (seqlen.dtype != torch.int64 or tuple(seqlen.shape) != (B,) or not seqlen.is_contiguous()):
        raise _lib.Dr4srError("gru_layer: seqlen must be a contiguous int64 tensor [B] (or None: every sequence has L steps)")
    n = int(_lib.load().dr4sr_gru_layer_saved_floats(B, L, I, H))          # the shape refusals (DR4SR_E_SHAPE)
    _lib.check(min(n, 0), "dr4sr_gru_layer_saved_floats")
    return B, L, I, H, n


def _gru_ws(lib, B, L, I, H, backward, device):
    nb = int(lib.dr4sr_gru_layer_workspace_bytes(B, L, I, H, backward))
    _lib.check(min(nb, 0), "dr4sr_gru_layer_workspace_bytes")
    return torch.empty(max(nb // 4, 1), dtype=torch.float32, device=device), nb


@torch.library.custom_op(f"{NS}::gru_layer", mutates_args=())
def gru_layer(x: torch.Tensor, weight_ih: torch.Tensor, weight_hh: torch.Tensor,
              seqlen: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """one layer of torch.nn.GRU(bias=False, batch_first=True) (module/layers.py:117-136) on x [B, L, I], h_0 = 0: I in {64, 128, 256},
    H in {128, 256}, L <= 1024.  seqlen None computes every step (the reference); with seqlen [B] int64 the steps at and behind
    seqlen[b] are skipped and y is 0 there.  -> (y [B, L, H], saved: the opaque buffer the backward reads)"""
    B, L, I, H, n = _gru_dims(x, weight_ih, weight_hh, seqlen)
    lib = _lib.load()
    y = torch.empty(B, L, H, dtype=torch.float32, device=x.device)
    saved = torch.empty(max(n, 1), dtype=torch.float32, device=x.device)
    ws, nb = _gru_ws(lib, B, L, I, H, 0, x.device)
    _lib.check(lib.dr4sr_gru_layer_fwd(_lib.ptr(x), _lib.ptr(weight_ih), _lib.ptr(weight_hh), _lib.ptr(seqlen), B, L, I, H, _lib.ptr(y),
                                       _lib.ptr(saved), _lib.ptr(ws), nb, _lib.cur_stream()), "dr4sr_gru_layer_fwd")
    return y, saved


@gru_layer.register_fake
def _(x, weight_ih, weight_hh, seqlen):
    B, L, _ = x.shape
    H = weight_hh.shape[1]
    return x.new_empty(B, L, H), x.new_empty(max(B * L * 4 * H, 1))


@torch.library.custom_op(f"{NS}::gru_layer_backward", mutates_args=())
def gru_layer_backward(x: torch.Tensor, weight_ih: torch.Tensor, weight_hh: torch.Tensor, seqlen: Optional[torch.Tensor], y: torch.Tensor,
                       saved: torch.Tensor, dy: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (dx, d weight_ih, d weight_hh); written, not accumulated; bit-reproducible.  dy behind seqlen is not read"""
    dyc = dy.contiguous().float()
    B, L, I, H, n = _gru_dims(x, weight_ih, weight_hh, seqlen, y, saved, dyc)
    if tuple(y.shape) != (B, L, H) or tuple(dyc.shape) != (B, L, H) or saved.numel() < n:
        raise _lib.Dr4srError("gru_layer_backward: y and dy must be [B, L, H], saved the forward's")
    lib = _lib.load()
    dx, dw_ih, dw_hh = torch.empty_like(x), torch.empty_like(weight_ih), torch.empty_like(weight_hh)
    ws, nb = _gru_ws(lib, B, L, I, H, 1, x.device)
    _lib.check(lib.dr4sr_gru_layer_bwd(_lib.ptr(x), _lib.ptr(weight_ih), _lib.ptr(weight_hh), _lib.ptr(seqlen), B, L, I, H, _lib.ptr(y),
                                       _lib.ptr(saved), _lib.ptr(dyc), _lib.ptr(dx), _lib.ptr(dw_ih), _lib.ptr(dw_hh), _lib.ptr(ws), nb,
                                       _lib.cur_stream()), "dr4sr_gru_layer_bwd")
    return dx, dw_ih, dw_hh


@gru_layer_backward.register_fake
def _(x, weight_ih, weight_hh, seqlen, y, saved, dy):
    return torch.empty_like(x), torch.empty_like(weight_ih), torch.empty_like(weight_hh)


def _gru_setup(ctx, inputs, output):
    x, weight_ih, weight_hh, seqlen = inputs
    ctx.has_seqlen = seqlen is not None
    ctx.save_for_backward(x, weight_ih, weight_hh, *([seqlen] if ctx.has_seqlen else []), output[0], output[1])
    ctx.mark_non_differentiable(output[1])


def _gru_backward(ctx, g_y, g_saved):
    x, weight_ih, weight_hh, *rest = ctx.saved_tensors
    seqlen = rest[0] if ctx.has_seqlen else None
    y, saved = rest[-2:]
    dx, dw_ih, dw_hh = gru_layer_backward(x, weight_ih, weight_hh, seqlen, y, saved, g_y)
    return dx, dw_ih, dw_hh, None


gru_layer.register_autograd(_gru_backward, setup_context=_gru_setup)


OPS = ("embed_gather_posadd", "score_bce", "score_bce_backward", "score_bpr", "score_bpr_backward", "loss_from_scores",
       "loss_from_scores_backward", "neg_sample", "full_score_topk", "target_rank", "fused_adam_",
       "sasrec_layer", "sasrec_layer_backward", "sasrec_layer_packed", "sasrec_layer_packed_backward", "seq_pool", "seq_pool_backward",
       "dropout", "embed_gather_posadd_backward",
       "fmlp_layer", "fmlp_layer_backward", "layer_norm", "layer_norm_backward", "gru_layer", "gru_layer_backward")
