"""SASRecQueryEncoderOps — the reference's SASRecQueryEncoder (model/sasrec.py:10-75) written on torch.ops.dr4sr_hip.* and plain torch.

What a reference-side user gets by binding the op library instead of the engines: the constructor arguments of the reference (with
`bidirectional`), plain nn.Parameters under the reference's state-dict names — a checkpoint of the engine-backed SASRec loads with the
`query_encoder.` prefix stripped —, the id path and the `seq_emb` path of forward, autograd through every op.  The two
TransformerEncoderLayer calls are torch.ops.dr4sr_hip.sasrec_layer (csrc/layer_op.hip), which computes all L positions of every sequence;
the engine-backed models (dr4sr_amd/model/*) pack the valid tokens and stay the fast path.  This class is registered nowhere in
get_model_class.

Dropout runs through the library's Philox masks, keyed by (seed, step, site): the embedding dropout (model/sasrec.py:66) is the tiny op
torch.ops.dr4sr_hip.dropout at DR4SR_SITE_EMB, the layers draw their four sites themselves.  `step` is an explicit counter: every
training forward uses self.step and then advances it by one, so two forwards never share masks and a run is reproducible from (seed,
step).  A query position with no admissible key (a padded row on the id path) gets a zero attention context where torch yields NaN; the
reference never reads such a position."""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import _lib
from .. import ops  # noqa: F401  (registers torch.ops.dr4sr_hip.*)

_POOLING = {"origin": _lib.POOL_ORIGIN, "last": _lib.POOL_LAST, "mean": _lib.POOL_MEAN}


class _Affine(nn.Module):
    """weight and bias under the names nn.Linear / nn.LayerNorm give them"""
    def __init__(self, *shape, ones=False):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(*shape) if ones else torch.empty(*shape))
        self.bias = nn.Parameter(torch.zeros(shape[0]))
        if not ones:
            nn.init.xavier_uniform_(self.weight)


class _SelfAttn(nn.Module):
    def __init__(self, D):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * D, D))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * D))
        self.out_proj = _Affine(D, D)
        nn.init.xavier_uniform_(self.in_proj_weight)


class _Layer(nn.Module):
    """the parameters of one torch.nn.TransformerEncoderLayer, same names, same shapes"""
    def __init__(self, D, F):
        super().__init__()
        self.self_attn = _SelfAttn(D)
        self.linear1 = _Affine(F, D)
        self.linear2 = _Affine(D, F)
        self.norm1 = _Affine(D, ones=True)
        self.norm2 = _Affine(D, ones=True)

    def tensors(self):
        """the 12 tensors in the flat layout's order (include/dr4sr_hip.h dr4sr_layer_weights)"""
        a = self.self_attn
        return (a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias, self.linear1.weight, self.linear1.bias,
                self.linear2.weight, self.linear2.bias, self.norm1.weight, self.norm1.bias, self.norm2.weight, self.norm2.bias)


class _Stack(nn.Module):
    def __init__(self, D, F, n_layer):
        super().__init__()
        self.layers = nn.ModuleList(_Layer(D, F) for _ in range(n_layer))


class SASRecQueryEncoderOps(nn.Module):
    def __init__(self, fiid, embed_dim, max_seq_len, n_head, hidden_size, dropout, activation, layer_norm_eps, n_layer, item_encoder,
                 bidirectional=False, training_pooling_type="origin", eval_pooling_type="last", seed: int = 2023) -> None:
        super().__init__()
        if activation != "gelu":
            raise NotImplementedError("torch.ops.dr4sr_hip.sasrec_layer computes the exact-erf GELU only (activation='gelu')")
        for t in (training_pooling_type, eval_pooling_type):
            if t not in _POOLING:
                raise NotImplementedError(f"pooling type {t!r}: torch.ops.dr4sr_hip.seq_pool has 'origin', 'last' and 'mean'")
        self.fiid = fiid
        self.item_encoder = item_encoder
        self.bidirectional = bool(bidirectional)
        self.training_pooling_type, self.eval_pooling_type = training_pooling_type, eval_pooling_type
        self.n_head, self.p_drop, self.eps = int(n_head), float(dropout), float(layer_norm_eps)
        self.position_emb = nn.Embedding(max_seq_len, embed_dim)
        self.transformer_layer = _Stack(embed_dim, hidden_size, n_layer)
        self.seed, self.step = int(seed), 0

    def forward(self, batch, need_pooling=True):
        o = torch.ops.dr4sr_hip
        p = self.p_drop if self.training else 0.0
        seed, step = self.seed, self.step
        if batch.get("seq_emb", None) is None:                                  # sasrec.py:42-48
            idx = batch["in_" + self.fiid]
            x = o.embed_gather_posadd(self.item_encoder.weight, self.position_emb.weight, idx)
            key_pad = idx == 0
        else:                                                                   # sasrec.py:50-54
            seq = batch["seq_emb"]
            x = seq + self.position_emb.weight[:seq.size(1)].unsqueeze(0)
            key_pad = None
        w = batch.get("input_weight", None)                                     # sasrec.py:61-64
        if w is not None:
            x = w * x
        if p > 0.0:                                                             # sasrec.py:66
            x = o.dropout(x, p, seed, step, _lib.SITE_EMB)
        for i, layer in enumerate(self.transformer_layer.layers):               # sasrec.py:65-68
            x, _ = o.sasrec_layer(x, key_pad, not self.bidirectional, *layer.tensors(), self.n_head, self.eps, p, seed, step, i)
        if self.training:
            self.step += 1
        if not need_pooling:
            return x
        kind = self.training_pooling_type if self.training else self.eval_pooling_type
        return o.seq_pool(x, batch["seqlen"], _POOLING[kind])
