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
reference never reads such a position.

use_seqlen=True (default False: the path above, bit for bit) runs the layers of the id path as torch.ops.dr4sr_hip.sasrec_layer_packed
(csrc/layer_packed.hip) on batch['seqlen']: short sequences share a 64-row tile, so the work goes with the valid tokens, and the rows at
and behind each length come out as zeros instead of the dense op's values there.  Nothing that the poolings read changes (the dropout
masks are the same).  ONE requirement: the ids are non-zero exactly at pos < seqlen — post-padded rows, which is what the project's and
the reference's SASRec datasets deliver.  The module checks it per batch, one device reduction and one host read beside the id check
embed_gather_posadd already makes, and under the same two exemptions (inside a stream capture, under DR4SR_NO_ID_CHECK), where it is
the caller's to keep.  A batch that does not meet it (an id 0 in front of a length: the reference masks that key, sasrec_layer_packed
has no way to) runs the dense op: the flag never changes what the module computes, only how.  The `seq_emb` path keeps the dense op
whatever the flag says.

FMLPEncoderOps / FMLPOps — the reference's FMLPEncoder (module/layers.py:740-808) and the encoder half of its FMLP model (model/fmlp.py:8-39)
written the same way: each `Layer` (FilterLayer + Intermediate) is one torch.ops.dr4sr_hip.fmlp_layer (csrc/fmlp_op.hip), the embedding
LayerNorm torch.ops.dr4sr_hip.layer_norm.  Parameters carry the reference's names, so a checkpoint of the engine-backed FMLP loads with
strict=True (its `item_embedding.weight` is the table the module is handed).  The dropout sites are the FMLP engine's: 0 for the
embedding, 1 + 2 l and 2 + 2 l for layer l; the step counter works as above.

GRULayerOps / GRU4RecQueryEncoderOps — the reference's GRULayer (module/layers.py:117-136) and the query encoder of its GRU4Rec
(model/gru4rec.py:12-34) written the same way: every GRU layer is one torch.ops.dr4sr_hip.gru_layer (csrc/gru_op.hip).  The op takes an
optional `seqlen`: without it every one of the L steps is computed, as torch.nn.GRU does on the padded batch; with it the steps behind
each length are skipped and come out as zeros, which changes nothing that 'origin' or 'last' pooling reads.  The H -> D projection
behind the GRU is the reference's own nn.Linear outside GRULayer and stays torch's (F.linear)."""
from __future__ import annotations

import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

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
                 bidirectional=False, training_pooling_type="origin", eval_pooling_type="last", seed: int = 2023,
                 use_seqlen: bool = False) -> None:
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
        self.use_seqlen = bool(use_seqlen)

    @staticmethod
    def _post_padded(idx, seqlen):
        """are the ids non-zero exactly at pos < seqlen?  (what sasrec_layer_packed's key mask assumes; not looked at where
        embed_gather_posadd does not look at the ids either)"""
        if torch.cuda.is_current_stream_capturing() or os.environ.get("DR4SR_NO_ID_CHECK"):
            return True
        L = idx.shape[1]
        valid = torch.arange(L, device=idx.device).view(1, L) < seqlen.clamp(0, L).view(-1, 1)
        return bool(((idx != 0) == valid).all())

    def forward(self, batch, need_pooling=True):
        o = torch.ops.dr4sr_hip
        p = self.p_drop if self.training else 0.0
        packed = self.use_seqlen and batch.get("seq_emb", None) is None      # seq_emb: no padding mask, every position is a key
        if packed:
            packed = self._post_padded(batch["in_" + self.fiid], batch["seqlen"])
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
            if packed:
                x, _ = o.sasrec_layer_packed(x.contiguous(), batch["seqlen"], not self.bidirectional, *layer.tensors(), self.n_head,
                                             self.eps, p, seed, step, i)
            else:
                x, _ = o.sasrec_layer(x, key_pad, not self.bidirectional, *layer.tensors(), self.n_head, self.eps, p, seed, step, i)
        if self.training:
            self.step += 1
        if not need_pooling:
            return x
        kind = self.training_pooling_type if self.training else self.eval_pooling_type
        return o.seq_pool(x, batch["seqlen"], _POOLING[kind])


class _FilterLayer(nn.Module):
    """FilterLayer's parameters (module/layers.py:740-745): complex_weight [1, L/2 + 1, D, 2] = randn * 0.02, LayerNorm"""
    def __init__(self, L, D):
        super().__init__()
        self.complex_weight = nn.Parameter(torch.randn(1, L // 2 + 1, D, 2, dtype=torch.float32) * 0.02)
        self.LayerNorm = nn.LayerNorm(D, eps=1e-12)


class _Intermediate(nn.Module):
    """Intermediate's parameters (module/layers.py:761-769)"""
    def __init__(self, D):
        super().__init__()
        self.dense_1 = nn.Linear(D, 4 * D)
        self.dense_2 = nn.Linear(4 * D, D)
        self.LayerNorm = nn.LayerNorm(D, eps=1e-12)


class _FMLPLayer(nn.Module):
    def __init__(self, L, D):
        super().__init__()
        self.filterlayer = _FilterLayer(L, D)
        self.intermediate = _Intermediate(D)

    def tensors(self):
        """the 9 tensors in the flat layout's order (include/dr4sr_hip.h dr4sr_fmlp_layer_weights)"""
        f, i = self.filterlayer, self.intermediate
        return (f.complex_weight, f.LayerNorm.weight, f.LayerNorm.bias, i.dense_1.weight, i.dense_1.bias, i.dense_2.weight, i.dense_2.bias,
                i.LayerNorm.weight, i.LayerNorm.bias)


class FMLPEncoderOps(nn.Module):
    """FMLPEncoder (module/layers.py:793-808): `num_hidden_layers` copies of ONE initialised Layer, as copy.deepcopy gives the reference.
    The reference hard-codes 50 positions, 64 features, dropout 0.5 and eps 1e-12; they are keyword arguments here.  p_drop applies in
    train mode only; seed / step key the masks and are set by the owner (FMLPOps) or the caller"""
    def __init__(self, num_hidden_layers=2, max_seq_len=50, hidden_size=64, dropout=0.5, layer_norm_eps=1e-12, seed: int = 2023) -> None:
        super().__init__()
        first = _FMLPLayer(max_seq_len, hidden_size)
        self.layer = nn.ModuleList([first] + [_FMLPLayer(max_seq_len, hidden_size) for _ in range(num_hidden_layers - 1)])
        for other in self.layer[1:]:
            other.load_state_dict(first.state_dict())
        self.p_drop, self.eps = float(dropout), float(layer_norm_eps)
        self.seed, self.step = int(seed), 0

    def forward(self, hidden_states, output_all_encoded_layers=True):
        p = self.p_drop if self.training else 0.0
        all_encoder_layers = []
        for i, layer in enumerate(self.layer):
            hidden_states, _ = torch.ops.dr4sr_hip.fmlp_layer(hidden_states, *layer.tensors(), self.eps, p, self.seed, self.step, i)
            if output_all_encoded_layers:
                all_encoder_layers.append(hidden_states)
        if not output_all_encoded_layers:
            all_encoder_layers.append(hidden_states)
        return all_encoder_layers


class FMLPOps(nn.Module):
    """the encoder of the reference's FMLP (model/fmlp.py:8-39) on `item_embedding` (an nn.Embedding the caller owns): position_embeddings,
    LayerNorm and item_encoder under the reference's names; forward(batch) is fmlp.py:30-39, the query x[:, -1] (need_pooling=False returns
    the last layer's [B, L, D])"""
    def __init__(self, item_embedding, n_layer, max_seq_len=50, dropout=0.5, layer_norm_eps=1e-12, seed: int = 2023, fiid="item_id") -> None:
        super().__init__()
        D = item_embedding.weight.shape[1]
        self.fiid = fiid
        self.item_embedding = item_embedding
        self.position_embeddings = nn.Embedding(max_seq_len, D)
        self.LayerNorm = nn.LayerNorm(D, eps=layer_norm_eps)
        self.item_encoder = FMLPEncoderOps(n_layer, max_seq_len, D, dropout, layer_norm_eps, seed)
        self.p_drop, self.eps = float(dropout), float(layer_norm_eps)
        self.seed, self.step = int(seed), 0

    def forward(self, batch, need_pooling=True):
        o = torch.ops.dr4sr_hip
        p = self.p_drop if self.training else 0.0
        x = o.embed_gather_posadd(self.item_embedding.weight, self.position_embeddings.weight, batch["in_" + self.fiid])     # fmlp.py:18-24
        x = o.layer_norm(x, self.LayerNorm.weight, self.LayerNorm.bias, self.eps)                                            # fmlp.py:25
        if p > 0.0:                                                                                                          # fmlp.py:26
            x = o.dropout(x, p, self.seed, self.step, _lib.SITE_EMB)
        self.item_encoder.seed, self.item_encoder.step = self.seed, self.step
        x = self.item_encoder(x, output_all_encoded_layers=True)[-1]
        if self.training:
            self.step += 1
        return x[:, -1] if need_pooling else x


class _GRUWeights(nn.Module):
    """the parameters of torch.nn.GRU(bias=False), same names, same shapes, same initialisation (uniform in +-1 / sqrt(hidden))"""
    def __init__(self, input_dim, hidden, num_layer):
        super().__init__()
        k = 1.0 / math.sqrt(hidden)
        for l in range(num_layer):
            self.register_parameter(f"weight_ih_l{l}", nn.Parameter(torch.empty(3 * hidden, input_dim if l == 0 else hidden).uniform_(-k, k)))
            self.register_parameter(f"weight_hh_l{l}", nn.Parameter(torch.empty(3 * hidden, hidden).uniform_(-k, k)))


class GRULayerOps(nn.Module):
    """GRULayer (module/layers.py:117-136): `num_layer` GRU layers without biases, h_0 = 0, on input [B, L, input_dim].
    forward(input, seqlen=None) -> out [B, L, output_dim], or (out, hidden [num_layer, B, output_dim]) with return_hidden, hidden being each
    layer's output at its last computed step (L - 1 without seqlen, seqlen - 1 with it; zeros for an empty sequence)"""
    def __init__(self, input_dim, output_dim, num_layer=1, bias=False, batch_first=True, bidirectional=False, return_hidden=False) -> None:
        super().__init__()
        for given, name in ((bias, "bias=True"), (not batch_first, "batch_first=False"), (bidirectional, "bidirectional=True")):
            if given:
                raise NotImplementedError(f"{name}: torch.ops.dr4sr_hip.gru_layer computes a forward-direction GRU without biases on "
                                          "[B, L, I] input (bias=False, batch_first=True, bidirectional=False)")
        self.gru = _GRUWeights(input_dim, output_dim, num_layer)
        self.num_layer, self.return_hidden = int(num_layer), return_hidden

    def forward(self, input, seqlen=None):
        o = torch.ops.dr4sr_hip
        if seqlen is not None:
            seqlen = seqlen.contiguous().view(-1).to(torch.int64)
        x, hidden = input.contiguous(), []
        for l in range(self.num_layer):
            x, _ = o.gru_layer(x, getattr(self.gru, f"weight_ih_l{l}"), getattr(self.gru, f"weight_hh_l{l}"), seqlen)
            if self.return_hidden:
                hidden.append(x[:, -1] if seqlen is None else o.seq_pool(x, seqlen, _lib.POOL_LAST))
        return (x, torch.stack(hidden)) if self.return_hidden else x


class GRU4RecQueryEncoderOps(nn.Module):
    """the query encoder of the reference's GRU4Rec (model/gru4rec.py:12-34) on `item_embedding` (an nn.Embedding the caller owns).  The
    children carry the names the reference's VStackLayer(Sequential(Lambda, table, Dropout, GRULayer), Linear) gives them, so the
    state-dict keys are 0.1.weight, 0.3.gru.weight_{ih,hh}_l{k}, 1.weight and 1.bias: a GRU4Rec checkpoint loads with the `query_encoder.`
    prefix stripped.  use_seqlen hands batch['seqlen'] to the GRU layers (the pads are skipped); False computes them as the reference does"""
    def __init__(self, fiid, item_embedding, hidden_size, layer_num, dropout, max_seq_len, seed: int = 2023, use_seqlen: bool = True) -> None:
        super().__init__()
        D = item_embedding.weight.shape[1]
        self.fiid, self.p_drop, self.use_seqlen = fiid, float(dropout), bool(use_seqlen)
        self.add_module("0", nn.ModuleDict({"1": item_embedding, "3": GRULayerOps(D, hidden_size, layer_num)}))
        self.add_module("1", nn.Linear(hidden_size, D))
        # E[idx] + 0 is the gather: embed_gather_posadd with a zero position table keeps the table scatter of the backward in HIP
        self.register_buffer("zero_pos", torch.zeros(max_seq_len, D), persistent=False)
        self.seed, self.step = int(seed), 0

    def forward(self, batch, need_pooling=True):
        o = torch.ops.dr4sr_hip
        inner, proj = self._modules["0"], self._modules["1"]
        p = self.p_drop if self.training else 0.0
        x = o.embed_gather_posadd(inner["1"].weight, self.zero_pos, batch["in_" + self.fiid])     # gru4rec.py:15-16
        if p > 0.0:                                                                                # gru4rec.py:17
            x = o.dropout(x, p, self.seed, self.step, _lib.SITE_EMB)
        x = inner["3"](x, batch["seqlen"] if self.use_seqlen else None)                            # gru4rec.py:18
        x = F.linear(x, proj.weight, proj.bias)                                                    # gru4rec.py:20 (torch's own)
        if self.training:
            self.step += 1
        if not need_pooling:
            return x
        return o.seq_pool(x, batch["seqlen"], _lib.POOL_ORIGIN if self.training else _lib.POOL_LAST)   # gru4rec.py:28-32
