"""GNN with the class surface of the reference's model/gnn.py (GNNQueryEncoder :12-75, GNN :77-177): SASRec over a LightGCN-style
smoothed item table.

  graph   built once at construction from the item sequences (build_graph): A = diag(1/deg) S + S diag(1/deg), S = M + M^T + I,
          M[a, b] = sum of 1/d over every pair (a, b) that sits d <= window positions apart in a sequence.  A is exactly symmetric.
  table   G = (E + A E + ... + A^gnn_layer E) / (gnn_layer + 1), recomputed from the current E in EVERY forward (train and eval):
          dr4sr_gnn_propagate (csrc/gnn.hip), one gather launch per hop
  encoder SASRec's, on G[in_item_id]: the model owns a SasrecEngine whose flat table slot holds G, so dr4sr_sasrec_encode / _encode_bwd run
          unchanged and dG lands in the table slot of the flat gradient
  scorer  negatives, loss, top-k: BaseModel's, against the RAW item_embedding.weight (E lives in a buffer of its own, with its own gradient
          and moments; `item_embedding.weight` and `query_encoder.item_encoder.weight` are views of it)
  grads   dE = dE_scorer + (I + A + ... + A^k) dG / (k + 1): the same propagation call (A is symmetric), accumulating into E's gradient

Parameters and state-dict keys are SASRec's (G is not a parameter; the graph is a plain attribute, as in the reference).  Training runs
through BaseModel's API path (the fused step gathers and scores ONE table), captured as a HIP graph per batch size when train.hip_graph.
Not implemented (NotImplementedError): bidirectional attention, WORLD_SIZE > 1, GNN as a MetaModel sub_model.
"""
from __future__ import annotations

from collections import OrderedDict

import torch
import torch.nn as nn

from .. import _lib
from ..engine import SasrecEngine
from .basemodel import BaseModel
from .loss_func import BinaryCrossEntropyLoss
from .sasrec import _Embedding, _Encoder


def build_graph(in_item_id: torch.Tensor, seqlen: torch.Tensor, n_items: int, window: int, drop_last: bool):
    """CSR of the reference's norm_adj (model/gnn.py:102-171) -> (row_ptr int64 [n_items + 1], col int32 [nnz], val float32 [nnz]), on the
    device of in_item_id, every row's columns ascending.  in_item_id [rows, L] holds each row's items in its first seqlen positions;
    drop_last = the 'old' graph (validation rows, whose last item is the training target: seqlen - 1 items), else the 'new' one.
    Sums run in float64 and the result is cast to fp32, as the reference does; A is asserted symmetric (the backward relies on it)."""
    items = in_item_id.long()
    dev, L, N = items.device, int(items.shape[1]), int(n_items)
    n = (seqlen.long() - (1 if drop_last else 0)).clamp(0, L).view(-1, 1)
    pos = torch.arange(L, device=dev).view(1, -1)
    rows, cols, vals = [], [], []
    for d in range(1, min(int(window), L - 1) + 1):                 # (item[i], item[i + d]) with weight 1 / d while i + d < len
        m = pos[:, :L - d] + d < n
        a, b = items[:, :L - d][m], items[:, d:][m]
        w = torch.full((int(a.numel()),), 1.0 / d, dtype=torch.float64, device=dev)
        rows += [a, b]                                              # M and M^T
        cols += [b, a]
        vals += [w, w]
    eye = torch.arange(N, device=dev)
    rows.append(eye)
    cols.append(eye)
    vals.append(torch.ones(N, dtype=torch.float64, device=dev))
    S = torch.sparse_coo_tensor(torch.stack([torch.cat(rows), torch.cat(cols)]), torch.cat(vals), (N, N)).coalesce()
    r, c = S.indices()
    s = S.values()
    deg = torch.bincount(r, minlength=N)                            # non-zeros per row of S (the self loop makes it >= 1)
    inv = 1.0 / deg.to(torch.float64)
    val = (s * inv[r] + s * inv[c]).to(torch.float32)
    row_ptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    row_ptr[1:] = torch.cumsum(deg, 0)
    At = torch.sparse_coo_tensor(torch.stack([c, r]), val, (N, N)).coalesce()
    assert torch.equal(At.indices(), S.indices()) and torch.equal(At.values(), val), "GNN graph: the normalised adjacency is not symmetric"
    return row_ptr, c.to(torch.int32).contiguous(), val.contiguous()


class _GnnEngine:
    """What BaseModel and the parameter holders see as `model.engine`: the SasrecEngine whose table slot holds G, with
    views / grad_views['item_embedding.weight'] mapped to the RAW table's buffers (the scorer's backward writes there)."""

    def __init__(self, inner: SasrecEngine):
        self.inner = inner
        N, D, dev = inner.n_items, inner.D, inner.device
        self.raw = torch.zeros(N * D, dtype=torch.float32, device=dev)
        self.raw_grad = torch.zeros(N * D + _lib.GRAD_TAIL, dtype=torch.float32, device=dev)       # + the optimizer's tail
        self.raw_m = torch.zeros(N * D, dtype=torch.float32, device=dev)
        self.raw_v = torch.zeros(N * D, dtype=torch.float32, device=dev)
        self.raw_state = torch.zeros(_lib.STATE_WORDS, dtype=torch.int32, device=dev)              # a per-step copy of the step word
        key = "item_embedding.weight"
        self.table, self.table_grad = inner.views[key], inner.grad_views[key]                      # G and dG
        self.views = OrderedDict(inner.views)
        self.grad_views = OrderedDict(inner.grad_views)
        self.views[key] = self.raw.view(N, D)
        self.grad_views[key] = self.raw_grad[:N * D].view(N, D)

    def __getattr__(self, name):                  # everything else (lib, D, n_items, seed, state, ...) is the inner engine's
        inner = self.__dict__.get("inner")
        if inner is None:
            raise AttributeError(name)
        return getattr(inner, name)


class _GnnOptimizer:
    """optimizer facade: dr4sr_optimizer_flat over the reference's parameter set — the raw table, then position table + layers (the rest of
    the engine's flat buffer) — with ONE step count (the engine's state word; the raw table's call works on a copy of it).  G carries no
    moments and is never stepped."""

    def __init__(self, model):
        self.model = model
        eng = model.engine
        self.param_groups = [{"lr": eng.lr, "weight_decay": eng.weight_decay}]

    def zero_grad(self, set_to_none: bool = False):
        eng = self.model.engine
        eng.inner.grads.zero_()
        eng.raw_grad.zero_()

    def step(self):
        eng = self.model.engine
        inner, lib = eng.inner, eng.lib
        nd, n_all, off = eng.raw.numel(), inner.n_params, inner.offsets[1]
        inner.grads[n_all:n_all + 1].fill_(1.0)                    # API path: the loss is already normalised
        eng.raw_grad[nd:nd + 1].fill_(1.0)
        eng.raw_state[:1].copy_(inner.state[:1])                   # both calls see step t - 1 and bump their own word
        args = (eng.lr, eng.betas[0], eng.betas[1], eng.adam_eps, eng.weight_decay, _lib.cur_stream())
        _lib.check(lib.dr4sr_optimizer_flat(eng.optimizer, _lib.ptr(eng.raw), _lib.ptr(eng.raw_grad), _lib.ptr(eng.raw_m), _lib.ptr(eng.raw_v),
                                            nd, _lib.ptr(eng.raw_state), *args), "dr4sr_optimizer_flat (item table)")
        _lib.check(lib.dr4sr_optimizer_flat(eng.optimizer, _lib.ptr(inner.params[off:]), _lib.ptr(inner.grads[off:]),
                                            _lib.ptr(inner.adam_m[off:]), _lib.ptr(inner.adam_v[off:]), n_all - off, _lib.ptr(inner.state),
                                            *args), "dr4sr_optimizer_flat (encoder)")

    def state_dict(self):
        eng = self.model.engine
        off = eng.inner.offsets[1]
        return {"step": int(eng.inner.state[_lib.STATE_STEP]),
                "exp_avg": torch.cat([eng.raw_m, eng.inner.adam_m[off:]]), "exp_avg_sq": torch.cat([eng.raw_v, eng.inner.adam_v[off:]])}


class _Propagate(torch.autograd.Function):
    """E -> G (GNNQueryEncoder.get_gnn_embeddings) through dr4sr_gnn_propagate; the backward is the same call on dG, accumulating into E's
    gradient buffer (A is symmetric)"""

    @staticmethod
    def forward(ctx, model, E):
        eng = model.engine
        model._propagate(eng.views["item_embedding.weight"], eng.table, 0)
        ctx.model = model
        return eng.table.detach()

    @staticmethod
    def backward(ctx, gG):
        model = ctx.model
        model._propagate(gG.contiguous(), model.engine.grad_views["item_embedding.weight"], 1)
        return None, None


class _Encode(torch.autograd.Function):
    """SASRec's encoder on G (the engine's table slot) through dr4sr_sasrec_encode / _encode_bwd; the backward hands dG (the table slot of
    the flat gradient, which belongs to this pass alone: G is never stepped) on to _Propagate"""

    @staticmethod
    def forward(ctx, model, G, idx, seqlen, training, pooling):
        inner = model.engine.inner
        idx, seqlen = idx.contiguous(), seqlen.contiguous()
        out = inner.encode(inner.make_plan(idx, None, seqlen), training, pooling)
        ctx.model, ctx.args = model, (idx, seqlen, training, pooling)
        return out

    @staticmethod
    def backward(ctx, gout):
        idx, seqlen, training, pooling = ctx.args
        eng = ctx.model.engine
        eng.table_grad.zero_()
        eng.inner.encode_bwd(eng.inner.make_plan(idx, None, seqlen), training, pooling, gout.contiguous())
        return None, eng.table_grad, None, None, None, None


class GNNQueryEncoder(nn.Module):
    def __init__(self, fiid, embed_dim, max_seq_len, n_head, hidden_size, dropout, activation, layer_norm_eps, n_layer, item_encoder, graph,
                 gnn_layer=2, bidirectional=False, training_pooling_type="origin", eval_pooling_type="last", engine=None, owner=None) -> None:
        super().__init__()
        if bidirectional:
            raise NotImplementedError("HIP GNN: bidirectional attention is not implemented (the encoder kernels are causal)")
        if activation != "gelu":
            raise NotImplementedError("HIP GNN: exact-erf GELU only (configs/gnn.yaml)")
        self.fiid, self.item_encoder, self.gnn_layer = fiid, item_encoder, int(gnn_layer)
        self.training_pooling_type, self.eval_pooling_type = training_pooling_type, eval_pooling_type
        pre = "query_encoder."
        self.position_emb = _Embedding(engine, pre + "position_emb.weight", max_seq_len, embed_dim)
        self.transformer_layer = _Encoder(engine, pre + "transformer_layer.", embed_dim, hidden_size, layer_norm_eps, n_layer)
        self.dropout = nn.Dropout(p=dropout)
        self.norm_adj = graph                     # (row_ptr, col, val): a plain attribute, not a buffer (as the reference's)
        self._owner = [owner]                     # not a submodule (avoid a cycle in the module tree)
        w = torch.empty(3 * embed_dim, embed_dim)                     # torch's MultiheadAttention init, as SASRecQueryEncoder
        nn.init.xavier_uniform_(w)
        for lyr in self.transformer_layer.layers:
            lyr.self_attn.in_proj_weight.data.copy_(w)
            lyr.self_attn.in_proj_bias.data.zero_()

    _POOL = {"origin": _lib.POOL_ORIGIN, "last": _lib.POOL_LAST, "mean": _lib.POOL_MEAN}

    def get_gnn_embeddings(self):
        model = self._owner[0]
        return _Propagate.apply(model, model.item_embedding.weight)

    def forward(self, batch, need_pooling=True):
        if batch.get("seq_emb", None) is not None or "input_weight" in batch:
            raise NotImplementedError("seq_emb / input_weight inputs are unused by the shipped configs and not on the HIP path")
        if not need_pooling:
            pooling = _lib.POOL_NONE
        else:
            pooling = self._POOL[self.training_pooling_type if self.training else self.eval_pooling_type]
        return _Encode.apply(self._owner[0], self.get_gnn_embeddings(), batch["in_" + self.fiid], batch["seqlen"], bool(self.training), pooling)


class GNN(BaseModel):
    def __init__(self, config, dataset_list) -> None:
        super().__init__(config, dataset_list)
        mc, tc = config["model"], config["train"]
        if self.world_size > 1:
            raise NotImplementedError("HIP GNN: data parallelism (WORLD_SIZE > 1) is not implemented")
        if mc.get("bidirectional", False):
            raise NotImplementedError("HIP GNN: bidirectional attention is not implemented (the encoder kernels are causal)")
        if mc["graph"] not in ("old", "new"):
            raise ValueError(f"model.graph {mc['graph']!r}: 'old' (validation rows) or 'new' (training rows)")
        max_b = max(int(tc["batch_size"]), int(config["eval"]["batch_size"]))
        inner = SasrecEngine(self.num_items, self.max_seq_len, self.embed_dim, mc["head_num"], mc["hidden_size"], mc["layer_num"],
                             mc["layer_norm_eps"], mc["dropout_rate"], max_b, self.device, seed=int(tc["seed"]) + 7919 * self.rank,
                             lr=float(tc["learning_rate"]), weight_decay=float(tc["weight_decay"]))
        self.engine = _GnnEngine(inner)
        self.device = inner.device
        fields = getattr(dataset_list[0], "fields", None)
        sl = fields().get("seqlen") if callable(fields) else None
        inner.mean_len = float(sl.clamp(0, self.max_seq_len).float().mean()) if sl is not None and sl.numel() else None
        graph = self._build_graph_old() if mc["graph"] == "old" else self._build_graph()
        self.gnn_layer = int(mc["gnn_layer"])
        self.item_embedding = _Embedding(self.engine, "item_embedding.weight", self.num_items, self.embed_dim, padding_idx=0)
        self.query_encoder = GNNQueryEncoder(self.fiid, self.embed_dim, self.max_seq_len, mc["head_num"], mc["hidden_size"], mc["dropout_rate"],
                                             mc["activation"], mc["layer_norm_eps"], mc["layer_num"], self.item_embedding, graph,
                                             self.gnn_layer, engine=self.engine, owner=self)
        self.set_graph(graph)

    # ---- graph (model/gnn.py:102-171) ---------------------------------------------------------------------------------------
    def _graph_of(self, data, drop_last):
        ids, sl = data[1].to(self.device), data[3].to(self.device)
        return build_graph(ids, sl, self.num_items, int(self.config["model"]["window"]), drop_last)

    def _build_graph_old(self):
        """the validation split's rows of the eval domain, without their last item (the training target)"""
        val = self.dataset_list[1]
        return self._graph_of(val.data[val.eval_domain], True)

    def _build_graph(self):
        """the training split's rows"""
        return self._graph_of(self.dataset_list[0].data, False)

    def set_graph(self, graph):
        """install (row_ptr, col, val) — build_graph's CSR on this model's device — and size the propagation workspace for it"""
        row_ptr, col, val = (t.to(self.device).contiguous() for t in graph)
        assert row_ptr.dtype == torch.int64 and col.dtype == torch.int32 and val.dtype == torch.float32
        assert int(row_ptr.numel()) == self.num_items + 1 and int(col.numel()) == int(val.numel())
        self._gnn_ws_bytes = int(self.engine.lib.dr4sr_gnn_workspace_bytes(self.num_items, self.embed_dim, int(col.numel())))
        if self._gnn_ws_bytes <= 0:
            raise _lib.Dr4srError(f"GNN: embed_dim {self.embed_dim}: dr4sr_gnn_workspace_bytes failed: "
                                  + _lib._ERR.get(self._gnn_ws_bytes, str(self._gnn_ws_bytes)) + " — built for embed_dim 64 or 128")
        self._gnn_ws = torch.empty(self._gnn_ws_bytes, dtype=torch.uint8, device=self.device)
        self.query_encoder.norm_adj = (row_ptr, col, val)
        self.__dict__.pop("_api_graphs", None)       # captured steps hold the old graph's addresses

    def _propagate(self, src, dst, accumulate):
        """dst (+)= mean_{k = 0..gnn_layer} A^k src  (dr4sr_gnn_propagate on the current stream)"""
        row_ptr, col, val = self.query_encoder.norm_adj
        _lib.check(self.engine.lib.dr4sr_gnn_propagate(_lib.ptr(row_ptr), _lib.ptr(col), _lib.ptr(val), self.num_items, self.embed_dim,
                                                       self.gnn_layer, _lib.ptr(src), _lib.ptr(dst), int(accumulate), _lib.ptr(self._gnn_ws),
                                                       self._gnn_ws_bytes, _lib.cur_stream()), "dr4sr_gnn_propagate")

    # ---- model surface ----------------------------------------------------------------------------------------------------------
    def forward(self, batch, need_pooling=True):
        return self.query_encoder(batch, need_pooling)

    def training_step(self, batch, reduce=True, return_query=False, align=False):
        return super().training_step(batch, reduce, return_query)

    def _get_optimizers(self):
        super()._get_optimizers()                  # the optimizer's kind and constants, on the engine facade
        return _GnnOptimizer(self)

    def _fast_path_ok(self) -> bool:             # the fused step gathers and scores one table
        return False

    # ---- API step under a HIP graph --------------------------------------------------------------------------------------------
    def _api_graph_ok(self) -> bool:
        return bool(self.config["train"].get("hip_graph", True)) and self.world_size == 1

    def _api_graph_fields(self):
        return {"in_" + self.fiid, self.fiid, "seqlen", self.fuid}

    def _api_graph_state(self):
        eng = self.engine
        return super()._api_graph_state() + [eng.raw, eng.raw_m, eng.raw_v, eng.raw_state]

    def _api_step_body(self, batch):
        """the loop body of basemodel.py:192-200 composed from the C-ABI calls directly (what autograd would run, in the same order,
        without its bookkeeping): propagate, encode, scorer + BCE forward and backward, encoder backward, propagate dG, optimizer"""
        if not isinstance(self.loss_fn, BinaryCrossEntropyLoss):
            return super()._api_step_body(batch)
        eng, inner, lib = self.engine, self.engine.inner, self.engine.lib
        ids, tgt, lens = batch["in_" + self.fiid].contiguous(), batch[self.fiid].contiguous(), batch["seqlen"].contiguous()
        neg = self._neg_sampling(batch).contiguous().view(-1)
        self.optimizer.zero_grad()
        E, dE = eng.views["item_embedding.weight"], eng.grad_views["item_embedding.weight"]
        self._propagate(E, eng.table, 0)
        pooling = GNNQueryEncoder._POOL[self.query_encoder.training_pooling_type]
        plan = inner.make_plan(ids, None, lens)
        q = inner.encode(plan, True, pooling)
        B, L = int(tgt.shape[0]), int(tgt.shape[1]) if tgt.dim() == 2 else 1
        lp = torch.empty(B * L, dtype=torch.float32, device=self.device)
        stats = torch.zeros(2, dtype=torch.float32, device=self.device)
        st = _lib.cur_stream
        _lib.check(lib.dr4sr_score_bce_fwd(_lib.ptr(q), _lib.ptr(E), _lib.ptr(tgt.view(-1)), _lib.ptr(neg), None, None, _lib.ptr(lp),
                                           _lib.ptr(stats), B, L, eng.D, st()), "score_loss_fwd")
        loss = stats[1] / stats[0]
        dq = torch.empty_like(q)
        scale = (1.0 / stats[0]).reshape(1).contiguous()
        _lib.check(lib.dr4sr_score_bce_bwd(_lib.ptr(q), _lib.ptr(E), _lib.ptr(tgt.view(-1)), _lib.ptr(neg), None, _lib.ptr(scale), _lib.ptr(dq),
                                           _lib.ptr(dE), B, L, eng.D, st()), "score_loss_bwd")
        inner.encode_bwd(plan, True, pooling, dq)
        self._propagate(eng.table_grad, dE, 1)
        self.optimizer.step()
        return loss
