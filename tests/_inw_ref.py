"""CPU torch restatement of SASRec's encoder with a per-token input weight (the reference's model/sasrec.py:61-64:
`transformer_input = batch['input_weight'] * (seq_embs + position_embs)`, then the embedding-stage dropout), composed from
oracle.sasrec_oracle: embed_posadd, _drop at SITE_EMB, sasrec_layer, the poolings and score_bce.  The yardstick of
tests/test_input_weight_cpu.py (which proves it equal to the golden vectors made by running the reference) and of
tests/test_gpu_input_weight.py; and the loader of tests/golden/sasrec_input_weight.npz."""
import os

import numpy as np
import torch

from oracle import sasrec_oracle as O

TABLE = "item_embedding.weight"
TIED = "query_encoder.item_encoder.weight"
GOLDEN = "sasrec_input_weight.npz"


def load_golden(golden_dir):
    z = np.load(os.path.join(golden_dir, GOLDEN))
    return {k: z[k] for k in z.files}


def golden_params(g):
    p = {k[len("param."):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param.")}
    p[TIED] = p[TABLE]
    return p


def golden_batch(g):
    return {k[len("batch."):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("batch.")}


def encode(p, idx, seqlen, weight, H, n_layer, eps, pooling, masks=None, pdrop=0.0):
    """O.sasrec_encode with x0 = drop(weight * (E[idx] + P)); weight broadcasts to [B, L, 1] (None: no weight);
    pooling 'origin' | 'last' | 'mean' | None"""
    x = O.embed_posadd(p[TABLE], p["query_encoder.position_emb.weight"], idx)
    if weight is not None:
        x = weight * x
    x = O._drop(x, masks, O.SITE_EMB, pdrop)
    key_pad = idx == 0
    for i in range(n_layer):
        x = O.sasrec_layer(x, key_pad, p, O.layer_prefix(i), H, eps, masks, i, pdrop)
    B, L, D = x.shape
    keep = (torch.arange(L).view(1, L) < seqlen.view(B, 1)).unsqueeze(-1)
    if pooling == "origin":
        return torch.where(keep, x, torch.zeros((), dtype=x.dtype))
    if pooling == "last":
        return x[torch.arange(B), seqlen - 1]
    if pooling == "mean":
        return torch.where(keep, x, torch.zeros((), dtype=x.dtype)).sum(1) / seqlen.view(B, 1).to(x.dtype)
    if pooling is None:
        return x
    raise ValueError(pooling)


def _leaves(params, weight, dtype):
    leaf = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items() if k != TIED}
    w = weight.detach().to(dtype).clone().requires_grad_(True)
    return leaf, w


def _grads(out, leaf, w, grad_out=None):
    names = list(leaf)
    gs = torch.autograd.grad(out, [leaf[k] for k in names] + [w], grad_out, allow_unused=True)
    g = {k: (v if v is not None else torch.zeros_like(leaf[k])).detach() for k, v in zip(names, gs[:-1])}
    return g, (gs[-1] if gs[-1] is not None else torch.zeros_like(w)).detach()


def encode_grads(params, idx, seqlen, weight, d_out, H, n_layer, eps, pooling="origin", masks=None, pdrop=0.0, dtype=torch.float32):
    """-> (out, {param: d <out, d_out> / d param}, d / d weight in weight's shape): what dr4sr_sasrec_encode_w + _encode_w_bwd compute"""
    leaf, w = _leaves(params, weight, dtype)
    out = encode(leaf, idx, seqlen, w, H, n_layer, eps, pooling, masks, pdrop)
    g, gw = _grads(out, leaf, w, d_out.to(dtype))
    return out.detach(), g, gw


def step_grads(params, batch, weight, H, n_layer, eps, masks=None, pdrop=0.0, dtype=torch.float32):
    """-> (loss, query, grads, d loss / d weight): BaseModel.training_step (origin pooling, BCE, reduce=True) with the weighted encoder"""
    leaf, w = _leaves(params, weight, dtype)
    q = encode(leaf, batch["in_item_id"], batch["seqlen"], w, H, n_layer, eps, "origin", masks, pdrop)
    loss, _, _ = O.score_bce(q, leaf[TABLE], batch["item_id"], batch["neg_item"])
    g, gw = _grads(loss, leaf, w)
    return loss.detach(), q.detach(), g, gw


def rel(a, b):
    """max |a - b| relative to max |b|"""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
