"""CPU torch restatement of the GNN step (the reference's model/gnn.py), the yardstick of tests/test_gnn_cpu.py (which proves it equal to
the golden vectors made by running the reference) and tests/test_gpu_gnn.py:
  G = mean_{k = 0..n_hop} A^k E   (dense or torch.sparse propagation)
  query = oracle.sasrec_oracle.sasrec_encode on a parameter dict whose table is G
  loss = score_bce against the RAW E; gradients by autograd to the raw E
and loaders of tests/golden/gnn_small*.npz."""
import os

import numpy as np
import torch

from oracle import sasrec_oracle as O

TABLE = "item_embedding.weight"
TIED = "query_encoder.item_encoder.weight"


def load_golden(golden_dir):
    """-> (shared, {'old': part, 'new': part}) as dicts of numpy arrays"""
    def npz(name):
        z = np.load(os.path.join(golden_dir, name))
        return {k: z[k] for k in z.files}
    return npz("gnn_small.npz"), {m: npz(f"gnn_small.part_{m}.npz") for m in ("old", "new")}


def golden_params(shared):
    p = {k[len("param."):]: torch.from_numpy(v) for k, v in shared.items() if k.startswith("param.")}
    p[TIED] = p[TABLE]
    return p


def golden_batch(shared, prefix="batch."):
    return {k[len(prefix):]: torch.from_numpy(v) for k, v in shared.items() if k.startswith(prefix)}


def golden_rows(shared, mode):
    """the rows graph `mode` is built from -> (in_item_id int64 [rows, L], seqlen int64 [rows], drop_last)"""
    split = "val" if mode == "old" else "train"
    return (torch.from_numpy(shared[f"rows.{split}.in_item_id"].astype(np.int64)),
            torch.from_numpy(shared[f"rows.{split}.seqlen"].astype(np.int64)), mode == "old")


def coo_to_csr(row, col, val, n):
    """coalesced COO sorted by (row, col) -> (row_ptr int64, col int32, val float32) tensors"""
    row = torch.as_tensor(np.asarray(row)).long()
    ptr = torch.zeros(n + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.bincount(row, minlength=n), 0)
    return ptr, torch.as_tensor(np.asarray(col)).to(torch.int32), torch.as_tensor(np.asarray(val)).to(torch.float32)


def csr_to_sparse(row_ptr, col, val, dtype=torch.float32):
    n = int(row_ptr.numel()) - 1
    row = torch.repeat_interleave(torch.arange(n), (row_ptr[1:] - row_ptr[:-1]).cpu())
    return torch.sparse_coo_tensor(torch.stack([row, col.cpu().long()]), val.cpu().to(dtype), (n, n)).coalesce()


def propagate(A, X, n_hop):
    """mean_{k = 0..n_hop} A^k X, as GNNQueryEncoder.get_gnn_embeddings (model/gnn.py:43-50) computes it; A dense or sparse"""
    embs = [X]
    for _ in range(n_hop):
        X = torch.sparse.mm(A, X) if A.is_sparse else A @ X
        embs.append(X)
    return torch.stack(embs, dim=1).mean(1)


def gnn_step(params, A, batch, H, n_layer, eps, n_hop, reduce=True, dtype=torch.float32):
    """-> (loss, query, G, grads): one training step's forward and (reduce=True) its gradient for every parameter"""
    leaf = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items() if k != TIED}
    E = leaf[TABLE]
    G = propagate(A.to(dtype), E, n_hop)
    p2 = dict(leaf)
    p2[TABLE] = G
    q = O.sasrec_encode(p2, batch["in_item_id"], batch["seqlen"], H, n_layer, eps, "origin")
    loss, _, _ = O.score_bce(q, E, batch["item_id"], batch["neg_item"], reduce=reduce)
    grads = None
    if reduce:
        names = list(leaf)
        gs = torch.autograd.grad(loss, [leaf[k] for k in names], allow_unused=True)
        grads = {k: (g if g is not None else torch.zeros_like(leaf[k])).detach() for k, g in zip(names, gs)}
    return loss.detach(), q.detach(), G.detach(), grads


def adam1(params, grads, lr, wd):
    """the parameters after the first torch.optim.Adam step"""
    keys = [k for k in params if k != TIED]
    p = {k: params[k].clone() for k in keys}
    m = {k: torch.zeros_like(p[k]) for k in keys}
    v = {k: torch.zeros_like(p[k]) for k in keys}
    return O.adam_step(p, grads, m, v, 1, lr=lr, wd=wd)


def rel(a, b):
    """max |a - b| relative to max |b|"""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
