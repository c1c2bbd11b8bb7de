"""ORACLE (test infrastructure, NOT product code) — CPU restatement of CL4SRec's contrastive branch
(/root/reference model/cl4srec.py:49-73, module/data_augmentation.py:305-350, :577-619, module/functional.py:28-55).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module.
Pinned against tests/golden/cl4srec_d64.npz (made by RUNNING the reference with its drawn views recorded: tools/make_golden.py
run_cl_case) by tests/test_cl_oracle.py.  Also holds reference-style augmentations in plain Python for distribution tests.

The draw mirrors at the end (augment_mirror, neg_sample_mirror, fmlp_neg_mirror) are not restatements of the reference but of the
product's kernels, and they take their Philox4x32-10 from the product (dr4sr_amd.regen_dropout.philox4x32_10, numpy): that function is
pinned by the known-answer test of tests/test_pairs_cpu.py and bit-equal to csrc/common.h by tests/test_gpu_regen_dropout.py.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from dr4sr_amd.regen_dropout import philox4x32_10

from . import sasrec_oracle as so


def mean_pool(x, seqlen):
    """seq_pooling_function(pooling_type='mean') (module/functional.py:28-55): rows >= seqlen zeroed, sum / seqlen"""
    L = x.shape[1]
    keep = (torch.arange(L).view(1, L) < seqlen.view(-1, 1)).unsqueeze(-1)
    return torch.where(keep, x, torch.zeros((), dtype=x.dtype)).sum(1) / seqlen.view(-1, 1).to(x.dtype)


def infonce(rep_i, rep_j, temperature=1.0, reduce=True):
    """InfoNCELoss(sim_method='inner_product', neg_type='batch_both') (data_augmentation.py:322-350)"""
    B = rep_i.shape[0]
    sim_ii = rep_i @ rep_i.T / temperature
    sim_ij = rep_i @ rep_j.T / temperature
    sim_ii = sim_ii.masked_fill(torch.eye(B, dtype=torch.bool), float("-inf"))
    logits = torch.cat([sim_ij, sim_ii], dim=-1)
    labels = torch.arange(B)
    if reduce:
        return F.cross_entropy(logits, labels)
    return F.cross_entropy(logits, labels, reduction="none") / B


def view_mean(p, view, view_len, H, n_layer, eps):
    x = so.sasrec_encode(p, view, view_len, H, n_layer, eps, None)
    return mean_pool(x, view_len)


def training_loss(p, batch, views, cfg, reduce=True):
    """CL4SRec.training_step (cl4srec.py:49-73) on given views = ((seq_i, len_i), (seq_j, len_j))"""
    H, nl, eps = cfg["H"], cfg["n_layer"], cfg["eps"]
    bce, q, _, _ = so.training_step(p, batch, H, nl, eps, reduce=reduce)
    (vi, li), (vj, lj) = views
    oi, oj = view_mean(p, vi, li, H, nl, eps), view_mean(p, vj, lj, H, nl, eps)
    keep = batch["seqlen"] != 1                                       # data_augmentation.py:613-615
    cl = infonce(oi[keep], oj[keep], cfg["temperature"], reduce)
    return bce + cfg["cl_weight"] * cl, bce, cl, oi, oj


def training_loss_q(p, batch, views, cfg, reduce=True):
    """CL4SRec.training_step(return_query=True) (cl4srec.py:49-73): reduce=True -> (bce + cl_weight * InfoNCE, query); reduce=False ->
    ((bce per position / n_valid, cl_weight * InfoNCE rows / kept rows), query) — the tuple MetaModel.training_step takes apart
    (metamodel.py:186-192)"""
    H, nl, eps = cfg["H"], cfg["n_layer"], cfg["eps"]
    bce, q, _, _ = so.training_step(p, batch, H, nl, eps, reduce=reduce)
    (vi, li), (vj, lj) = views
    oi, oj = view_mean(p, vi, li, H, nl, eps), view_mean(p, vj, lj, H, nl, eps)
    keep = batch["seqlen"] != 1
    cl = cfg["cl_weight"] * infonce(oi[keep], oj[keep], cfg["temperature"], reduce)
    return (bce + cl if reduce else (bce, cl)), q


# ---- reference-style augmentations (plain Python), for distribution tests of dr4sr_cl_augment
def crop_len(n, tau):
    return max(1, int(tau * n))


def mask_count(n, gamma):
    return int(gamma * n)


def reorder_len(n, beta):
    return int(beta * n)


# ---- host mirror of the device draws (numpy only): csrc/cl.hip k_cl_augment word for word, and the negative samplers of
# csrc/common.h sample_neg_id / csrc/fmlp.hip k_fmlp_score.  The kernels are the authority; tests/test_gpu_cl_kernels.py holds them
# bit-equal to these functions, tests/test_cl_augment_cpu.py checks the DISTRIBUTION of what these functions draw.
SITE_AUG = 0x41554721            # DR4SR_SITE_AUG (csrc/cl.hip)
SITE_NEG = 0x4E454721            # DR4SR_SITE_NEG (csrc/common.h)
SITE_NEG_F = 0x4E454722          # DR4SR_SITE_NEG_F (csrc/fmlp.hip)
RANDOM_STREAM = 0xFFFFFF         # the stream whose word 0 picks Item_Random's method, once per call
AUG_WORDS = 68                   # a full-width reorder at L = 64 reads word 64: 17 Philox calls per stream


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def stream_words(site, streams, n_words, seed, step, shift=8):
    """uint64 [len(streams), n_words]: word k of stream s at (seed, step) = component k & 3 of
    philox(counter = (lo, hi, site, step), key = seed) with lo | hi << 32 = (s << shift) + (k >> 2)  (csrc/common.h rng_call)"""
    m32 = np.uint64(0xFFFFFFFF)
    s = _u64(streams).reshape(-1)
    call = (s[:, None] << np.uint64(shift)) + np.arange((int(n_words) + 3) // 4, dtype=np.uint64)[None, :]
    w = philox4x32_10(call & m32, call >> np.uint64(32), np.uint64(site), np.uint64(int(step) & 0xFFFFFFFF), int(seed) & 0xFFFFFFFFFFFFFFFF)
    return np.stack(w, -1).reshape(s.shape[0], -1)[:, :int(n_words)]


def rand_below(r, n):
    """(r * n) >> 32 for a 32-bit word r: uniform on [0, n)  (__umulhi)"""
    return ((_u64(r) * _u64(n)) >> np.uint64(32)).astype(np.int64)


def augment_mirror(seq, seqlen, mode, tau, gamma, beta, mask_id, seed, step, rows=None):
    """(out [B, L], out_len [B], mode_used) of k_cl_augment at call number `step`: mode 0 crop (tau), 1 mask (gamma, mask_id),
    2 reorder (beta), 3 one of the three drawn once per call.  rows != None: seq / seqlen are dataset tensors and the batch is
    their rows rows[0..B); the stream of a sequence is keyed by its batch slot b (stream b + 1) either way.  Every slot runs the
    kernel's serial chain; the chains of the batch advance together, one numpy operation per link."""
    seq, seqlen = np.asarray(seq, dtype=np.int64), np.asarray(seqlen, dtype=np.int64)
    if rows is not None:
        rows = np.asarray(rows, dtype=np.int64)
        seq, seqlen = seq[rows], seqlen[rows]
    B, L = seq.shape
    if not (0 < L <= 64) or mode not in (0, 1, 2, 3):
        raise ValueError("k_cl_augment takes 0 < L <= 64 and mode 0..3")
    if mode == 3:
        mode = int(rand_below(stream_words(SITE_AUG, [RANDOM_STREAM], 1, seed, step)[0, 0], 3))
    n = np.clip(seqlen, 0, L)
    w = stream_words(SITE_AUG, np.arange(B, dtype=np.uint64) + np.uint64(1), AUG_WORDS, seed, step)
    pos = np.arange(L, dtype=np.int64)[None, :]
    nf = n.astype(np.float64)
    if mode == 0:
        sub = np.where(n > 0, np.maximum(1, (tau * nf).astype(np.int64)), 0)            # int(tau * n) in double
        start = np.where(n > 0, rand_below(w[:, 0], np.maximum(n - sub + 1, 1)), 0)
        src = np.take_along_axis(seq, np.minimum(start[:, None] + pos, L - 1), 1)
        return np.where(pos < sub[:, None], src, 0), sub, mode
    if mode == 1:
        need = (gamma * nf).astype(np.int64)
        out = seq.copy()
        for l in range(L):                                 # selection sampling: position l is taken with probability need / remaining
            take = (l < n) & (need > 0) & (rand_below(w[:, l], np.maximum(n - l, 0)) < need)
            out[take, l] = mask_id
            need = need - take
        return out, n, mode
    sub = (beta * nf).astype(np.int64)
    start = rand_below(w[:, 0], n - sub + 1)
    idx = np.broadcast_to(pos, (B, L)).copy()
    b = np.arange(B)
    for k in range(L - 1, 0, -1):                          # Fisher-Yates from the segment's end; slots with sub <= k sit this link out
        j = np.where(k < sub, rand_below(w[:, 1 + k], k + 1), k)
        t = idx[b, k].copy()
        idx[b, k] = idx[b, j]
        idx[b, j] = t
    inside = (pos >= start[:, None]) & (pos < (start + sub)[:, None])
    from_ = start[:, None] + np.take_along_axis(idx, np.clip(pos - start[:, None], 0, L - 1), 1)
    return np.where(inside, np.take_along_axis(seq, np.clip(from_, 0, L - 1), 1), seq), n, mode


def _neg_ids(site, n, n_items, seed, step):
    w = stream_words(site, np.arange((int(n) + 3) // 4, dtype=np.uint64), 4, seed, step, shift=0).reshape(-1)[:int(n)]
    return 1 + rand_below(w, n_items - 1)


def neg_sample_mirror(n, n_items, seed, step):
    """int64 [n]: what dr4sr_neg_sample writes, and element b * L + pos of an in-step draw at (seed, state[RNGSTEP]): element e is
    1 + ((w * (n_items - 1)) >> 32) with w = word e & 3 of call e >> 2 of site DR4SR_SITE_NEG: uniform on [1, n_items - 1]"""
    return _neg_ids(SITE_NEG, n, n_items, seed, step)


def fmlp_neg_mirror(B, n_items, seed, step):
    """int64 [B]: the negative of row b of an FMLP step (one per row): the same draw from site DR4SR_SITE_NEG_F, element b"""
    return _neg_ids(SITE_NEG_F, B, n_items, seed, step)
