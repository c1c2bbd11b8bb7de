"""Rank metrics with the semantics of the reference's evaluation/__init__.py: recall (:9-33), precision (:39-62), f1 (:65-84),
map (:87-104), ndcg (:107-134), mrr (:137-156), hits (:159-171) on [B, K] hit matrices, and the registry (:235-299).  The shipped
configs use eval.val_metrics/test_metrics = [ndcg, recall].

rank_metrics() is the same seven metrics as functions of ONE integer per row, the target's rank: the oracle of the device path of
eval.rank_eval (csrc/rank.hip, dr4sr_rank_metrics_accumulate) and the statement of its formulas."""
from __future__ import annotations

import sys
from typing import List, Union

import torch


def recall(pred: torch.Tensor, target: torch.Tensor, k: int, mean: bool = True):
    """pred [B,K] bool hit matrix in rank order; target [B,n_target] relevance."""
    count = (target > 0).sum(-1)
    out = pred[:, :k].sum(dim=-1).float() / count
    return out.mean() if mean else out


def _dcg(pred: torch.Tensor, k: int):
    k = min(k, pred.size(1))
    denom = torch.log2(torch.arange(k, device=pred.device).type_as(pred) + 2.0).view(1, -1)
    return (pred[:, :k] / denom).sum(dim=-1)


def ndcg(pred: torch.Tensor, target: torch.Tensor, k: int, mean: bool = True):
    pred_dcg = _dcg(pred.float(), k)
    ideal = _dcg(torch.sort((target > 0).float(), descending=True)[0], k)
    irrelevant = torch.all(target <= sys.float_info.epsilon, dim=-1)
    pred_dcg = torch.where(irrelevant, torch.zeros_like(pred_dcg), pred_dcg / torch.where(irrelevant, torch.ones_like(ideal), ideal))
    return pred_dcg.mean() if mean else pred_dcg


def precision(pred: torch.Tensor, target: torch.Tensor, k: int):
    return (pred[:, :k].sum(dim=-1).float() / k).mean()


def f1(pred: torch.Tensor, target: torch.Tensor, k: int):
    count = (target > 0).sum(-1)
    return (2 * pred[:, :k].sum(dim=-1).float() / (count + k)).mean()


def map(pred: torch.Tensor, target: torch.Tensor, k: int):  # noqa: A001  (the reference's name)
    """mean average precision; k must not exceed pred's width (the reference's positions 1..k do not broadcast otherwise)"""
    count = (target > 0).sum(-1)
    p = pred[:, :k].float()
    prec_at = p.cumsum(dim=-1) / torch.arange(1, k + 1, device=p.device).type_as(p)
    return ((prec_at * p).sum(dim=-1) / torch.minimum(count, torch.full_like(count, k))).mean()


def mrr(pred: torch.Tensor, target: torch.Tensor, k: int):
    """1 / (1-based position of the row's first hit among the first k), 0 for a row without one"""
    p = pred[:, :k] > 0
    first = p.float().argmax(dim=-1) + 1                   # argmax returns the first maximum
    return torch.where(p.any(dim=-1), 1.0 / first.float(), torch.zeros(p.size(0), device=p.device)).mean()


def hits(pred: torch.Tensor, target: torch.Tensor, k: int):
    return torch.any(pred[:, :k] > 0, dim=-1).float().mean()


def rank_metrics(rank: torch.Tensor, label: torch.Tensor, names, cutoffs, topk: int, dtype=torch.float64):
    """{"name@c": mean over the rows} from rank [B] (the number of valid items ahead of the row's single target;
    _lib.RANK_NONE = the target is no valid item, a miss at every cutoff) and label [B] (the target's relevance).  Per row, with
    h = [rank < c] and count = [label > 0] — what the matrix functions above give for a hit matrix with its one True at column rank:

        hit = h    recall = h / count    precision = h / c    f1 = 2 h / (count + c)    mrr = h ? 1 / (rank + 1) : 0
        map = h (1 / (rank + 1)) / min(count, c)    ndcg = label <= eps ? 0 : h / log2(rank + 2)   (one relevant item: ideal DCG 1)

    A row with label <= 0 gives what these formulas give, NaN included.  Pure torch, any device."""
    names = names if isinstance(names, (list, tuple)) else [names]
    cutoffs = cutoffs if isinstance(cutoffs, (list, tuple)) else [cutoffs]
    r = rank.reshape(-1).to(dtype)
    lab = label.reshape(-1).to(dtype)
    count = (lab > 0).to(dtype)
    inv = 1.0 / (r + 1.0)
    zero = torch.zeros_like(r)
    out = {}
    for c in cutoffs:
        if not 1 <= int(c) <= int(topk):
            raise ValueError(f"cutoff {c} is outside [1, topk = {topk}]")
        hb = r < c
        h = hb.to(dtype)
        per_row = {"hit": h, "recall": h / count, "precision": h / c, "f1": 2 * h / (count + c), "mrr": torch.where(hb, inv, zero),
                   "map": h * inv / torch.clamp(count, max=float(c)),
                   "ndcg": torch.where(lab <= sys.float_info.epsilon, zero, h / torch.log2(r + 2.0))}
        for n in names:
            out[f"{n}@{c}"] = per_row[n].mean()
    return out


metric_dict = {"ndcg": ndcg, "recall": recall, "precision": precision, "map": map, "mrr": mrr, "hit": hits, "f1": f1}
_RANK = {"ndcg", "precision", "recall", "map", "mrr", "hit", "f1"}


def get_rank_metrics(metric):
    metric = metric if isinstance(metric, list) else [metric]
    return [(m, metric_dict[m]) for m in metric if m in _RANK and m in metric_dict]


def get_eval_metrics(metric_names: Union[List[str], str], cutoffs, validation: bool = False) -> List[str]:
    metric_names = metric_names if isinstance(metric_names, list) else [metric_names]
    rank = {m for m, _ in get_rank_metrics(metric_names)}
    if cutoffs is None:
        return []
    cutoffs = cutoffs if isinstance(cutoffs, list) else [cutoffs]
    if validation:
        cutoffs = cutoffs[:1]
    return [f"{m}@{c}" if m in rank else m for c in cutoffs for m in metric_names]
