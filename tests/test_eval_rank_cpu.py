"""CPU tests of the evaluation module's rank metrics (dr4sr_amd/evaluation): the seven [B, K] hit-matrix functions against outputs
recorded from the reference (tests/golden/eval_metrics.npz, tools/make_eval_metrics_golden.py), rank_metrics — the same metrics as
functions of the target's rank, the oracle of the device path — against those functions, and the registry."""
import os

import numpy as np
import pytest
import torch

from dr4sr_amd import _lib, evaluation

NAMES = ["ndcg", "recall", "precision", "map", "mrr", "hit", "f1"]


def test_metric_functions_equal_the_recorded_reference_outputs(golden_dir):
    z = np.load(os.path.join(golden_dir, "eval_metrics.npz"))
    pred, target = torch.from_numpy(z["pred"]), torch.from_numpy(z["target"])
    assert pred.shape == (37, 100) and pred.dtype == torch.bool and int(pred.sum(1).max()) == 1 and int(pred.sum(1).min()) == 0
    assert [int(c) for c in z["cutoffs"]] == [1, 5, 10, 20, 100]
    fns = dict(evaluation.get_rank_metrics(NAMES))
    assert list(fns) == NAMES
    for name in NAMES:
        for c in z["cutoffs"]:
            got, ref = float(fns[name](pred, target, int(c))), float(z[f"out.{name}@{int(c)}"])
            assert abs(got - ref) <= 1e-6, (name, int(c), got, ref)


def _ranks(topk, gen):
    """0, both sides of each cutoff, the last column, >= topk, RANK_NONE, then random ones"""
    fixed = [0, 1, 4, 5, 6, 9, 10, 11, 19, 20, 21, topk - 1, topk, topk + 1, 10 * topk, _lib.RANK_NONE, _lib.RANK_NONE]
    rnd = torch.randint(0, 2 * topk, (80,), generator=gen).tolist()
    return torch.tensor(fixed + rnd, dtype=torch.int32)


@pytest.mark.parametrize("topk", [20, 100])
def test_rank_metrics_restate_the_matrix_functions(topk):
    gen = torch.Generator().manual_seed(topk)
    rank = _ranks(topk, gen)
    B = rank.numel()
    label = torch.ones(B)
    pred = torch.zeros(B, topk, dtype=torch.bool)
    inside = rank < topk
    pred[torch.arange(B)[inside], rank[inside].long()] = True
    cutoffs = [c for c in (1, 5, 10, 20, 100) if c <= topk]
    got = evaluation.rank_metrics(rank, label, NAMES, cutoffs, topk)
    assert list(got) == [f"{n}@{c}" for c in cutoffs for n in NAMES]
    fns = dict(evaluation.get_rank_metrics(NAMES))
    for c in cutoffs:
        for n in NAMES:
            v = got[f"{n}@{c}"]
            assert v.dtype == torch.float64
            ref = float(fns[n](pred, label.view(-1, 1), c))             # fp32
            assert abs(float(v) - ref) <= 1e-6, (n, c, float(v), ref)
    with pytest.raises(ValueError):
        evaluation.rank_metrics(rank, label, ["map"], [topk + 1], topk)


def test_registry_no_longer_drops_the_reference_metrics():
    got = evaluation.get_rank_metrics(["ndcg", "mrr", "hit"])
    assert [m for m, _ in got] == ["ndcg", "mrr", "hit"] and got[2][1] is evaluation.hits
    assert set(evaluation.metric_dict) == set(NAMES)
    assert evaluation.get_eval_metrics(["ndcg", "mrr", "hit"], [20, 10]) == ["ndcg@20", "mrr@20", "hit@20", "ndcg@10", "mrr@10", "hit@10"]
    assert evaluation.get_eval_metrics(["ndcg", "mrr", "hit"], [20, 10], validation=True) == ["ndcg@20", "mrr@20", "hit@20"]


def test_binding_names_the_rank_entry_points():
    assert _lib.RANK_NONE == 2 ** 31 - 1 and tuple(_lib.RANK_METRICS) == ("ndcg", "recall", "precision", "map", "mrr", "hit", "f1")
    lib = _lib.load()
    assert {"dr4sr_target_rank_workspace_bytes", "dr4sr_target_rank", "dr4sr_rank_metrics_accumulate"} <= set(_lib.SYMBOLS)
    # argument checks need no GPU
    assert lib.dr4sr_target_rank_workspace_bytes(0) >= 0 and lib.dr4sr_target_rank_workspace_bytes(-1) == -1
    assert lib.dr4sr_target_rank_workspace_bytes(2048) >= 2048 * 8
    assert lib.dr4sr_target_rank(None, None, None, None, None, None, 0, 64, 10, 0, None, 0, None) == 0          # B = 0: no-op
    assert lib.dr4sr_target_rank(None, None, None, None, None, None, 0, 96, 10, 0, None, 0, None) == -2         # width
    assert lib.dr4sr_target_rank(None, None, None, None, None, None, -1, 64, 10, 0, None, 0, None) == -1
    assert lib.dr4sr_target_rank(None, None, None, None, None, None, 4, 64, 10, 0, None, 0, None) == -1         # null pointers
    import ctypes as C
    cuts = (C.c_int32 * 2)(10, 101)
    assert lib.dr4sr_rank_metrics_accumulate(None, None, 0, cuts, 2, 100, C.c_void_p(8), None) == -1            # cutoff above topk
    cuts = (C.c_int32 * 2)(10, 100)
    assert lib.dr4sr_rank_metrics_accumulate(None, None, 0, cuts, 2, 100, C.c_void_p(8), None) == 0             # B = 0: no-op
    assert lib.dr4sr_rank_metrics_accumulate(None, None, 0, cuts, 9, 100, C.c_void_p(8), None) == -1
