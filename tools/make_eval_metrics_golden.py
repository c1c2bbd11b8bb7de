#!/usr/bin/env python
"""Golden fixture of the seven rank metrics (tests/golden/eval_metrics.npz) by RUNNING the reference's evaluation/__init__.py.

Works only where the reference checkout (USTC-StarTeam/DR4SR) exists.  The module is imported unmodified, with the no-op stub of the
absent torchmetrics package that make_golden.py installs; its metric_dict functions are applied to seeded hit
matrices: B = 37 rows, K = 100 columns, at most one hit per row (the evaluation's case: one target per row), some rows with none, one
hit in the first and one in the last column; labels all 1; cutoffs [1, 5, 10, 20, 100].

Only DATA is written: the inputs (pred [37, 100] bool, target [37, 1] fp32, cutoffs) and the recorded outputs, one fp64 scalar per
metric and cutoff under "out.<name>@<c>".

    python tools/make_eval_metrics_golden.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from make_golden import REF, _install_stubs  # noqa: E402  (where the reference checkout lives; the torchmetrics stub)

NAMES = ("ndcg", "recall", "precision", "map", "mrr", "hit", "f1")
CUTOFFS = (1, 5, 10, 20, 100)
B, K, SEED = 37, 100, 20240


def main():
    if not os.path.isdir(REF):
        sys.exit("reference not present; golden vectors can only be regenerated where its checkout exists")
    _install_stubs()
    spec = importlib.util.spec_from_file_location("reference_evaluation", os.path.join(REF, "evaluation", "__init__.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    gen = torch.Generator().manual_seed(SEED)
    col = torch.randint(0, K, (B,), generator=gen)
    col[0], col[1], col[2], col[3] = 0, K - 1, 4, 5            # first / last column, both sides of the cutoff 5
    has = torch.rand(B, generator=gen) < 0.7
    has[:4] = True
    has[4] = False
    pred = torch.zeros(B, K, dtype=torch.bool)
    pred[torch.arange(B)[has], col[has]] = True
    target = torch.ones(B, 1)
    out = {"pred": pred.numpy(), "target": target.numpy(), "cutoffs": np.asarray(CUTOFFS, dtype=np.int64)}
    for name in NAMES:
        for c in CUTOFFS:
            out[f"out.{name}@{c}"] = np.float64(float(ref.metric_dict[name](pred.clone(), target.clone(), c)))
    path = os.path.join(ROOT, "tests", "golden", "eval_metrics.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", int(has.sum()), "of", B, "rows with a hit")


if __name__ == "__main__":
    main()
