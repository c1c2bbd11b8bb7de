#!/usr/bin/env python3
"""Measurement of evaluation by target rank (eval.rank_eval, csrc/rank.hip) against the top-k evaluation on one GPU.

  batch   one eval batch of B = 2 048 rows with Lh = 50 history words, at N = 11 925 / D = 64 and N = 20 034 / D = 128, both ways on the
          same random tensors, between HIP events, in alternating rounds inside one process (median and minimum of the per-round means):
            topk   dr4sr_full_score_topk_masked_ws (k = 100) + what BaseModel._test_step does with its ids: the hit matrix and the
                   torch metric functions (ndcg, recall at the cutoffs 20 and 10)
            rank   dr4sr_target_rank + dr4sr_rank_metrics_accumulate (all seven metrics at both cutoffs)
          with the algorithmic bytes and FLOPs of each (what has to cross HBM once; the top-k's [B, N] score matrix is written and read).
  pass    a whole validation pass (validation_epoch + validation_epoch_end: forward, scoring, metrics, the copies to the host) of SASRec on
          the synthetic-toys split, eval.rank_eval off and on, host clock around synchronised passes, alternating.
One JSON object on stdout and in --out (default profiles/eval_rank_bench.json).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CUTOFFS, TOPK = [20, 10], 100


def event_ms(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def stats(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(np.min(xs)), "rounds": len(xs)}


def bench_batch(B, N, D, Lh, rounds, iters, warmup):
    import torch
    from dr4sr_amd import _lib, evaluation
    lib = _lib.load()
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(N + D)
    q = torch.randn(B, D, generator=gen).to(dev)
    E = (0.05 * torch.randn(N, D, generator=gen)).to(dev)
    hist = torch.randint(1, N, (B, Lh), generator=gen).to(dev)
    target = torch.randint(1, N, (B,), generator=gen).to(dev)
    label = torch.ones(B, device=dev)
    # ---- top-k path
    nb_t = int(lib.dr4sr_full_score_topk_workspace_bytes(B, N))
    ws_t = torch.empty(nb_t // 4, dtype=torch.float32, device=dev)
    sc = torch.empty(B, TOPK, device=dev)
    ids = torch.empty(B, TOPK, dtype=torch.int64, device=dev)
    fns = evaluation.get_rank_metrics(["ndcg", "recall"])

    def topk_path():
        _lib.check(lib.dr4sr_full_score_topk_masked_ws(_lib.ptr(q), _lib.ptr(E), _lib.ptr(hist), None, _lib.ptr(sc), _lib.ptr(ids), B, D, N,
                                                       Lh, TOPK, _lib.ptr(ws_t), nb_t, _lib.cur_stream()), "topk")
        hit = target.view(-1, 1) == ids
        pos = label.view(-1, 1)
        return {f"{n}@{c}": fn(hit, pos, c) for c in CUTOFFS for n, fn in fns}
    # ---- rank path
    nb_r = int(lib.dr4sr_target_rank_workspace_bytes(B))
    ws_r = torch.empty(nb_r // 4, dtype=torch.int32, device=dev)
    rank = torch.empty(B, dtype=torch.int32, device=dev)
    acc = torch.zeros(1 + 7 * len(CUTOFFS), dtype=torch.float64, device=dev)
    cuts = (C.c_int32 * len(CUTOFFS))(*CUTOFFS)

    def rank_path():
        _lib.check(lib.dr4sr_target_rank(_lib.ptr(q), _lib.ptr(E), _lib.ptr(target), _lib.ptr(hist), None, _lib.ptr(rank), B, D, N, Lh,
                                         _lib.ptr(ws_r), nb_r, _lib.cur_stream()), "target_rank")
        _lib.check(lib.dr4sr_rank_metrics_accumulate(_lib.ptr(rank), _lib.ptr(label), B, cuts, len(CUTOFFS), TOPK, _lib.ptr(acc),
                                                     _lib.cur_stream()), "accumulate")

    def rank_only():
        _lib.check(lib.dr4sr_target_rank(_lib.ptr(q), _lib.ptr(E), _lib.ptr(target), _lib.ptr(hist), None, _lib.ptr(rank), B, D, N, Lh,
                                         _lib.ptr(ws_r), nb_r, _lib.cur_stream()), "target_rank")

    def topk_only():
        _lib.check(lib.dr4sr_full_score_topk_masked_ws(_lib.ptr(q), _lib.ptr(E), _lib.ptr(hist), None, _lib.ptr(sc), _lib.ptr(ids), B, D, N,
                                                       Lh, TOPK, _lib.ptr(ws_t), nb_t, _lib.cur_stream()), "topk")
    paths = {"topk": topk_path, "rank": rank_path, "topk_kernels_only": topk_only, "rank_kernels_only": rank_only}
    for fn in paths.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            times[k].append(event_ms(fn, iters))
    # the two paths agree on these tensors
    m = topk_path()
    acc.zero_()
    rank_path()
    a = acc.cpu()
    agree = {k: abs(float(v) - float(a[1 + 7 * CUTOFFS.index(int(k.split("@")[1])) + _lib.RANK_METRICS.index(k.split("@")[0])]) / B)
             for k, v in m.items()}
    lds_s = (N + 63) // 64 * 64
    inputs = B * D * 4 + N * D * 4 + B * Lh * 8
    return {
        "shape": {"B": B, "N": N, "D": D, "Lh": Lh, "k": TOPK, "cutoffs": CUTOFFS},
        "calls_per_path": rounds * iters,
        "time": {k: stats(v) for k, v in times.items()},
        "flops": 2 * B * N * D,
        "algorithmic_bytes": {"topk": inputs + 2 * B * lds_s * 4 + B * TOPK * 12, "rank": inputs + B * 8 + B * 4 + 2 * B * 8},
        "max_abs_metric_difference": max(agree.values()),
    }


def bench_pass(rounds):
    import torch
    from dr4sr_amd.utils import prepare_datasets, prepare_model, seed_everything
    cfg = {
        "data": {"dataset": "synthetic-toys", "domain_name_list": ["toy"], "max_seq_len": 50, "dataset_class": "synthetic", "train_file": ""},
        "model": {"model": "SASRec", "embed_dim": 64, "loss_fn": "bce", "hidden_size": 128, "layer_num": 2, "head_num": 2,
                  "dropout_rate": 0.5, "activation": "gelu", "layer_norm_eps": 1e-12},
        "train": {"batch_size": 256, "early_stop_mode": "max", "early_stop_patience": 20, "epochs": 1, "device": "cuda",
                  "optimizer": "adam", "learning_rate": 0.001, "weight_decay": 0, "num_neg": 1, "seed": 2023, "hip_graph": True},
        "eval": {"batch_size": 2048, "cutoff": [20, 10], "val_metrics": ["ndcg", "recall"], "test_metrics": ["ndcg", "recall"],
                 "topk": TOPK, "save_path": "./saved/"},
    }
    seed_everything(cfg["train"]["seed"])
    ds = prepare_datasets(cfg)
    model = prepare_model(cfg, ds)
    model._init_model(ds[0])
    model.eval()
    model.logged_metrics = {}                              # what fit_loop sets up per epoch: validation_epoch_end logs into it
    val = ds[1]
    val.set_eval_domain("toy")
    model.set_eval_domain("toy")

    def one(rank_eval):
        model.config["eval"]["rank_eval"] = rank_eval
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = model.validation_epoch(0, val.get_loader())
        out = model.validation_epoch_end(outs, "toy")
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out, sum(b for _, b in outs), len(outs)
    for re in (False, True, False, True):
        one(re)
    times = {False: [], True: []}
    for _ in range(rounds):
        for re in (False, True):
            ms, out, rows, nb = one(re)
            times[re].append(ms)
    _, off, rows, nb = one(False)
    _, on, _, _ = one(True)
    return {"model": "SASRec", "dataset": "synthetic-toys", "n_items": model.num_items, "rows": int(rows), "batches_topk_path": nb,
            "eval_batch": 2048, "time": {"topk": stats(times[False]), "rank": stats(times[True])},
            "metrics_topk": off, "metrics_rank": on}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_rank_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--pass-rounds", type=int, default=10)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    assert a.rounds * a.iters >= 200
    res = {"device": torch.cuda.get_device_name(0),
           "batch": [bench_batch(2048, 11925, 64, 50, a.rounds, a.iters, a.warmup), bench_batch(2048, 20034, 128, 50, a.rounds, a.iters, a.warmup)],
           "pass": bench_pass(a.pass_rounds)}
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
