#!/usr/bin/env python3
"""Measurement of the GNN model's propagation (dr4sr_gnn_propagate, csrc/gnn.hip) and of its training step on one GPU.

Graph: the 'new' graph (window 2) of the toys-shaped synthetic training rows (dr4sr_amd/data/synthetic.py: N = 11 925 items, 19 412 rows).
  propagate   forward (E -> G) + backward (dG -> dE, accumulate) of 3 hops at D = 64 between HIP events, against the reference's op on the
              same device and data: torch.sparse.mm forward (the mean of the stacked powers, model/gnn.py:43-50) + its autograd backward.
              The two are timed in alternating rounds inside one process; median and minimum of the per-round means are reported, and the
              outputs are compared.  The forward alone at 1, 2 and 3 hops gives, by a line through the three times, the cost of a hop and
              the cost every call pays whatever its hops (the launch that derives the chunk list, k_gnn_plan).
  step        ms per GNN API step (batch 256, dropout 0.5), eager and captured (train.hip_graph), beside SASRec's API-path step
              (DR4SR_NO_FAST_PATH=1: the reference-shaped loop, what the GNN's step is built from) — host clock around synchronised windows.
One JSON object on stdout and in --out (default profiles/gnn_bench.json).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def config(model, batch=256, hip_graph=True):
    return {
        "data": {"dataset": "synthetic-toys", "domain_name_list": ["toy"], "max_seq_len": 50, "dataset_class": "synthetic",
                 "train_file": "", "n_eval_rows": 256},
        "model": {"model": model, "embed_dim": 64, "loss_fn": "bce", "hidden_size": 128, "layer_num": 2, "head_num": 2,
                  "dropout_rate": 0.5, "activation": "gelu", "layer_norm_eps": 1e-12, "graph": "new", "gnn_layer": 3, "window": 2},
        "train": {"batch_size": batch, "early_stop_mode": "max", "early_stop_patience": 20, "epochs": 1, "device": "cuda",
                  "optimizer": "adam", "learning_rate": 0.001, "weight_decay": 0, "num_neg": 1, "seed": 2023, "hip_graph": hip_graph},
        "eval": {"batch_size": 256, "cutoff": [20, 10], "val_metrics": ["ndcg", "recall"], "test_metrics": ["ndcg", "recall"],
                 "topk": 100, "save_path": "./saved/"},
    }


def build(cfg):
    from dr4sr_amd.utils import prepare_datasets, prepare_model, seed_everything
    seed_everything(cfg["train"]["seed"])
    ds = prepare_datasets(cfg)
    model = prepare_model(cfg, ds)
    model._init_model(ds[0])
    model.train()
    return ds, model


def event_ms(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def bench_propagate(model, rounds, iters, warmup):
    import torch
    row_ptr, col, val = model.query_encoder.norm_adj
    N, D, k = model.num_items, model.embed_dim, model.gnn_layer
    dev = model.device
    gen = torch.Generator().manual_seed(1)
    E = (0.02 * torch.randn(N, D, generator=gen)).to(dev)
    dG = torch.randn(N, D, generator=gen).to(dev)
    G, dE = torch.empty_like(E), torch.zeros_like(E)

    def hip():
        model._propagate(E, G, 0)
        model._propagate(dG, dE, 1)
    row = torch.repeat_interleave(torch.arange(N, device=dev), row_ptr[1:] - row_ptr[:-1])
    A = torch.sparse_coo_tensor(torch.stack([row, col.long()]), val, (N, N)).coalesce()        # the reference's operand: coalesced COO
    Et = E.clone().requires_grad_(True)

    def ref():
        emb, embs = Et, [Et]
        for _ in range(k):
            emb = torch.sparse.mm(A, emb)
            embs.append(emb)
        out = torch.stack(embs, dim=1).mean(1)
        Et.grad = None
        out.backward(dG)
        return out
    for _ in range(warmup):
        hip()
        ref()
    torch.cuda.synchronize()
    dE.zero_()
    hip()
    out_ref = ref()
    agree = {"G_rel": float((G - out_ref.detach()).abs().max() / out_ref.detach().abs().max()),
             "dE_rel": float((dE - Et.grad).abs().max() / Et.grad.abs().max())}
    t_hip, t_ref = [], []
    for _ in range(rounds):                                   # alternating rounds in one process
        t_hip.append(event_ms(hip, iters))
        t_ref.append(event_ms(ref, iters))
    # forward alone at 1, 2, 3 hops: t(k) = per_call + k * per_hop
    from dr4sr_amd import _lib
    lib = model.engine.lib

    def fwd(k_):
        _lib.check(lib.dr4sr_gnn_propagate(_lib.ptr(row_ptr), _lib.ptr(col), _lib.ptr(val), N, D, k_, _lib.ptr(E), _lib.ptr(G), 0,
                                           _lib.ptr(model._gnn_ws), model._gnn_ws_bytes, _lib.cur_stream()), "dr4sr_gnn_propagate")
    t_k = {}
    for k_ in (1, 2, 3):
        fwd(k_)
        t_k[k_] = float(np.median([event_ms(lambda: fwd(k_), iters) for _ in range(rounds)]))
    per_hop = (t_k[3] - t_k[1]) / 2.0
    per_call = t_k[1] - per_hop
    deg = (row_ptr[1:] - row_ptr[:-1]).cpu().numpy()
    nnz = int(col.numel())
    gather_bytes = 2 * k * (nnz * (D * 4 + 8) + 3 * N * D * 4)        # per fwd + bwd: every edge reads one source row + its (col, val); S / cur / out traffic
    med = float(np.median(t_hip))
    return {"n_items": N, "rows": int(model.dataset_list[0].data[1].shape[0]), "nnz": nnz, "degree_max": int(deg.max()),
            "degree_median": float(np.median(deg)), "rows_split": int((deg > model.engine.lib.dr4sr_gnn_split_rows()).sum()),
            "D": D, "n_hop": k, "iters": rounds * iters,
            "hip_fwd_bwd_ms": round(med, 4), "hip_fwd_bwd_ms_min": round(float(min(t_hip)), 4),
            "torch_sparse_mm_fwd_bwd_ms": round(float(np.median(t_ref)), 4), "torch_sparse_mm_fwd_bwd_ms_min": round(float(min(t_ref)), 4),
            "speedup_vs_torch_sparse_mm": round(float(np.median(t_ref)) / med, 2),
            "hip_fwd_ms_by_hops": {str(k_): round(v, 4) for k_, v in t_k.items()}, "hip_per_hop_ms": round(per_hop, 4),
            "hip_per_call_ms": round(per_call, 4), "per_call_share_of_3_hop_fwd": round(per_call / t_k[3], 3),
            "algorithmic_bytes": gather_bytes, "algorithmic_GBps": round(gather_bytes / (med * 1e-3) / 1e9, 1), "agreement": agree}


def step_ms(step, batches, warmup, steps):
    import torch
    for i in range(warmup):
        step(batches[i % len(batches)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        step(batches[i % len(batches)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gnn_bench.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "gnn_bench.py measures on a GPU; it has no CPU fall-back"
    from dr4sr_amd.model.basemodel import BaseModel
    res = {"metric": "gnn_bench", "device": torch.cuda.get_device_name(0)}
    ds, gnn = build(config("GNN", hip_graph=True))
    res["propagate"] = bench_propagate(gnn, a.rounds, a.iters, a.warmup)
    batches = [b for b, _ in zip(ds[0].get_loader(shuffle=False), range(16))]             # 16 full batches of 256
    res["step"] = {"batch": 256, "steps": a.steps}
    res["step"]["gnn_eager_ms"] = round(step_ms(gnn._api_step_body, batches, a.warmup, a.steps), 4)
    res["step"]["gnn_captured_ms"] = round(step_ms(gnn._api_step_graph, batches, a.warmup, a.steps), 4)
    res["step"]["gnn_eager_autograd_ms"] = round(step_ms(lambda b: BaseModel._api_step_body(gnn, b), batches, a.warmup, a.steps), 4)
    del gnn
    # the captured step with the reference-shaped (autograd) loop body inside the graph, on a model of its own
    ds1, gnn1 = build(config("GNN", hip_graph=True))
    gnn1._api_step_body = lambda b: BaseModel._api_step_body(gnn1, b)
    try:
        res["step"]["gnn_captured_autograd_ms"] = round(step_ms(gnn1._api_step_graph, batches, a.warmup, a.steps), 4)
    except Exception as e:      # noqa: BLE001 — recorded, not fatal: the figure is a comparison, the shipped step is measured above
        res["step"]["gnn_captured_autograd_ms"] = None
        res["step"]["gnn_captured_autograd_error"] = f"{type(e).__name__}: {e}"[:300]
    del gnn1
    os.environ["DR4SR_NO_FAST_PATH"] = "1"
    ds2, sas = build(config("SASRec", hip_graph=True))
    assert not sas._fast_path_ok()
    batches2 = [b for b, _ in zip(ds2[0].get_loader(shuffle=False), range(16))]
    res["step"]["sasrec_api_path_ms"] = round(step_ms(lambda b: BaseModel._api_step_body(sas, b), batches2, a.warmup, a.steps), 4)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
