#!/usr/bin/env python3
"""Measurement of the GRU4Rec training step at embed_dim 128 on one GPU -> profiles/gru_d128_bench.json (one JSON line per record).

Rows: amazon-beauty-shaped (N = 12 102) and yelp-shaped (N = 20 034) synthetic rows, L = 50, GRU 2 x 256, dropout 0.2, Adam with weight
decay 1e-4, in-kernel negatives, B = 256 and B = 8 192.  Per (rows, B) one record with four step times:
  d128_fused_us      D = 128, the fused glue kernels where the plan takes them (B L <= the latency boundary; above it the record says so)
  d128_separate_us   D = 128 with DR4SR_GRU_NOFUSE_GLUE=1 (the switch is read while the graph is captured)
  d64_us             D = 64, same build, same rows
  torch_fp32_us      fp32 torch on the same GPU with the reference's op sequence: nn.Embedding -> Dropout -> nn.GRU(bias=False) -> Linear ->
                     BCE scorer with one sampled negative -> Adam; padded [B, L] batch, eager
The library's steps run as a captured graph of --group steps (dr4sr_gru4rec_train_steps, as bench.py runs them), timed between HIP events;
the variants alternate inside every round so that clock drift hits them alike.  Round 0 warms up; every figure is the median over
--rounds rounds, min and max over rounds are kept as the spread.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, H, NL, P_DROP = 50, 256, 2, 0.2
ROWS = {"beauty": 12102, "yelp": 20034}


def stats(xs, key):
    return {key: round(float(np.median(xs)), 2), key + "_min": round(float(min(xs)), 2), key + "_max": round(float(max(xs)), 2)}


def hip_variant(torch, rows_np, N, D, B, group, nofuse):
    from dr4sr_amd import _lib
    from dr4sr_amd.gru_engine import GruEngine
    from dr4sr_amd.utils.graphs import capture as graph_capture
    dev = torch.device("cuda", 0)
    eng = GruEngine(N, L, D, H, NL, P_DROP, B, dev, seed=2023, lr=1e-3, weight_decay=1e-4)
    g = torch.Generator().manual_seed(2023)
    for k, v in eng.views.items():                                   # bench.py's initialisation
        v.copy_((torch.rand(v.shape, generator=g) * 2 - 1) / 16.0 if "gru" in k else 0.02 * torch.randn(v.shape, generator=g))
    eng.views["item_embedding.weight"][0] = 0
    data = {k: torch.from_numpy(rows_np[k]).to(dev) for k in ("in_item_id", "item_id", "seqlen")}
    U = int(data["seqlen"].shape[0])
    perm = torch.randperm(U, generator=torch.Generator().manual_seed(7)).to(dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    rows_buf = torch.zeros(B, dtype=torch.int64, device=dev)
    negbuf = torch.zeros(B * L, dtype=torch.int64, device=dev)
    plan = eng.make_plan(data["in_item_id"], data["item_id"], data["seqlen"], rows=rows_buf, neg_item=negbuf, sample_neg=True,
                         perm_sel=(perm, B, 0, counter))
    stream = torch.cuda.Stream(device=dev)
    _lib.set_env("DR4SR_GRU_NOFUSE_GLUE", "1" if nofuse else None)
    try:
        with torch.cuda.stream(stream):
            for _ in range(3):
                eng.train_step(plan)
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with graph_capture(graph, stream=stream):
                eng.train_steps(plan, group)
            stream.synchronize()
    finally:
        _lib.set_env("DR4SR_GRU_NOFUSE_GLUE", None)

    def run(reps):                                                   # (the batch index wraps modulo the permutation: no host work between replays)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            for _ in range(reps):
                graph.replay()
            e1.record()
            stream.synchronize()
        eng.check_device_error()
        return e0.elapsed_time(e1) * 1e3 / (reps * group)
    return run, (eng, plan, data, perm, counter, rows_buf, negbuf, graph)


def torch_variant(torch, rows_np, N, D, B):
    import torch.nn as nn
    import torch.nn.functional as F
    dev = torch.device("cuda", 0)
    torch.manual_seed(2023)
    emb = nn.Embedding(N, D, padding_idx=0).to(dev)
    drop = nn.Dropout(P_DROP)
    gru = nn.GRU(D, H, NL, bias=False, batch_first=True).to(dev)
    lin = nn.Linear(H, D).to(dev)
    params = list(emb.parameters()) + list(gru.parameters()) + list(lin.parameters())
    opt = torch.optim.Adam(params, lr=1e-3, weight_decay=1e-4)
    data = {k: torch.from_numpy(rows_np[k]).to(dev) for k in ("in_item_id", "item_id")}
    U = int(data["in_item_id"].shape[0])
    state = {"i": 0}

    def step():
        lo = (state["i"] * B) % max(1, U - B + 1)
        state["i"] += 1
        idx, tgt = data["in_item_id"][lo:lo + B], data["item_id"][lo:lo + B]
        neg = torch.randint(1, N, tgt.shape, device=dev)
        q = lin(gru(drop(emb(idx)))[0])
        pos = (q * emb.weight[tgt]).sum(-1)
        ng = (q * emb.weight[neg]).sum(-1)
        live = (tgt != 0).float()
        loss = ((F.softplus(-pos) + F.softplus(ng)) * live).sum() / live.sum()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()

    def run(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=40, help="graph replays (library) per timed section")
    ap.add_argument("--group", type=int, default=10, help="steps per captured graph")
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 8192])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru_d128_bench.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    torch.cuda.set_device(0)
    from dr4sr_amd.data.synthetic import make_rows
    lines = []
    for name, N in ROWS.items():
        for B in a.batches:
            rows_np = make_rows(n_rows=max(19412, 3 * B), n_items=N, seed=2024)
            group = a.group if B <= 1024 else max(1, a.group // 5)
            inner = a.inner if B <= 1024 else max(1, a.inner // 5)
            keep = []
            runs = {}
            for key, D, nofuse in (("d128_fused_us", 128, False), ("d128_separate_us", 128, True), ("d64_us", 64, False)):
                runs[key], k = hip_variant(torch, rows_np, N, D, B, group, nofuse)
                keep.append(k)
            torch_run = torch_variant(torch, rows_np, N, 128, B)
            times = {k: [] for k in list(runs) + ["torch_fp32_us"]}
            for r in range(a.rounds + 1):                            # round 0 warms every variant up
                for k, run in runs.items():
                    t = run(inner)
                    if r:
                        times[k].append(t)
                t = torch_run(max(2, inner * group // 10))
                if r:
                    times["torch_fp32_us"].append(t)
            rec = {"metric": "gru4rec_d128_step", "rows": name, "n_items": N, "B": B, "L": L, "hidden": H, "layers": NL, "dropout": P_DROP,
                   "fused_glue_applies": bool(B * L <= 16384), "rounds": a.rounds, "steps_per_graph": group, "replays_per_section": inner}
            for k in times:
                rec.update(stats(times[k], k))
            rec["separate_over_fused"] = round(rec["d128_separate_us"] / rec["d128_fused_us"], 4)
            rec["d128_over_d64"] = round(rec["d128_fused_us"] / rec["d64_us"], 4)
            rec["torch_over_d128"] = round(rec["torch_fp32_us"] / rec["d128_fused_us"], 2)
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
            del keep, runs
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
