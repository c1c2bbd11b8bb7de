#!/usr/bin/env python3
"""Measurement of teacher-forced regenerator scoring (RegenModel.score, csrc/regen_score.hip) on one GPU.

Toys-shaped pairs: 19 412 sequences (tools/pairs_bench.py toys_sequences, cut to their last 48 ids: the position table has 50 rows)
x up to 10 patterns each (ordered subsequences of 2..4 of the sequence's ids), K = 5, a random regenerator with a condition encoder.
Mode "all" scores every pair under the 5 one-hot conditions: about a million score rows.

  hip_ms        every launch of the whole file (condition logits + dr4sr_regen_score, PAIRS_PER_CALL pairs per call, tensors already
                on the device) between HIP events: median of --repeats after --warmup
  torch_ms      backend="torch" (fp32 eager) on the same GPU over the same device tensors, ROWS_PER_TORCH pairs per batch
One JSON line on stdout and in --out.  --profile runs only the HIP path once (for rocprofv3 --kernel-trace --stats); --stats-csv
folds that run's kernel statistics into the JSON.
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def toys_pairs(n_seq, seed=0):
    from pairs_bench import toys_sequences
    rng = np.random.default_rng(seed)
    pairs = []
    for s in toys_sequences(n_seq):
        s = s[-48:]
        if len(s) < 2:
            continue
        for _ in range(10 if len(s) >= 4 else 2 * len(s)):
            k = min(int(rng.choice([2, 3, 4], p=[0.6, 0.3, 0.1])), len(s))
            pos = sorted(rng.choice(len(s), k, replace=False).tolist())
            pairs.append([s, [s[p] for p in pos]])
    return pairs


def median_ms(torch, fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(min(times)), float(max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-seq", type=int, default=19412)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--torch-repeats", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--stats-csv", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from dr4sr_amd import regen, regen_torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    m = regen.RegenModel.from_state_dict(regen.random_state_dict(seed=3, std=0.3, condition_encoder=True), dev)
    pairs = toys_pairs(a.n_seq)
    src, src_len, tgt, tgt_len, Ls, T = m._pack_pairs(pairs, None)
    n = len(pairs)
    eye = torch.eye(m.K, device=dev)

    def chunks(step):
        out = []
        for lo in range(0, n, step):
            hi = min(n, lo + step)
            out.append([t[lo:hi].to(dev).contiguous() for t in (src, src_len, tgt, tgt_len)]
                       + [eye[:, None, :].expand(m.K, hi - lo, m.K).contiguous()])
        return out

    hip_chunks = chunks(regen.PAIRS_PER_CALL)
    lib_ws = {}

    def run_hip():
        for s, sl, t, tl, w in hip_chunks:
            key = s.shape[0]
            if key not in lib_ws:
                lib_ws[key] = torch.empty(int(regen._lib.load().dr4sr_regen_score_workspace_bytes(
                    regen.C.byref(m.score_plan()), key, Ls, T, m.K)), dtype=torch.uint8, device=dev)
            m.condition_device(t, tl, lib_ws[key])
            m.score_device(s, sl, t, tl, w, True, lib_ws[key])

    r = {"metric": "regen_score", "pairs": n, "score_rows": n * m.K, "live_tokens": int((tgt[:, 1:] != 0).sum()) * m.K, "K": m.K,
         "width": [Ls, T], "mean_src_len": round(float(src_len.double().mean()), 2), "mean_tgt_len": round(float(tgt_len.double().mean()), 2),
         "pairs_per_call": regen.PAIRS_PER_CALL}
    if a.profile:
        run_hip()
        run_hip()
        torch.cuda.synchronize()
        return
    med, lo, hi = median_ms(torch, run_hip, a.warmup, a.repeats)
    r.update(hip_ms=round(med, 3), hip_ms_min=round(lo, 3), hip_ms_max=round(hi, 3), repeats=a.repeats,
             score_rows_per_s=round(n * m.K / (med * 1e-3), 0))
    if not a.no_torch:
        torch_chunks = chunks(regen.ROWS_PER_TORCH)

        def run_torch():
            with torch.no_grad():
                for s, sl, t, tl, w in torch_chunks:
                    regen_torch.score_forward(m, s, t, tl, w, True, True, torch.float32)

        med_t, lo_t, hi_t = median_ms(torch, run_torch, 1, a.torch_repeats)
        r.update(torch_ms=round(med_t, 3), torch_ms_min=round(lo_t, 3), torch_ms_max=round(hi_t, 3), torch_repeats=a.torch_repeats,
                 hip_speedup_vs_torch=round(med_t / med, 2))
    else:
        r["torch_ms"] = None
    if a.stats_csv and os.path.exists(a.stats_csv):
        with open(a.stats_csv) as f:
            rows = list(csv.DictReader(f))
        r["kernel_split"] = [{k: row[k] for k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage") if k in row} for row in rows[:8]]
    else:
        r["kernel_split"] = None
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
