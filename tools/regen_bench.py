#!/usr/bin/env python3
"""Measurement of dataset regeneration (dr4sr_amd.regen): one JSON line for N toys-shaped sources x K conditions.

  hip_s          the HIP path (dr4sr_regen_encode + _decode per chunk of rows, tokens copied to the host), after a warm-up, synced
  hip_api_s      the same through RegenModel.decode (+ the host-side token lists)
  torch_s        the batched eager restatement (backend="torch") on the same GPU
  loop_est_s     the reference's way — one (source, condition) at a time, a host sync per token — timed on --loop-sample decodes
                 and extrapolated to N x K
  agree          with --check: the fraction of rows whose HIP and torch tokens are identical

Model: a seeded random regenerator (random_state_dict, the default), or --fixture tests/golden/regen_toys.npz (a trained one).

Usage:  python tools/regen_bench.py [--n 19412] [--fixture PATH] [--check] [--no-torch] [--loop-sample 200]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def sources(n, n_item, seed):
    g = np.random.default_rng(seed)
    lens = np.minimum(g.geometric(1 / 9.0, n), 47)
    return [[n_item] + g.integers(1, n_item, int(l) + 1).tolist() + [n_item + 1] for l in lens]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=19412)
    ap.add_argument("--fixture", default=None)
    ap.add_argument("--std", type=float, default=0.1)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--loop-sample", type=int, default=200)
    a = ap.parse_args()
    from dr4sr_amd import regen, regen_torch
    dev = torch.device("cuda", 0)
    if a.fixture:
        z = np.load(a.fixture)
        sd = {k: torch.from_numpy(z[f"p:{k}"].astype(np.float32)) for k in regen.param_names()}
        model_name = os.path.basename(a.fixture)
    else:
        sd = regen.random_state_dict(seed=0, std=a.std)
        model_name = f"random(seed 0, std {a.std})"
    m = regen.RegenModel.from_state_dict(sd, dev)
    src_list = sources(a.n, m.n_item, 1)
    src, lens = m._pack(src_list)
    K = m.K
    chunk = max(1, regen.ROWS_PER_CALL // K)

    def run_hip():
        out = []
        for s0 in range(0, a.n, chunk):
            s1 = min(a.n, s0 + chunk)
            Lc = int(lens[s0:s1].max())
            out.append(m._decode_hip(src[s0:s1, :Lc].contiguous(), lens[s0:s1].contiguous(), 0, K))
        torch.cuda.synchronize()
        return out

    m._decode_hip(src[:64, :int(lens[:64].max())].contiguous(), lens[:64].contiguous(), 0, K)      # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hip_out = run_hip()
    hip_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    hip_tok = m.decode(src_list, backend="hip")
    hip_api_s = time.perf_counter() - t0
    mean_len = float(np.mean([len(t) for t in hip_tok]))
    res = {"metric": "regen_decode", "n_seq": a.n, "K": K, "rows": a.n * K, "n_rows_table": m.n_rows, "model": model_name,
           "hip_s": round(hip_s, 4), "hip_api_s": round(hip_api_s, 4), "mean_tokens": round(mean_len, 3)}
    if not a.no_torch:
        m.decode(src_list[:64], backend="torch")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch_tok = m.decode(src_list, backend="torch")
        torch.cuda.synchronize()
        res["torch_s"] = round(time.perf_counter() - t0, 4)
        res["speedup_vs_torch"] = round(res["torch_s"] / hip_s, 2)
        if a.check:
            res["agree"] = sum(x == y for x, y in zip(hip_tok, torch_tok)) / len(hip_tok)
    if a.loop_sample > 0:
        g = np.random.default_rng(2)
        picks = g.integers(0, a.n, a.loop_sample)
        conds = g.integers(0, K, a.loop_sample)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, c in zip(picks, conds):
            regen_torch.decode(m, src[i:i + 1, :int(lens[i])], lens[i:i + 1], int(c), 1)
        torch.cuda.synchronize()
        per = (time.perf_counter() - t0) / a.loop_sample
        res["loop_per_decode_s"] = round(per, 5)
        res["loop_est_s"] = round(per * a.n * K, 1)
        res["speedup_vs_loop"] = round(per * a.n * K / hip_s, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
