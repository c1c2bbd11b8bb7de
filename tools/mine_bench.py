#!/usr/bin/env python3
"""Measurement of the pattern miner (dr4sr_amd.mine, csrc/mine.hip) on one GPU.

Inputs: the toys fixture (tests/golden/mine_toys.npz: the shipped seq2pat_data.pth, 19 412 sequences) at alpha 5 and 8, and a synthetic
set of 8 x as many toys-shaped sequences (dr4sr_amd/data/synthetic.py, markov 0.5 so that there is something to find) at alpha 5;
beta 2 everywhere.  Per input, one JSON line on stdout and in --out:

  device_ms          one dr4sr_mine_patterns call (its three launches: clear, count, extract) between HIP events on a synchronised
                     stream, median (and minimum) of --repeats after --warmup, with the default table
  hip_s              mine_patterns(backend="hip") by the host clock: packing, transfers, the call, copy back, ordering, Python lists
  numpy_s, brute_s   mine_patterns(backend="numpy") and the brute-force statement of the rule (tests/_mine_ref.py) on the same host
  load_factor, mean_probe_length   of the finished table (taken slots / slots; 1 + mean distance of a tuple from its home slot)
seq2pat itself is installed nowhere this project runs, so it is not timed.  --profile runs only the HIP path.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
BETA = 2


def fixture_sequences():
    z = np.load(os.path.join(ROOT, "tests", "golden", "mine_toys.npz"))
    ids, off = z["ids"].astype(np.int64).tolist(), z["off"].tolist()
    return [ids[a:b] for a, b in zip(off[:-1], off[1:])]


def synthetic_sequences(n_seq, seed=2024):
    from dr4sr_amd.data.synthetic import make_rows
    d = make_rows(n_seq, seed=seed, markov=0.5)
    sl = d["seqlen"]
    return [d["in_item_id"][i, :sl[i]].tolist() + [int(d["item_id"][i, sl[i] - 1])] for i in range(n_seq) if sl[i] >= 1]


def device_ms(ids, off, alpha, warmup, repeats):
    """-> (median ms, min ms, n_out, stats of the table) of the call with the default table and room for every pattern"""
    import torch
    from dr4sr_amd import _lib, mine
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    slots = mine.table_slots_for(mine.candidate_count(off, alpha))
    nb = int(lib.dr4sr_mine_workspace_bytes(ids.size, len(off) - 1, alpha, slots))
    d_ids, d_off = torch.from_numpy(ids).to(dev), torch.from_numpy(off).to(dev)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    cap = max(1, min(mine.candidate_count(off, alpha), 1 << 22))
    out_ids = torch.empty(cap, alpha, dtype=torch.int32, device=dev)
    out_freq = torch.empty(cap, dtype=torch.int32, device=dev)
    n_out = torch.empty(1, dtype=torch.int32, device=dev)
    status = torch.empty(4, dtype=torch.int64, device=dev)

    def call():
        _lib.check(lib.dr4sr_mine_patterns(_lib.ptr(d_ids), _lib.ptr(d_off), ids.size, len(off) - 1, alpha, BETA, slots,
                                           C.c_void_p(ws.data_ptr()), nb, _lib.ptr(out_ids), _lib.ptr(out_freq), cap, _lib.ptr(n_out),
                                           _lib.ptr(status), _lib.cur_stream()), "dr4sr_mine_patterns")
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    st = status.tolist()
    assert st[0] == 0 and int(n_out) <= cap
    return float(np.median(times)), float(min(times)), int(n_out), {"table_slots": slots, "distinct_tuples": st[1],
                                                                    "load_factor": round(st[1] / slots, 4),
                                                                    "mean_probe_length": round(1.0 + st[2] / max(st[1], 1), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=8, help="the synthetic set has this many times the fixture's sequences")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--no-brute", action="store_true")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "mine_bench.py measures the GPU path: no GPU, no numbers"
    from _mine_ref import brute_force
    from dr4sr_amd import mine
    fixture = fixture_sequences()
    inputs = [("toys_fixture", fixture, 5), ("toys_fixture", fixture, 8), (f"synthetic_x{a.scale}", synthetic_sequences(a.scale * len(fixture)), 5)]
    lines = []
    for name, seqs, alpha in inputs:
        ids, off = mine.pack(seqs)
        if a.profile:
            device_ms(ids, off, alpha, 1, 3)
            continue
        r = {"metric": "mine_patterns", "input": name, "alpha": alpha, "beta": BETA, "n_seq": len(seqs), "n_ids": int(ids.size),
             "longest": int(np.diff(off).max()), "candidates": mine.candidate_count(off, alpha)}
        med, best, n, stats = device_ms(ids, off, alpha, a.warmup, a.repeats)
        r.update(device_ms=round(med, 3), device_ms_min=round(best, 3), launches=3, n_patterns=n, **stats)
        mine.mine_patterns(seqs[:100], alpha, BETA, "hip")
        torch.cuda.synchronize()
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            got = mine.mine_patterns(seqs, alpha, BETA, "hip")
            times.append(time.perf_counter() - t0)
        r["hip_s"], r["hip_s_min"] = round(float(np.median(times)), 4), round(min(times), 4)
        t0 = time.perf_counter()
        ref = mine.mine_patterns(seqs, alpha, BETA, "numpy")
        r["numpy_s"] = round(time.perf_counter() - t0, 3)
        r["hip_equals_numpy"] = got == ref and len(got) == n
        if not a.no_brute:
            t0 = time.perf_counter()
            bf = brute_force(seqs, alpha, BETA)
            r["brute_s"] = round(time.perf_counter() - t0, 3)
            r["hip_equals_brute"] = got == bf
        r["hip_faster_than_numpy"] = r["hip_s"] < r["numpy_s"]
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
    if a.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
