#!/usr/bin/env python3
"""Measurement of the regenerator's pre-training pairs (dr4sr_amd.pairs, csrc/pairs.hip) on one GPU.

19 412 toys-shaped sequences (dr4sr_amd/data/synthetic.py) x a stand-in pattern list (sample_patterns below: ordered 2- to 4-item
subsequences drawn from the sequences themselves inside a window of 6 positions — NOT seq2pat's semantics), at each --patterns size:

  kernel_ms     the three launches of one dr4sr_pairs_match call between HIP events, median of --repeats after --warmup
  hip_api_s     match_and_choose(backend="hip"): packing, transfers, kernel, copy back
  pair_list_s   building the Python [sequence, pattern] lists of seq-pat-pair.pth from `chosen`
  numpy_s       match_and_choose(backend="numpy") on the first --numpy-rows sequences, scaled to all of them
  loop_s        the reference's loop (shuffle the whole list, is_sublist until ten hits; 1.Build_pretraining_dataset.py:70-89,
                restated here) on --loop-rows evenly spaced sequences, scaled to all of them
One JSON line per size on stdout and in --out.  --profile runs only the HIP path (for rocprofv3 --kernel-trace --stats).
"""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def toys_sequences(n_seq=19412, seed=2024, repeat_every=16):
    """toys-shaped training sequences (history up to seqlen + the last target).  The Zipf item draws repeat an id in under 1 % of the
    rows, so every repeat_every-th row also ends with a copy of its first id"""
    from dr4sr_amd.data.synthetic import make_rows
    d = make_rows(n_seq, seed=seed)
    sl = d["seqlen"]
    seqs = [d["in_item_id"][i, :sl[i]].tolist() + [int(d["item_id"][i, sl[i] - 1])] for i in range(n_seq) if sl[i] >= 1]
    for s in seqs[::repeat_every]:
        s[-1] = s[0]
    return seqs


def sample_patterns(seqs, n_pat, seed=0, span=5):
    """stand-in for mined patterns: n_pat distinct ordered subsequences of 2..4 ids, each taken from some sequence inside a window of
    span + 1 positions; every 50th one repeats its first id ([a, ..., a]) so that repeated ids are exercised"""
    rng = np.random.default_rng(seed)
    rows = [s for s in seqs if len(s) >= 2]
    weight = np.array([len(s) for s in rows], np.float64)
    out, seen = [], set()
    while len(out) < n_pat:
        pick = rng.choice(len(rows), size=n_pat, p=weight / weight.sum())
        n_ids = rng.choice([2, 3, 4], size=n_pat, p=[0.6, 0.3, 0.1])
        u = rng.random((n_pat, 2))
        for r, n, (ua, ub) in zip(pick.tolist(), n_ids.tolist(), u.tolist()):
            s = rows[r]
            a = int(ua * (len(s) - 1))
            win = s[a:a + span + 1]
            n = min(n, len(win))
            pos = sorted(random.Random(int(ub * 1e9)).sample(range(1, len(win)), n - 1))
            p = [win[0]] + [win[k] for k in pos]
            if len(out) % 50 == 49:
                p = p + [p[0]]
            t = tuple(p)
            if t not in seen:
                seen.add(t)
                out.append(p)
                if len(out) == n_pat:
                    break
    return out


def reference_loop(seqs, patterns, rows, seed=0):
    """1.Build_pretraining_dataset.py:70-89 on the given rows: seconds, pairs"""
    def is_sublist(sublst, lst):
        for element in sublst:
            try:
                ind = lst.index(element)
            except ValueError:
                return False
            lst = lst[ind + 1:]
        return True
    rnd = random.Random(seed)
    values = [list(p) for p in patterns]
    pairs = []
    t0 = time.perf_counter()
    for i in rows:
        rnd.shuffle(values)
        cnt = 0
        for p in values:
            if is_sublist(p, seqs[i]):
                pairs.append([seqs[i], p])
                cnt += 1
            if cnt == 10:
                break
    return time.perf_counter() - t0, pairs


def kernel_ms(seqs, patterns, seed, warmup, repeats, n_chunks=0):
    import torch
    from dr4sr_amd import _lib, pairs
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    seq_ids, seq_len = pairs.pack_sequences(seqs)
    pat_ids, pat_off = pairs.pack_patterns(patterns)
    S, Lmax, P = seq_ids.shape[0], seq_ids.shape[1], len(patterns)
    d = [torch.from_numpy(x).to(dev) for x in (seq_ids, seq_len, pat_ids, pat_off)]
    nb = int(lib.dr4sr_pairs_workspace_bytes(S, P, n_chunks))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    n_match = torch.empty(S, dtype=torch.int32, device=dev)
    chosen = torch.empty(S, pairs.N_CHOSEN, dtype=torch.int32, device=dev)

    def call():
        _lib.check(lib.dr4sr_pairs_match(_lib.ptr(d[0]), _lib.ptr(d[1]), S, Lmax, _lib.ptr(d[2]), _lib.ptr(d[3]), P, int(pat_ids.size),
                                         C.c_uint64(seed), 0, 0, n_chunks, C.c_void_p(ws.data_ptr()), nb, _lib.ptr(n_match), _lib.ptr(chosen),
                                         _lib.cur_stream()), "dr4sr_pairs_match")
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
    return float(np.median(times)), float(min(times)), n_match.cpu().numpy(), chosen.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", type=int, nargs="+", default=[25000, 250000])
    ap.add_argument("--n-seq", type=int, default=19412)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--numpy-rows", type=int, default=4096)
    ap.add_argument("--loop-rows", type=int, default=40)
    ap.add_argument("--chunks", type=int, nargs="+", default=[0], help="n_chunks values to time the kernel with (0: the library's choice)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from dr4sr_amd import pairs
    seqs = toys_sequences(a.n_seq)
    lines = []
    for n_pat in a.patterns:
        patterns = sample_patterns(seqs, n_pat, seed=1)
        if a.profile:
            kernel_ms(seqs, patterns, a.seed, 1, 3)
            continue
        r = {"metric": "pairs_match", "n_seq": len(seqs), "n_pat": n_pat, "mean_seq_len": round(float(np.mean([len(s) for s in seqs])), 2),
             "mean_pat_len": round(float(np.mean([len(p) for p in patterns])), 2)}
        for c in a.chunks:
            med, best, n_match, chosen = kernel_ms(seqs, patterns, a.seed, a.warmup, a.repeats, c)
            key = "kernel_ms" if c == 0 else f"kernel_ms_chunks{c}"
            r[key], r[key + "_min"] = round(med, 3), round(best, 3)
        r["pairs_per_s_kernel"] = round(len(seqs) * n_pat / (r["kernel_ms"] * 1e-3), 0) if "kernel_ms" in r else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nm, ch = pairs.match_and_choose(seqs, patterns, a.seed, "hip")
        r["hip_api_s"] = round(time.perf_counter() - t0, 4)
        t0 = time.perf_counter()
        pl = pairs.pair_list(seqs, patterns, ch)
        r["pair_list_s"] = round(time.perf_counter() - t0, 4)
        r["n_pairs"], r["n_matches"], r["max_m"] = len(pl), int(nm.sum()), int(nm.max())
        r["rows_m0"], r["rows_m_gt10"] = int((nm == 0).sum()), int((nm > 10).sum())
        nr = min(a.numpy_rows, len(seqs))
        t0 = time.perf_counter()
        nm2, ch2 = pairs.match_and_choose(seqs[:nr], patterns, a.seed, "numpy")
        t = time.perf_counter() - t0
        r["numpy_rows"], r["numpy_sample_s"], r["numpy_s"] = nr, round(t, 3), round(t * len(seqs) / nr, 2)
        r["numpy_equals_hip"] = bool(np.array_equal(nm2, nm[:nr]) and np.array_equal(ch2, ch[:nr]))
        rows = np.linspace(0, len(seqs) - 1, a.loop_rows).astype(int).tolist()
        t, ref_pairs = reference_loop(seqs, patterns, rows, a.seed)
        r["loop_rows"], r["loop_sample_s"], r["loop_s"] = len(rows), round(t, 3), round(t * len(seqs) / len(rows), 1)
        r["loop_seq_per_s"] = round(len(rows) / t, 2)
        r["loop_pairs_agree"] = bool(len(ref_pairs) == int(np.minimum(nm[rows], 10).sum()))
        r["speedup_kernel_vs_loop"] = round(r["loop_s"] / (r["kernel_ms"] * 1e-3), 0) if "kernel_ms" in r else None
        r["speedup_api_vs_loop"] = round(r["loop_s"] / (r["hip_api_s"] + r["pair_list_s"]), 1)
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
    if a.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
