#!/usr/bin/env python3
"""Golden fixture of the pattern miner (tests/golden/mine_toys.npz): the shipped amazon-toys seq2pat_data.pth and what the brute-force
statement of the mining rule (tests/_mine_ref.py) finds in it at alpha = 5, beta = 2.

Works only where the reference checkout (USTC-StarTeam/DR4SR) exists: the sequences are its data file.  seq2pat itself is installed
nowhere this project builds, so the expected patterns come from this project's own plain statement of the rule, NOT from a seq2pat run.
Only DATA is written: ids (uint16: toys has 11 924 items) + offsets, and the patterns as zero padded rows + frequencies, in result order.

Usage:  python tools/make_mine_golden.py [--out tests/golden/mine_toys.npz]
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from make_golden import REF  # noqa: E402  (where the reference checkout lives)
from _mine_ref import brute_force  # noqa: E402

TOYS = os.path.join(REF, "dataset", "amazon-toys", "toy")
ALPHA, BETA = 5, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "mine_toys.npz"))
    a = ap.parse_args()
    import torch
    seqs = [[int(v) for v in s] for s in torch.load(os.path.join(TOYS, "seq2pat_data.pth"), weights_only=False)]
    lens = np.array([len(s) for s in seqs], np.int64)
    ids = np.array([v for s in seqs for v in s], np.int64)
    assert ids.min() >= 1 and ids.max() < 2 ** 16
    t0 = time.perf_counter()
    mined = brute_force(seqs, ALPHA, BETA)
    print(f"{len(seqs)} sequences, {ids.size} ids, longest {lens.max()}: {len(mined)} patterns in {time.perf_counter() - t0:.1f} s")
    pat = np.zeros((len(mined), ALPHA), np.uint16)
    for j, p in enumerate(mined):
        pat[j, :len(p) - 1] = p[:-1]
    freq = np.array([p[-1] for p in mined], np.int32)
    k = (pat != 0).sum(1)
    print({int(n): int((k == n).sum()) for n in range(2, ALPHA + 1)}, "largest frequency", int(freq.max()))
    np.savez_compressed(a.out, ids=ids.astype(np.uint16), off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
                        pat_ids=pat, pat_freq=freq, alpha=np.int32(ALPHA), beta=np.int32(BETA))
    size = os.path.getsize(a.out)
    print(a.out, size, "bytes")
    assert size < (1 << 20)


if __name__ == "__main__":
    main()
