#!/usr/bin/env python3
"""Golden fixture of the regenerator's pre-training pairs (tests/golden/pairs_toys.npz) by RUNNING the reference's stage 1 script.

Works only where the reference checkout (USTC-StarTeam/DR4SR) exists.  1.Build_pretraining_dataset.py is exec'd unmodified (the way
tools/make_regen_golden.py runs stages 2 and 3).  The seq2pat library it imports is not installed anywhere this project builds, so a
stand-in `sequential.seq2pat` module is defined below whose Seq2Pat.get_patterns returns this tool's own pattern list; `random` is
seeded before the run.  Only DATA is written, as integer arrays.

  rows      the first 400 REAL amazon-toys training rows, rebuilt from the shipped seq2pat_data.pth (every user's chronological items
            minus the last two: history = s[:-1], target = s[1:], each cut to its last 50 — tools/make_golden.py build_real_toys, with
            the cut applied to the row so that users with more than 50 training items give rows of the full 51 ids), plus hand-made
            rows with repeated ids (no real row among the 400 repeats an id).
  patterns  this tool's simple miner over the whole seq2pat_data.pth: every ordered 2- and 3-item subsequence whose first and last
            positions are at most 5 apart and that occurs in at least 2 sequences (24 045 of them), plus hand-made patterns with
            repeated ids, one pattern of 51 ids equal to a whole row and one longer than every row.  NOT seq2pat's semantics.
  matches   the complete relation, computed with the reference's own is_sublist taken from the exec'd globals, as sorted (i, j).
  files     the reference's patterns.pth rows (as arrays) and the seq-pat-pair.pth it drew, as (row, pattern) indices.

Usage:  python tools/make_pairs_golden.py [--out tests/golden/pairs_toys.npz]
"""
import argparse
import collections
import itertools
import os
import random
import sys
import tempfile
import textwrap
import types

import numpy as np

L = 50
N_REAL = 400
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF  # noqa: E402  (where the reference checkout lives)

TOYS = os.path.join(REF, "dataset", "amazon-toys", "toy")


def mine(seqs, span=5, lengths=(2, 3), min_frequency=2):
    """stand-in miner: ordered subsequences of the given lengths inside a window of span + 1 positions, with their sequence counts"""
    cnt = collections.Counter()
    for q in seqs:
        seen = set()
        for a in range(len(q)):
            hi = min(len(q), a + span + 1)
            for n in lengths:
                for rest in itertools.combinations(range(a + 1, hi), n - 1):
                    seen.add((q[a],) + tuple(q[r] for r in rest))
        cnt.update(seen)
    return [list(p) + [c] for p, c in cnt.items() if c >= min_frequency]


def row_of(user, s):
    h, t = list(s[:-1])[-L:], list(s[1:])[-L:]
    sl = len(h)
    return [user, h + [0] * (L - sl), t + [0] * (L - sl), sl, [1] * sl + [0] * (L - sl), [0] * L]


def hand_made():
    a, b, c = 1, 2, 3
    seqs = [[a, b], [a, a], [a, b, a], [a, a, b], [b, a, a, b, a], [a, b, c, a, b, c], [a] * 5, [b, a, b, a, b], [c, b, a, c],
            [a, b, c] * 17, [c] * 51]
    pats = [[a, a], [a, b, a], [a, a, b], [a, a, a], [b, a, b, a], [a, b, c, a, b, c], [c, c], [a] * 6, [a], [b, b, b],
            [a, b, c] * 17, [c] * 51, [c] * 52, [c, a, b, c]]
    return seqs, pats


def fixture_conditions(n_match, lens):
    """what the fixture must cover (asserted again by tests/test_pairs_cpu.py)"""
    n_match, lens = np.asarray(n_match), np.asarray(lens)
    got = {"m0": int((n_match == 0).sum()), "m1_9": int(((n_match >= 1) & (n_match <= 9)).sum()), "m10": int((n_match == 10).sum()),
           "m_gt10": int((n_match > 10).sum()), "m_max": int(n_match.max()), "len51": int((lens == 51).sum())}
    ok = got["m0"] >= 50 and got["m1_9"] >= 100 and got["m10"] >= 1 and got["m_gt10"] >= 50 and got["m_max"] >= 500 and got["len51"] >= 20
    return ok, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "tests", "golden", "pairs_toys.npz"))
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import torch
    users = torch.load(os.path.join(TOYS, "seq2pat_data.pth"), weights_only=False)
    hand_seqs, hand_pats = hand_made()
    train = [row_of(u, s) for u, s in enumerate(users[:N_REAL], start=1)]
    train += [row_of(N_REAL + 1 + k, s) for k, s in enumerate(hand_seqs)]
    mined = mine(users)
    have = {tuple(p[:-1]) for p in mined}
    mined += [list(p) + [2] for p in hand_pats if tuple(p) not in have]
    assert len({tuple(p[:-1]) for p in mined}) == len(mined)
    print(f"{len(train)} rows, {len(mined)} patterns")

    # ---- the stand-in `sequential` package: hands the list above to the script
    class Seq2Pat:
        def __init__(self, sequences, n_jobs=2, max_span=5):
            self.sequences = sequences

        def get_patterns(self, min_frequency=2):
            return [list(p) for p in mined]

    pkg, mod = types.ModuleType("sequential"), types.ModuleType("sequential.seq2pat")
    mod.Seq2Pat = Seq2Pat
    pkg.seq2pat = mod
    sys.modules["sequential"], sys.modules["sequential.seq2pat"] = pkg, mod

    root = tempfile.mkdtemp(prefix="pairs_golden_")
    torch.save([list(s) for s in users[:8]], os.path.join(root, "seq2pat_data.pth"))      # only its length is printed; mining is the stub's
    torch.save(train, os.path.join(root, "train.pth"))
    name = "1.Build_pretraining_dataset.py"
    head, body = open(os.path.join(REF, name)).read().split("if __name__ == '__main__':", 1)
    g = {"__name__": "pairs_reference", "__file__": os.path.join(REF, name)}
    sys.argv = [name, "--root_path", root]
    random.seed(a.seed)
    exec(compile(head, name, "exec"), g)
    exec(compile(textwrap.dedent(body), name, "exec"), g)

    # ---- what it wrote
    values = [p[:-1] for p in mined]
    index_of = {tuple(p): j for j, p in enumerate(values)}
    seqs = g["seq_list_ori"]
    row_of_seq = {id(s): i for i, s in enumerate(seqs)}
    pairs = g["data_generation_pair"]
    assert torch.load(os.path.join(root, "seq-pat-pair.pth")) == pairs
    pair_i = np.array([row_of_seq[id(s)] for s, _ in pairs], np.int32)
    pair_j = np.array([index_of[tuple(p)] for _, p in pairs], np.int32)
    assert all(list(seqs[i]) == list(s) for i, (s, _) in zip(pair_i, pairs))
    ref_rows = torch.load(os.path.join(root, "patterns.pth"))
    n_pat_rows = len(ref_rows) - len(train)
    assert ref_rows[n_pat_rows:] == train

    # ---- the complete match relation with the reference's own is_sublist
    is_sublist = g["is_sublist"]
    mi, mj = [], []
    for i, s in enumerate(seqs):
        for j, p in enumerate(values):
            if is_sublist(p, s):
                mi.append(i)
                mj.append(j)
    n_match = np.bincount(np.array(mi), minlength=len(seqs))
    ok, got = fixture_conditions(n_match, [len(s) for s in seqs])
    print(got, f"{len(mi)} matching pairs, the reference drew {len(pairs)}")
    assert ok, got
    per_row = collections.defaultdict(list)
    for i, j in zip(pair_i.tolist(), pair_j.tolist()):
        per_row[i].append(j)
    match_set = set(zip(mi, mj))
    for i in range(len(seqs)):                                # the reference's own draw: min(10, m) distinct matching patterns per row
        assert len(per_row[i]) == len(set(per_row[i])) == min(10, n_match[i]) and all((i, j) in match_set for j in per_row[i])

    lens = np.array([len(p) for p in values], np.int64)
    out = dict(
        train_user=np.array([r[0] for r in train], np.int32), train_items=np.array([r[1] for r in train], np.int32),
        train_targets=np.array([r[2] for r in train], np.int32), train_seqlen=np.array([r[3] for r in train], np.int32),
        pat_ids=np.array([v for p in values for v in p], np.int32), pat_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
        pat_freq=np.array([p[-1] for p in mined], np.int32),
        match_i=np.array(mi, np.int32), match_j=np.array(mj, np.int32), pair_i=pair_i, pair_j=pair_j,
        ref_pat_user=np.array([r[0] for r in ref_rows[:n_pat_rows]], np.int32),
        ref_pat_items=np.array([r[1] for r in ref_rows[:n_pat_rows]], np.int32),
        ref_pat_targets=np.array([r[2] for r in ref_rows[:n_pat_rows]], np.int32),
        ref_pat_seqlen=np.array([r[3] for r in ref_rows[:n_pat_rows]], np.int32),
        ref_pat_label=np.array([r[4] for r in ref_rows[:n_pat_rows]], np.uint8),
        ref_pat_domain=np.array([r[5] for r in ref_rows[:n_pat_rows]], np.uint8),
        n_real=np.int32(N_REAL), random_seed=np.int32(a.seed))
    np.savez_compressed(a.out, **out)
    size = os.path.getsize(a.out)
    print(a.out, size, "bytes")
    assert size < (1 << 20)


if __name__ == "__main__":
    main()
