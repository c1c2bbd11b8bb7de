"""Pattern mining for the regenerator — the first step of DR4SR stage 1 (the reference's 1.Build_pretraining_dataset.py:24-27,
`Seq2Pat(sequences, max_span=alpha).get_patterns(min_frequency=beta)`) without the third-party `sequential` package.

    mined = mine_patterns(sequences, alpha=5, beta=2)                   # [[id_0, ..., id_{k-1}, frequency], ...] of Python ints
    python -m dr4sr_amd.mine --root_path dataset/amazon-toys/toy/ --out mined.pth     # a file `dr4sr_amd.pairs --patterns_file` accepts

The rule (tests/_mine_ref.py states it by brute force): a pattern is a tuple of k ids, 2 <= k <= alpha; it occurs in a
sequence if its ids stand at increasing positions whose first and last are at most reach(alpha) = alpha - 1 apart (all items inside a
window of alpha consecutive positions); its frequency is the number of sequences with at least one occurrence; the result is every
pattern with frequency >= beta, frequency descending, then id tuple ascending (a prefix of another tuple first).  The rule is what
seq2pat 1.4.0 DOCUMENTS for its built-in index-span constraint (span <= max_span - 1); seq2pat is installed nowhere this project builds
or runs, so "equals seq2pat" rests on that documentation and not on a run.  seq2pat leaves the order of equal frequencies unspecified;
here it is fixed, because pairs.pattern_rows and the Philox keys of pairs.match_and_choose depend on the patterns' order.

backend="hip" is csrc/mine.hip through dr4sr_mine_patterns (one thread per candidate, an open-addressing table of owner words and integer
counts); backend="numpy" restates the rule with integer numpy (candidate matrix, one row per (sequence, tuple), then per tuple), in
chunks of sequences, and works without a GPU.  Both return the identical list.  Nothing switches backends on its own.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os

import numpy as np

ALPHA_MIN, ALPHA_MAX = 2, 10
MAX_SEQ_LEN = 4096             # the earlier-start test of the kernel reads a candidate's whole sequence prefix: quadratic per sequence
ID_MAX = 2 ** 31 - 1
_CHUNK_CANDIDATES = 1 << 21    # numpy backend: (position, mask) pairs per block of sequences
_MERGE_ROWS = 1 << 23          # numpy backend: pending (tuple, count) rows before they are merged
_FIRST_CAP = 1 << 20           # hip backend: output rows of the first call (a larger result takes a second call sized by n_out)


def reach(alpha: int) -> int:
    """THE span rule of the numpy backend and of every size computed here: the last item of an occurrence lies at most this many
    positions after its first.  If a run of the real seq2pat ever shows the bound to be off by one, this line changes and nothing else
    (csrc/mine.hip mine_reach is the same place of the HIP backend)."""
    return alpha - 1


# ---------------------------------------------------------------------------------------------------- checks and packing
def _check_args(alpha, beta, backend):
    if backend not in ("hip", "numpy"):
        raise ValueError(f"backend must be 'hip' or 'numpy', not {backend!r}")
    if int(alpha) != alpha or not ALPHA_MIN <= alpha <= ALPHA_MAX:
        raise ValueError(f"alpha must be an integer in {ALPHA_MIN}..{ALPHA_MAX}, not {alpha!r}")
    if int(beta) != beta or beta < 1:
        raise ValueError(f"beta must be an integer >= 1, not {beta!r} (a fractional min_frequency is not supported)")


def pack(sequences):
    """-> ids int32 [n_ids], offsets int64 [S + 1]; refuses ids outside 1..2^31-1 and sequences of more than 4 096 ids"""
    lens = np.fromiter((len(s) for s in sequences), dtype=np.int64, count=len(sequences))
    if len(sequences) and int(lens.max()) > MAX_SEQ_LEN:
        raise ValueError(f"sequence {int(np.argmax(lens))} has {int(lens.max())} ids: at most {MAX_SEQ_LEN} are supported")
    off = np.zeros(len(sequences) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    ids = np.fromiter((int(v) for s in sequences for v in s), dtype=np.int64, count=int(off[-1]))
    if ids.size and (int(ids.min()) < 1 or int(ids.max()) > ID_MAX):
        bad = int(ids[(ids < 1) | (ids > ID_MAX)][0])
        raise ValueError(f"item id {bad}: ids must lie in 1..{ID_MAX}")
    return ids.astype(np.int32), off


def candidate_count(off, alpha: int) -> int:
    """the exact number of candidates: (position, non-empty offset set) pairs whose highest offset lies inside the position's sequence"""
    lens = np.diff(off)
    r = reach(alpha)
    total = 0
    for h in range(1, r + 1):                                  # offset sets whose highest offset is h: 2^(h-1), at len - h positions
        total += int(np.maximum(lens - h, 0).sum()) << (h - 1)
    return total


def canonical(ids2d, freq):
    """rows of zero padded ids + frequencies -> the result list: frequency descending, then ids ascending (padding 0 sorts a prefix first)"""
    ids2d, freq = np.asarray(ids2d, dtype=np.int64), np.asarray(freq, dtype=np.int64)
    if ids2d.shape[0] == 0:
        return []
    order = np.lexsort(tuple(ids2d[:, c] for c in range(ids2d.shape[1] - 1, -1, -1)) + (-freq,))
    rows, k, f = ids2d[order].tolist(), (ids2d[order] != 0).sum(axis=1).tolist(), freq[order].tolist()
    return [row[:n] + [c] for row, n, c in zip(rows, k, f)]


# ---------------------------------------------------------------------------------------------------- numpy restatement
def _groups(keys):
    """rows sorted by the key columns (first key most significant) -> (order, starts of the runs of equal rows in that order)"""
    order = np.lexsort(tuple(reversed(keys)))
    new = np.zeros(order.size, dtype=bool)
    new[:1] = True
    for k in keys:
        s = k[order]
        new[1:] |= s[1:] != s[:-1]
    return order, np.nonzero(new)[0]


def _merge(parts):
    """[(words [n, W], count [n])] -> one (words, count) with every distinct row once and its counts summed"""
    words, count = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    if words.shape[0] == 0:
        return words, count
    order, starts = _groups([words[:, w] for w in range(words.shape[1])])
    return words[order[starts]], np.add.reduceat(count[order], starts)


def _mine_numpy(ids, off, alpha, beta):
    r = reach(alpha)
    n_mask = (1 << r) - 1
    uniq, rank = np.unique(ids, return_inverse=True)           # dense ranks 1..V keep the ids' order and pack into few 64-bit words
    rank = rank.astype(np.int64) + 1
    bits = max(1, int(uniq.size).bit_length())
    per_word = 63 // bits
    n_words = -(-(r + 1) // per_word)
    masks = np.arange(1, n_mask + 1, dtype=np.int64)
    top = np.array([int(m).bit_length() for m in masks], dtype=np.int64)          # highest offset of each mask
    cols = np.full((n_mask, r + 1), -1, dtype=np.int64)        # cols[m, c]: the offset of the mask's c-th item, -1 past its last
    cols[:, 0] = 0
    for a, m in enumerate(masks.tolist()):
        offs = [j + 1 for j in range(r) if (m >> j) & 1]
        cols[a, 1:1 + len(offs)] = offs
    lens = np.diff(off)
    S = len(lens)
    parts, pending = [], 0
    a = 0
    while a < S:
        b = a + 1
        while b < S and (off[b + 1] - off[a]) * n_mask <= _CHUNK_CANDIDATES:
            b += 1
        g0, g1 = int(off[a]), int(off[b])
        seq = np.repeat(np.arange(a, b, dtype=np.int64), lens[a:b])
        room = off[seq + 1] - 1 - np.arange(g0, g1, dtype=np.int64)               # positions after each one inside its sequence
        gi, mi = np.nonzero(top[None, :] <= room[:, None])
        a = b
        if gi.size == 0:
            continue
        c = cols[mi]
        vals = np.where(c >= 0, rank[g0 + gi[:, None] + np.maximum(c, 0)], 0)
        words = np.zeros((gi.size, n_words), dtype=np.int64)
        for col in range(r + 1):
            w, slot = divmod(col, per_word)
            words[:, w] |= vals[:, col] << (bits * (per_word - 1 - slot))
        keys = [words[:, w] for w in range(n_words)]
        order, starts = _groups([seq[gi]] + keys)              # one row per (sequence, tuple)
        once = words[order[starts]]
        order, starts = _groups([once[:, w] for w in range(n_words)])             # ... then per tuple: sequences of this block holding it
        parts.append((once[order[starts]], np.diff(np.append(starts, order.size))))
        pending += starts.size
        if pending > _MERGE_ROWS:
            parts = [_merge(parts)]
            pending = parts[0][1].size
    if not parts:
        return []
    words, count = _merge(parts)
    keep = count >= beta
    words, count = words[keep], count[keep]
    ids2d = np.zeros((words.shape[0], r + 1), dtype=np.int64)
    lookup = np.concatenate([[0], uniq.astype(np.int64)])
    for col in range(r + 1):
        w, slot = divmod(col, per_word)
        ids2d[:, col] = lookup[(words[:, w] >> (bits * (per_word - 1 - slot))) & ((1 << bits) - 1)]
    return canonical(ids2d, count)


# ---------------------------------------------------------------------------------------------------- HIP
def table_slots_for(n_candidates: int) -> int:
    """the default table: the first power of two at or above twice the exact candidate count (at least 256) — every distinct tuple is
    some candidate's, so this table cannot fill up, and it is at most half full"""
    slots = 256
    while slots < 2 * n_candidates:
        slots <<= 1
    return slots


def mine_hip_raw(ids, off, alpha, beta, table_slots=0, cap=None, device="cuda"):
    """one or two dr4sr_mine_patterns calls -> (ids2d int32 [n, alpha], freq int32 [n], stats): the patterns in the device's order.
    stats: table_slots, distinct tuples, load factor and mean probe length of the finished table, calls made"""
    import torch
    from . import _lib
    lib = _lib.load()
    dev = torch.device(device)
    n_ids, n_seq = int(ids.size), len(off) - 1
    slots = int(table_slots) if table_slots else table_slots_for(candidate_count(off, alpha))
    cap = int(cap) if cap is not None else max(1, min(_FIRST_CAP, slots))
    with torch.cuda.device(dev):
        nb = int(lib.dr4sr_mine_workspace_bytes(n_ids, n_seq, alpha, slots))
        if nb < 0:
            _lib.check(nb, "dr4sr_mine_workspace_bytes")
        d_ids = torch.from_numpy(ids if n_ids else np.zeros(1, np.int32)).to(dev)
        d_off = torch.from_numpy(off).to(dev)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        n_out = torch.empty(1, dtype=torch.int32, device=dev)
        status = torch.empty(4, dtype=torch.int64, device=dev)
        calls = 0
        while True:
            out_ids = torch.empty(cap, alpha, dtype=torch.int32, device=dev)
            out_freq = torch.empty(cap, dtype=torch.int32, device=dev)
            _lib.check(lib.dr4sr_mine_patterns(_lib.ptr(d_ids), _lib.ptr(d_off), n_ids, n_seq, alpha, beta, slots, C.c_void_p(ws.data_ptr()),
                                               nb, _lib.ptr(out_ids), _lib.ptr(out_freq), cap, _lib.ptr(n_out), _lib.ptr(status),
                                               _lib.cur_stream()), "dr4sr_mine_patterns")
            calls += 1
            st = status.tolist()
            if st[0]:
                raise _lib.Dr4srError(f"dr4sr_mine_patterns: the table of {slots} slots filled up (table_slots is smaller than the number "
                                      f"of distinct tuples); pass table_slots=0 for a table sized from the candidate count")
            n = int(n_out)
            if n <= cap:
                break
            cap = n                                            # the counter holds the whole result's size: one more call, sized by it
        stats = {"table_slots": slots, "distinct_tuples": st[1], "load_factor": st[1] / slots,
                 "mean_probe_length": 1.0 + st[2] / max(st[1], 1), "calls": calls}
        return out_ids[:n].cpu().numpy(), out_freq[:n].cpu().numpy(), stats


# ---------------------------------------------------------------------------------------------------- public
def mine_patterns(sequences, alpha: int = 5, beta: int = 2, backend: str = "hip", device="cuda", table_slots: int = 0):
    """what `Seq2Pat(sequences, max_span=alpha).get_patterns(min_frequency=beta)` is documented to return, in a fixed order: a list of
    [id_0, ..., id_{k-1}, frequency] (Python ints), 2 <= k <= alpha, frequency descending, then ids ascending.

    sequences: lists of ids in 1..2^31-1, of any length up to 4 096 (0 and 1 included).  alpha in 2..10, beta >= 1.  table_slots (hip):
    slots of the kernel's table, a power of two; 0 sizes it from the exact candidate count so that it cannot fill up.  A table that is
    too small raises Dr4srError; no table size changes the result."""
    _check_args(alpha, beta, backend)
    alpha, beta = int(alpha), int(beta)
    ids, off = pack(sequences)
    if backend == "numpy":
        return _mine_numpy(ids, off, alpha, beta)
    ids2d, freq, _ = mine_hip_raw(ids, off, alpha, beta, table_slots, device=device)
    return canonical(ids2d, freq)


def mine_file(root_path: str, alpha: int = 5, beta: int = 2, backend: str = "hip", device="cuda"):
    """1.Build_pretraining_dataset.py:20-27 over seq2pat_data.pth under root_path, with this module's miner"""
    import torch
    data = torch.load(os.path.join(root_path, "seq2pat_data.pth"))
    return mine_patterns(data, alpha, beta, backend, device)


def main(argv=None):
    ap = argparse.ArgumentParser(description="DR4SR stage 1, mining: the patterns of seq2pat_data.pth, in Seq2Pat.get_patterns' format")
    ap.add_argument("--root_path", type=str, default="./dataset/amazon-toys/toy/", help="The path to the training dataset.")
    ap.add_argument("--alpha", type=int, default=5, help="The sliding window size for pre-training dataset construction.")
    ap.add_argument("--beta", type=int, default=2, help="The threshold for pre-training dataset construction.")
    ap.add_argument("--backend", type=str, default="hip", choices=("hip", "numpy"))
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--out", type=str, default=None, help="where to torch.save the list (default: mined.pth under --root_path)")
    a = ap.parse_args(argv)
    import torch
    device = "cpu"
    if a.backend == "hip":
        torch.cuda.set_device(a.gpu)
        device = torch.device("cuda", a.gpu)
    mined = mine_file(a.root_path, a.alpha, a.beta, a.backend, device)
    out = a.out or os.path.join(a.root_path, "mined.pth")
    torch.save(mined, out)
    print(out)


if __name__ == "__main__":
    main()
