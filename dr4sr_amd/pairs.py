"""The regenerator's pre-training data — stage 1 of DR4SR (the reference's 1.Build_pretraining_dataset.py) without the Python loop.

The reference mines patterns with seq2pat, writes `patterns.pth` (the deduplicated patterns as training rows + the original rows) and
then, for every training sequence, shuffles the whole pattern list and walks it with a pure-Python subsequence test until ten
patterns matched (`seq-pat-pair.pth`, what 2.Pretrain_regenerator.py trains on).  Here the sequences x patterns tests run in one
kernel (csrc/pairs.hip through dr4sr_pairs_match), and the random choice is a counter-based key per (sequence, pattern):

    n_match, chosen = match_and_choose(sequences_of(train_rows), pattern_values(mined), seed=0)
    build_pretraining_dataset("dataset/amazon-toys/toy/", patterns=mined)        # writes patterns.pth and seq-pat-pair.pth
    python -m dr4sr_amd.pairs --root_path dataset/amazon-toys/toy/ --patterns_file mined.pth

chosen[i] holds the min(10, m_i) patterns of sequence i's m_i matching ones with the smallest (key, j), ascending, -1 padded;
key(i, j) = word x of Philox4x32-10 with counter (i, j, 0x50414952, 0) and key (seed low, seed high) — a uniformly random subset in
uniformly random order, as "shuffle, take the first ten hits" draws, but a pure function of (seed, i, j).  The reference draws from
Python's unseeded `random`, so its file is not reproducible bit for bit by anything; the match relation is reproduced exactly.

backend="hip" is the kernel; backend="numpy" restates it on the host with integer numpy (same subsequence rule, same signatures, same
Philox keys), so both return identical arrays and the module works without a GPU.  Nothing switches backends on its own.
Mining: pass what `Seq2Pat.get_patterns` returned, let the CLI import seq2pat (`sequential.seq2pat`, the default), or mine with this
project's own miner (dr4sr_amd/mine.py: `miner="hip"` / `"numpy"`, `--miner hip|numpy`), which needs no seq2pat.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

N_CHOSEN = 10                  # 1.Build_pretraining_dataset.py:88
L_MAX = 64                     # longest sequence the kernel holds (toys rows have at most 51 ids)
MAX_SEQ_LEN = 50               # 1.Build_pretraining_dataset.py:17
KEY_SITE = 0x50414952          # third counter word of the Philox call ("PAIR")
_M32 = np.uint64(0xFFFFFFFF)
_BLOCK = 64                    # sequences per numpy block


def sequences_of(train_rows):
    """1.Build_pretraining_dataset.py:34: history up to seqlen plus the last target, per train.pth row"""
    return [list(r[1][:r[3]]) + [r[2][r[3] - 1]] for r in train_rows]


def pattern_values(mined):
    """1.Build_pretraining_dataset.py:28: what Seq2Pat.get_patterns returned, without each pattern's trailing frequency"""
    return [list(p[:-1]) for p in mined]


def pattern_rows(patterns, max_seq_len: int = MAX_SEQ_LEN):
    """1.Build_pretraining_dataset.py:37-65: pattern id lists -> the deduplicated, padded training rows of patterns.pth, in the
    reference's order (the same tuples inserted into a set in the same order iterate in the same order)"""
    def truncate_or_pad(seq):
        return seq[-max_seq_len:] if len(seq) > max_seq_len else seq + [0] * (max_seq_len - len(seq))

    train_set = set()
    for pattern in patterns:
        seq = [int(v) for v in pattern]
        train_set.add(tuple(truncate_or_pad(seq[:-1]) + truncate_or_pad(seq[1:])))
    rows = []
    for t in list(train_set):
        item_seq, target_seq = t[:max_seq_len], t[max_seq_len:]
        seq_len = sum(a != 0 for a in item_seq)
        rows.append([0, item_seq, target_seq, seq_len, [1] * seq_len + [0] * (max_seq_len - seq_len), [0] * max_seq_len])
    return rows


# ---------------------------------------------------------------------------------------------------- packing
def pack_sequences(seqs):
    """-> ids int32 [S, Lmax] (0 padded), lengths int32 [S]"""
    lens = np.fromiter((len(s) for s in seqs), dtype=np.int32, count=len(seqs))
    Lmax = int(lens.max()) if len(seqs) else 1
    if Lmax > L_MAX:
        raise ValueError(f"a sequence of {Lmax} ids: at most {L_MAX} are supported (the reference's rows have at most {MAX_SEQ_LEN + 1})")
    Lmax = max(Lmax, 1)
    ids = np.zeros((len(seqs), Lmax), dtype=np.int32)
    for i, s in enumerate(seqs):
        ids[i, :lens[i]] = s
    return ids, lens


def pack_patterns(patterns):
    """-> ids int32 [n_ids], offsets int64 [P + 1]; an empty pattern is refused (seq2pat never emits one)"""
    lens = np.fromiter((len(p) for p in patterns), dtype=np.int64, count=len(patterns))
    if len(patterns) and int(lens.min()) < 1:
        raise ValueError(f"pattern {int(np.argmin(lens))} is empty")
    off = np.zeros(len(patterns) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    ids = np.fromiter((v for p in patterns for v in p), dtype=np.int32, count=int(off[-1]))
    return ids, off


# ---------------------------------------------------------------------------------------------------- numpy restatement
def philox_keys(seed: int, i, j):
    """word x of philox4x32_10(counter (i, j, KEY_SITE, 0), key (seed low, seed high)) for uint32 arrays i, j (csrc/common.h)"""
    c0 = np.asarray(i, dtype=np.uint64) & _M32
    c1 = np.asarray(j, dtype=np.uint64) & _M32
    c2 = np.full_like(c0, KEY_SITE)
    c3 = np.zeros_like(c0)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0


def _sig_bits(ids):
    """the 128-bit signature's bit of each id, as (word 0 mask, word 1 mask) uint64"""
    bit = (ids.astype(np.uint32) * np.uint32(0x9E3779B1)) >> np.uint32(25)
    m = np.uint64(1) << (bit & np.uint32(63)).astype(np.uint64)
    hi = bit >= 64
    return np.where(hi, np.uint64(0), m), np.where(hi, m, np.uint64(0))


def _match_block(a, b, seq_ids, seq_len, pat2d, plen, ps0, ps1):
    """matching (i, j) of sequences a..b-1 against every pattern: signature reject, then the greedy left-most scan, vectorised"""
    sl = seq_len[a:b]
    valid = np.arange(seq_ids.shape[1])[None, :] < sl[:, None]
    m0, m1 = _sig_bits(seq_ids[a:b])
    ss0 = np.bitwise_or.reduce(np.where(valid, m0, np.uint64(0)), axis=1)
    ss1 = np.bitwise_or.reduce(np.where(valid, m1, np.uint64(0)), axis=1)
    cand = ((ps0[None, :] & ~ss0[:, None]) | (ps1[None, :] & ~ss1[:, None])) == 0
    cand &= plen[None, :] <= sl[:, None]
    ii, jj = np.nonzero(cand)
    if ii.size == 0:
        return ii.astype(np.int64), jj.astype(np.int64)
    k = np.zeros(ii.size, dtype=np.int64)
    pl, rows, last = plen[jj], seq_ids[a:b], pat2d.shape[1] - 1
    sli = sl[ii]
    for t in range(int(sl.max())):
        want = pat2d[jj, np.minimum(k, last)]
        k += (rows[ii, t] == want) & (k < pl) & (t < sli)
    hit = k >= pl
    return ii[hit].astype(np.int64) + a, jj[hit].astype(np.int64)


def _match_numpy(seq_ids, seq_len, pat_ids, pat_off, threads):
    P = len(pat_off) - 1
    plen = np.diff(pat_off)
    width = int(min(max(int(plen.max()), 1), L_MAX))
    pat2d = np.zeros((P, width), dtype=np.int32)
    cols = np.arange(len(pat_ids), dtype=np.int64) - np.repeat(pat_off[:-1], plen)
    keep = cols < width                                     # ids past 64 of an over-long pattern: it matches no sequence anyway
    pat2d[np.repeat(np.arange(P), plen)[keep], cols[keep]] = pat_ids[keep]
    m0, m1 = _sig_bits(pat_ids)
    ps0, ps1 = np.bitwise_or.reduceat(m0, pat_off[:-1]), np.bitwise_or.reduceat(m1, pat_off[:-1])
    blocks = [(a, min(a + _BLOCK, len(seq_len))) for a in range(0, len(seq_len), _BLOCK)]
    run = lambda ab: _match_block(ab[0], ab[1], seq_ids, seq_len, pat2d, plen, ps0, ps1)
    if threads > 1 and len(blocks) > 1:
        with ThreadPoolExecutor(threads) as ex:
            parts = list(ex.map(run, blocks))
    else:
        parts = [run(ab) for ab in blocks]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def matches_numpy(seqs, patterns, threads: int | None = None):
    """the complete match relation as sorted (i, j) int64 arrays — the host restatement of is_sublist over all pairs"""
    seq_ids, seq_len = pack_sequences(seqs)
    pat_ids, pat_off = pack_patterns(patterns)
    if len(seqs) == 0 or len(patterns) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return _match_numpy(seq_ids, seq_len, pat_ids, pat_off, _threads(threads))


def _threads(threads):
    return max(1, min(16, os.cpu_count() or 1)) if threads is None else max(1, int(threads))


def _choose_numpy(S, mi, mj, seed, seq_index0, pat_index0):
    n_match = np.bincount(mi, minlength=S).astype(np.int32)
    chosen = np.full((S, N_CHOSEN), -1, dtype=np.int32)
    if mi.size:
        gj = (mj + pat_index0).astype(np.uint64)
        word = (philox_keys(seed, mi + seq_index0, gj) << np.uint64(32)) | gj
        order = np.lexsort((word, mi))
        si = mi[order]
        start = np.concatenate([[0], np.cumsum(n_match)[:-1]])
        rank = np.arange(si.size) - start[si]
        top = rank < N_CHOSEN
        chosen[si[top], rank[top]] = gj[order][top].astype(np.int32)
    return n_match, chosen


# ---------------------------------------------------------------------------------------------------- HIP
def _match_hip(seq_ids, seq_len, pat_ids, pat_off, seed, seq_index0, pat_index0, n_chunks, device):
    import torch
    from . import _lib
    lib = _lib.load()
    dev = torch.device(device)
    S, Lmax = seq_ids.shape
    P = len(pat_off) - 1
    with torch.cuda.device(dev):
        d_seq, d_len = torch.from_numpy(seq_ids).to(dev), torch.from_numpy(seq_len).to(dev)
        d_ids = torch.from_numpy(pat_ids if pat_ids.size else np.zeros(1, np.int32)).to(dev)
        d_off = torch.from_numpy(pat_off).to(dev)
        nb = lib.dr4sr_pairs_workspace_bytes(S, P, n_chunks)
        if nb < 0:
            _lib.check(int(nb), "dr4sr_pairs_workspace_bytes")
        ws = torch.empty(int(nb), dtype=torch.uint8, device=dev)
        n_match = torch.empty(max(S, 1), dtype=torch.int32, device=dev)
        chosen = torch.empty(max(S, 1), N_CHOSEN, dtype=torch.int32, device=dev)
        _lib.check(lib.dr4sr_pairs_match(_lib.ptr(d_seq), _lib.ptr(d_len), S, Lmax, _lib.ptr(d_ids), _lib.ptr(d_off), P, int(pat_ids.size),
                                         C.c_uint64(seed), seq_index0, pat_index0, n_chunks, C.c_void_p(ws.data_ptr()), int(nb),
                                         _lib.ptr(n_match), _lib.ptr(chosen), _lib.cur_stream()), "dr4sr_pairs_match")
        return n_match[:S].cpu().numpy(), chosen[:S].cpu().numpy()


# ---------------------------------------------------------------------------------------------------- public
def match_and_choose(seqs, patterns, seed: int = 0, backend: str = "hip", *, seq_index0: int = 0, pat_index0: int = 0,
                     n_chunks: int = 0, seq_chunk: int | None = None, device="cuda", threads: int | None = None):
    """(n_match int32 [S], chosen int32 [S, 10]) as numpy arrays: per sequence the number of patterns that are subsequences of it, and
    the min(10, m) of them with the smallest (key, j) in ascending order, -1 padded (values are pat_index0 + position in `patterns`).

    seqs: lists of ids (at most 64 each); patterns: non-empty lists of ids.  seq_index0 / pat_index0: the index in the whole file /
    list of the first sequence / pattern given, when a caller splits either; n_chunks (hip): workgroups per sequence tile that share
    the pattern list (0: chosen from the sizes); seq_chunk: sequences per call (None: all at once).  None of them changes the result."""
    if backend not in ("hip", "numpy"):
        raise ValueError(f"backend must be 'hip' or 'numpy', not {backend!r}")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    seq_ids, seq_len = pack_sequences(seqs)
    pat_ids, pat_off = pack_patterns(patterns)
    S = len(seqs)
    step = S if not seq_chunk else int(seq_chunk)
    outs = []
    for a in range(0, S, max(step, 1)):
        b = min(S, a + step)
        if backend == "hip":
            outs.append(_match_hip(np.ascontiguousarray(seq_ids[a:b]), np.ascontiguousarray(seq_len[a:b]), pat_ids, pat_off, seed,
                                   seq_index0 + a, pat_index0, int(n_chunks), device))
        else:
            if len(patterns):
                mi, mj = _match_numpy(seq_ids[a:b], seq_len[a:b], pat_ids, pat_off, _threads(threads))
            else:
                mi = mj = np.zeros(0, np.int64)
            outs.append(_choose_numpy(b - a, mi, mj, seed, seq_index0 + a, pat_index0))
    if not outs:
        return np.zeros(0, np.int32), np.full((0, N_CHOSEN), -1, np.int32)
    return np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs])


def pair_list(seqs, patterns, chosen):
    """1.Build_pretraining_dataset.py:79-89: the [sequence, pattern] pairs of seq-pat-pair.pth, sequences in file order"""
    out = []
    for seq, row in zip(seqs, chosen.tolist()):
        for j in row:
            if j < 0:
                break
            out.append([seq, patterns[j]])
    return out


def mine_patterns(root_path: str, alpha: int = 5, beta: int = 2, n_jobs: int = 2):
    """1.Build_pretraining_dataset.py:20-27: seq2pat over seq2pat_data.pth.  Needs the `sequential` package (not part of this project)"""
    import torch
    from sequential.seq2pat import Seq2Pat
    data = torch.load(os.path.join(root_path, "seq2pat_data.pth"))
    return Seq2Pat(sequences=data, n_jobs=n_jobs, max_span=alpha).get_patterns(min_frequency=beta)


MINERS = ("seq2pat", "hip", "numpy")


def _mine(root_path, alpha, beta, n_jobs, miner, device):
    """seq2pat_data.pth under root_path -> the mined list: with seq2pat itself (the default), or with this project's miner
    (dr4sr_amd/mine.py, its HIP or its numpy backend), which never imports `sequential`"""
    miner = "seq2pat" if miner is None else miner
    if miner not in MINERS:
        raise ValueError(f"miner must be one of {MINERS}, not {miner!r}")
    if miner == "seq2pat":
        return mine_patterns(root_path, alpha, beta, n_jobs)
    from .mine import mine_file
    return mine_file(root_path, alpha, beta, miner, device)


def build_pretraining_dataset(root_path: str, patterns=None, alpha: int = 5, beta: int = 2, n_jobs: int = 2, seed: int = 0,
                              backend: str = "hip", device="cuda", miner: str | None = None):
    """1.Build_pretraining_dataset.py's __main__: reads train.pth under root_path, writes patterns.pth (pattern rows + training rows)
    and seq-pat-pair.pth next to it; returns both paths.  `patterns`: what Seq2Pat.get_patterns returned (each pattern's ids followed
    by its frequency); None mines them from seq2pat_data.pth (alpha = max_span, beta = min_frequency) with `miner`: None / "seq2pat" as
    the reference does, "hip" / "numpy" with dr4sr_amd.mine."""
    import torch
    if patterns is None:
        patterns = _mine(root_path, alpha, beta, n_jobs, miner, device)
    values = [[int(v) for v in p] for p in pattern_values(patterns)]
    train = torch.load(os.path.join(root_path, "train.pth"))
    pat_path = os.path.join(root_path, "patterns.pth")
    torch.save(pattern_rows(values) + train, pat_path)
    seqs = sequences_of(train)
    _, chosen = match_and_choose(seqs, values, seed, backend, device=device)
    pair_path = os.path.join(root_path, "seq-pat-pair.pth")
    torch.save(pair_list(seqs, values, chosen), pair_path)
    return pat_path, pair_path


def main(argv=None):
    ap = argparse.ArgumentParser(description="DR4SR stage 1: patterns.pth and seq-pat-pair.pth for the regenerator's pre-training")
    ap.add_argument("--root_path", type=str, default="./dataset/amazon-toys/toy/", help="The path to the training dataset.")
    ap.add_argument("--alpha", type=int, default=5, help="The sliding window size for pre-training dataset construction.")
    ap.add_argument("--beta", type=int, default=2, help="The threshold for pre-training dataset construction.")
    ap.add_argument("--n_jobs", type=int, default=2, help="The job number for Seq2Pat pattern mining.")
    ap.add_argument("--patterns_file", type=str, default=None,
                    help="torch.save of what Seq2Pat.get_patterns returned, mined wherever seq2pat is installed (skips mining here)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the random choice of ten patterns per sequence")
    ap.add_argument("--backend", type=str, default="hip", choices=("hip", "numpy"))
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--miner", type=str, default="seq2pat", choices=MINERS,
                    help="who mines seq2pat_data.pth without --patterns_file: seq2pat (the `sequential` package), or dr4sr_amd.mine on the "
                         "GPU (hip) or the host (numpy)")
    a = ap.parse_args(argv)
    import torch
    device = "cpu"
    if "hip" in (a.backend, a.miner if a.patterns_file is None else None):
        torch.cuda.set_device(a.gpu)
        device = torch.device("cuda", a.gpu)
    if a.patterns_file is not None:
        patterns = torch.load(a.patterns_file)
    else:
        try:
            patterns = _mine(a.root_path, a.alpha, a.beta, a.n_jobs, a.miner, device)
        except ImportError as e:
            if a.miner != "seq2pat":
                raise
            sys.exit(f"dr4sr_amd.pairs: cannot import sequential.seq2pat ({e}); mine the patterns where seq2pat is installed, "
                     f"torch.save what Seq2Pat.get_patterns returned, and pass it with --patterns_file (or mine here with --miner hip)")
    for path in build_pretraining_dataset(a.root_path, patterns, a.alpha, a.beta, a.n_jobs, a.seed, a.backend, device):
        print(path)


if __name__ == "__main__":
    main()
