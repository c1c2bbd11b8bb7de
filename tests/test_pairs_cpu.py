"""The regenerator's pre-training pairs (dr4sr_amd.pairs, DR4SR stage 1) without a GPU: the numpy restatement against the match relation
the reference's own is_sublist gave (tests/golden/pairs_toys.npz, tools/make_pairs_golden.py), the invariants and the law of the
selection, the patterns.pth / seq-pat-pair.pth writers, the CLI, and the C ABI's host-side checks."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "pairs_toys.npz")
L = 50


def load_fixture():
    """(z, train rows in the train.pth format, sequences, pattern id lists, what get_patterns returned)"""
    from dr4sr_amd.pairs import sequences_of
    z = np.load(GOLD)
    train = []
    for u, it, tg, sl in zip(z["train_user"].tolist(), z["train_items"].tolist(), z["train_targets"].tolist(), z["train_seqlen"].tolist()):
        train.append([u, it, tg, sl, [1] * sl + [0] * (L - sl), [0] * L])
    ids, off = z["pat_ids"].tolist(), z["pat_off"].tolist()
    values = [ids[a:b] for a, b in zip(off[:-1], off[1:])]
    mined = [v + [f] for v, f in zip(values, z["pat_freq"].tolist())]
    return z, train, sequences_of(train), values, mined


def golden_matches(z, n_seq):
    per = [set() for _ in range(n_seq)]
    for i, j in zip(z["match_i"].tolist(), z["match_j"].tolist()):
        per[i].add(j)
    return per


def check_selection(chosen, per_row):
    """the invariants of a draw, per row: min(10, m) entries, all distinct, all matching, -1 padding after"""
    for i, (row, m) in enumerate(zip(np.asarray(chosen).tolist(), per_row)):
        k = min(10, len(m))
        assert all(j >= 0 for j in row[:k]) and all(j == -1 for j in row[k:]), (i, row, len(m))
        assert len(set(row[:k])) == k and set(row[:k]) <= m, (i, row)


def sublist(p, s):
    """plain restatement of the subsequence rule for the tests' own small cases"""
    it = iter(s)
    return all(any(x == y for y in it) for x in p)


def test_fixture_covers_what_it_must():
    z, train, seqs, values, mined = load_fixture()
    per = golden_matches(z, len(seqs))
    m = np.array([len(s) for s in per])
    lens = np.array([len(s) for s in seqs])
    assert (m == 0).sum() >= 50 and ((m >= 1) & (m <= 9)).sum() >= 100 and (m == 10).sum() >= 1 and (m > 10).sum() >= 50
    assert m.max() >= 500 and (lens == 51).sum() >= 20 and lens.max() == 51
    n_real = int(z["n_real"])
    assert n_real == 400 and sum(len(set(s)) < len(s) for s in seqs[n_real:]) >= 8
    assert not any(len(set(s)) < len(s) for s in seqs[:n_real])
    # repeated ids are respected: [1, 1] needs two 1s, [1, 2, 1] matches 1 2 1 and not 1 1 2
    idx = {tuple(v): j for j, v in enumerate(values)}
    row = {tuple(s): i for i, s in enumerate(seqs)}
    assert idx[(1, 1)] not in per[row[(1, 2)]] and idx[(1, 1)] in per[row[(1, 1)]]
    assert idx[(1, 2, 1)] in per[row[(1, 2, 1)]] and idx[(1, 2, 1)] not in per[row[(1, 1, 2)]]
    assert idx[(3,) * 51] in per[row[(3,) * 51]] and not any(idx[(3,) * 52] in p for p in per)


def test_match_relation_equals_the_reference():
    from dr4sr_amd.pairs import match_and_choose, matches_numpy
    z, train, seqs, values, mined = load_fixture()
    per = golden_matches(z, len(seqs))
    mi, mj = matches_numpy(seqs, values)
    got = [set() for _ in seqs]
    for i, j in zip(mi.tolist(), mj.tolist()):
        got[i].add(j)
    assert got == per
    n_match, chosen = match_and_choose(seqs, values, seed=5, backend="numpy")
    assert n_match.dtype == np.int32 and chosen.dtype == np.int32 and chosen.shape == (len(seqs), 10)
    assert n_match.tolist() == [len(s) for s in per]
    check_selection(chosen, per)
    # the reference's recorded draw passes the same function
    ref = np.full((len(seqs), 10), -1, np.int64)
    fill = [0] * len(seqs)
    for i, j in zip(z["pair_i"].tolist(), z["pair_j"].tolist()):
        ref[i, fill[i]] = j
        fill[i] += 1
    assert np.all(np.diff(z["pair_i"]) >= 0)                      # sequences in file order
    check_selection(ref, per)


def test_selection_is_ascending_in_key_then_index():
    from dr4sr_amd.pairs import match_and_choose, philox_keys
    z, train, seqs, values, mined = load_fixture()
    per = golden_matches(z, len(seqs))
    seed = (7 << 32) | 123                                        # both halves of the 64-bit seed are used
    n_match, chosen = match_and_choose(seqs, values, seed=seed, backend="numpy")
    for i in (int(np.argmax(n_match)), int(np.argmax(n_match == 10)), int(np.argmax((n_match > 0) & (n_match < 10)))):
        js = np.array(sorted(per[i]), np.uint64)
        word = (philox_keys(seed, np.full(js.size, i, np.uint64), js) << np.uint64(32)) | js
        want = js[np.argsort(word)][:10].astype(np.int64).tolist()
        assert chosen[i, :len(want)].tolist() == want, i
    assert not np.array_equal(match_and_choose(seqs, values, seed=123, backend="numpy")[1], chosen)
    # Philox4x32-10 known answer (Random123 kat_vectors): counter 0, key 0 -> first word 6627e8d5
    from dr4sr_amd import pairs as P
    site = P.KEY_SITE
    try:
        P.KEY_SITE = 0
        assert int(philox_keys(0, np.zeros(1, np.uint64), np.zeros(1, np.uint64))[0]) == 0x6627E8D5
    finally:
        P.KEY_SITE = site


def test_selection_law_on_a_row_with_40_matches():
    """inclusion of each of 40 matching patterns ~ Binomial(4000, 10/40), first slot ~ Binomial(4000, 1/40): every one of the 80
    statistics within 5 sigma (false-alarm probability below 1e-4 for a uniform choice; seeds fixed, so the test is deterministic)"""
    from dr4sr_amd.pairs import match_and_choose
    seq = list(range(100, 140))
    hit = [[100 + k] for k in range(40)]
    miss = [[200 + k, 100] for k in range(25)]
    patterns = []
    for k in range(40):                                            # matching and non-matching patterns interleaved
        patterns.append(hit[k])
        if k < 25:
            patterns.append(miss[k])
    hit_idx = [j for j, p in enumerate(patterns) if sublist(p, seq)]
    assert len(hit_idx) == 40
    n_seed = 4000
    incl = np.zeros(len(patterns), np.int64)
    first = np.zeros(len(patterns), np.int64)
    for seed in range(n_seed):
        n_match, chosen = match_and_choose([seq], patterns, seed=seed, backend="numpy", seq_index0=3)
        assert int(n_match[0]) == 40 and set(chosen[0].tolist()) <= set(hit_idx) and len(set(chosen[0].tolist())) == 10
        incl[chosen[0]] += 1
        first[chosen[0, 0]] += 1
    for counts, p in ((incl, 10 / 40), (first, 1 / 40)):
        mean, sigma = n_seed * p, (n_seed * p * (1 - p)) ** 0.5
        dev = np.abs(counts[hit_idx] - mean) / sigma
        print("p", p, "worst deviation", float(dev.max()), "sigma")
        assert dev.max() <= 5.0, (p, counts[hit_idx].tolist())
    assert incl.sum() == 10 * n_seed and first.sum() == n_seed


def test_determinism_seeds_and_batch_independence():
    from dr4sr_amd.pairs import match_and_choose
    z, train, seqs, values, mined = load_fixture()
    a = match_and_choose(seqs, values, seed=11, backend="numpy")
    b = match_and_choose(seqs, values, seed=11, backend="numpy")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    c = match_and_choose(seqs, values, seed=12, backend="numpy")
    assert np.array_equal(a[0], c[0])
    big = np.nonzero(a[0] > 10)[0]
    assert any(not np.array_equal(a[1][i], c[1][i]) for i in big)
    for i in (0, int(big[0]), int(np.argmax(a[0])), len(seqs) - 1):                  # a row alone, told its index in the file
        n1, c1 = match_and_choose([seqs[i]], values, seed=11, backend="numpy", seq_index0=i)
        assert int(n1[0]) == int(a[0][i]) and np.array_equal(c1[0], a[1][i]), i
    d = match_and_choose(seqs, values, seed=11, backend="numpy", seq_chunk=97, threads=1)
    assert np.array_equal(a[0], d[0]) and np.array_equal(a[1], d[1])
    # patterns split by the caller: the same keys through pat_index0
    lo = match_and_choose(seqs[:50], values[:9000], seed=11, backend="numpy")
    hi = match_and_choose(seqs[:50], values[9000:], seed=11, backend="numpy", pat_index0=9000)
    assert np.array_equal(lo[0] + hi[0], a[0][:50])
    assert all(set(a[1][i].tolist()) <= set(lo[1][i].tolist()) | set(hi[1][i].tolist()) for i in range(50))


def test_refusals_and_edge_shapes():
    from dr4sr_amd.pairs import match_and_choose
    with pytest.raises(ValueError, match="empty"):
        match_and_choose([[1, 2]], [[1], []], backend="numpy")
    with pytest.raises(ValueError, match="at most 64"):
        match_and_choose([[1] * 65], [[1]], backend="numpy")
    with pytest.raises(ValueError, match="backend"):
        match_and_choose([[1]], [[1]], backend="torch")
    n, c = match_and_choose([[1, 2, 3], [4]], [], backend="numpy")
    assert n.tolist() == [0, 0] and c.tolist() == [[-1] * 10] * 2
    n, c = match_and_choose([], [[1]], backend="numpy")
    assert n.shape == (0,) and c.shape == (0, 10)
    n, c = match_and_choose([[5, 6, 5]], [[5, 5], [6, 6], [5, 6, 5, 5], [7] * 70], backend="numpy")
    assert n.tolist() == [1] and c[0].tolist() == [0] + [-1] * 9


def rows_plain(rows):
    return [[list(x) if isinstance(x, (tuple, list)) else x for x in r] for r in rows]


def test_pattern_rows_reproduce_the_reference_patterns_pth():
    from dr4sr_amd.pairs import pattern_rows, pattern_values
    z, train, seqs, values, mined = load_fixture()
    assert pattern_values(mined) == values
    got = pattern_rows(values)
    want = [[u, it, tg, sl, lb, dm] for u, it, tg, sl, lb, dm in zip(
        z["ref_pat_user"].tolist(), z["ref_pat_items"].tolist(), z["ref_pat_targets"].tolist(), z["ref_pat_seqlen"].tolist(),
        z["ref_pat_label"].tolist(), z["ref_pat_domain"].tolist())]
    assert len(got) == len(want) and rows_plain(got) == want
    assert isinstance(got[0][1], tuple) and isinstance(got[0][4], list)             # the reference's own types
    assert len(got) < len(values)                                                   # [c] * 51 and [c] * 52 give the same padded row


def test_build_pretraining_dataset_writes_both_files(tmp_path):
    from dr4sr_amd.pairs import build_pretraining_dataset, pattern_rows, sequences_of
    from dr4sr_amd.regen import hybrid_inference, random_state_dict
    z, train, seqs, values, mined = load_fixture()
    root = tmp_path / "dataset" / "tiny" / "tinyd"
    root.mkdir(parents=True)
    n_item = 60
    rng = np.random.default_rng(3)
    rows = []
    for u, sl in enumerate([1, 2, 5, 9, 30, 3, 47], 1):
        it = rng.integers(1, n_item, sl + 1).tolist()
        rows.append([u, it[:sl] + [0] * (L - sl), it[1:] + [0] * (L - sl), sl, [1] * sl + [0] * (L - sl), [0] * L])
    s = sequences_of(rows)
    pats = [[s[4][2], s[4][9], 7], [s[6][0], s[6][47], 3], [s[3][1], s[3][1], 2], [59, 58, 57, 2]] + [[v, 2] for v in sorted(set(s[4]))]
    torch.save(rows, root / "train.pth")
    p_path, q_path = build_pretraining_dataset(str(root) + "/", patterns=pats, seed=9, backend="numpy")
    assert os.path.basename(p_path) == "patterns.pth" and os.path.basename(q_path) == "seq-pat-pair.pth"
    vals = [p[:-1] for p in pats]
    assert torch.load(p_path) == pattern_rows(vals) + rows
    pairs = torch.load(q_path)
    per = [[j for j, p in enumerate(vals) if sublist(p, q)] for q in s]
    assert len(pairs) == sum(min(10, len(m)) for m in per) and max(len(m) for m in per) > 10
    at = 0
    for q, m in zip(s, per):                                       # file order; [sequence, pattern] as lists of ids
        mine = pairs[at:at + min(10, len(m))]
        at += len(mine)
        assert all(a == q and b in [vals[j] for j in m] for a, b in mine)
        assert len({tuple(b) for _, b in mine}) == len(mine)
    # stage 3 reads the written patterns.pth unchanged
    sd = random_state_dict(n_item, K=2, seed=4, std=0.3)
    torch.save(sd, root / "regenerator.pth")
    out = torch.load(hybrid_inference(str(root) + "/", backend="torch", device="cpu"))
    assert out[:len(rows)] == rows and out[len(rows):len(rows) + len(pattern_rows(vals))] == pattern_rows(vals)


def test_cli_needs_seq2pat_or_a_patterns_file(tmp_path):
    z, train, seqs, values, mined = load_fixture()
    torch.save(train[:20], tmp_path / "train.pth")
    torch.save([s for s in seqs[:20]], tmp_path / "seq2pat_data.pth")
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "dr4sr_amd.pairs", "--root_path", str(tmp_path), "--backend", "numpy"], capture_output=True,
                       text=True, env=env, cwd=ROOT)
    assert r.returncode != 0 and "--patterns_file" in r.stderr and "seq2pat" in r.stderr, (r.returncode, r.stderr[-400:])
    assert not (tmp_path / "patterns.pth").exists()
    torch.save(mined[:3000], tmp_path / "mined.pth")
    r = subprocess.run([sys.executable, "-m", "dr4sr_amd.pairs", "--root_path", str(tmp_path), "--backend", "numpy", "--seed", "4",
                        "--patterns_file", str(tmp_path / "mined.pth")], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-400:]
    assert r.stdout.split() == [str(tmp_path / "patterns.pth"), str(tmp_path / "seq-pat-pair.pth")]
    from dr4sr_amd.pairs import match_and_choose, pair_list
    _, chosen = match_and_choose(seqs[:20], values[:3000], seed=4, backend="numpy")
    assert torch.load(tmp_path / "seq-pat-pair.pth") == pair_list(seqs[:20], values[:3000], chosen)


def test_lib_binds_pairs_entry_points():
    from dr4sr_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 10 and lib.dr4sr_abi_version() == 10
    wb = lib.dr4sr_pairs_workspace_bytes

    def al16(n):
        return (n + 15) // 16 * 16
    assert wb(100, 1000, 3) == al16(1000 * 16) + al16(1000 * 8) + al16(100 * 3 * 80) + al16(100 * 3 * 4)
    assert wb(19412, 250000, 0) == al16(250000 * 16) + al16(250000 * 8) + al16(19412 * 27 * 80) + al16(19412 * 27 * 4)   # 607 tiles -> 27 chunks
    assert wb(5, 0, 0) == 16 and wb(0, 0, 0) == 16
    assert wb(-1, 10, 0) == -1 and wb(10, -1, 0) == -1 and wb(10, 10, 65) == -1 and wb(10, 10, -1) == -1 and wb(1 << 31, 1, 0) == -1
    p = C.c_void_p(4096)                                           # never dereferenced by the host-side checks
    big = 1 << 40

    def call(seqs=p, lens=p, S=4, Lmax=51, ids=p, off=p, P=7, n_ids=20, seed=1, i0=0, j0=0, chunks=0, ws=p, nb=big, nm=p, ch=p):
        return lib.dr4sr_pairs_match(seqs, lens, S, Lmax, ids, off, P, n_ids, seed, i0, j0, chunks, ws, nb, nm, ch, None)
    assert call(Lmax=65) == -2                                     # DR4SR_E_SHAPE
    assert call(Lmax=0) == -1
    for kw in ({"seqs": None}, {"lens": None}, {"ids": None}, {"off": None}, {"nm": None}, {"ch": None}, {"S": -1}, {"P": -1}, {"n_ids": -1},
               {"n_ids": 1 << 31}, {"i0": -1}, {"j0": -1}, {"i0": (1 << 31) - 3}, {"j0": (1 << 31) - 6}, {"chunks": 65}, {"chunks": -2}):
        assert call(**kw) == -1, kw                                # DR4SR_E_ARG
    assert call(ws=None) == -3 and call(nb=wb(4, 7, 0) - 1) == -3  # DR4SR_E_WS
    assert call(S=0) == 0                                          # nothing to do, nothing launched
