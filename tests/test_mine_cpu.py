"""The pattern miner (dr4sr_amd.mine, the first step of DR4SR stage 1) without a GPU: the numpy backend against the brute-force statement
of the rule (tests/_mine_ref.py) on crafted and random cases and against the toys fixture (tests/golden/mine_toys.npz,
tools/make_mine_golden.py), the way its result feeds dr4sr_amd.pairs, the refusals, the CLIs, and the C ABI's host-side checks.
Every comparison is exact: equality of lists of Python ints, order included."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _mine_ref import brute_force

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "mine_toys.npz")
ALPHAS, BETAS = (2, 3, 5, 6, 10), (1, 2, 3)
TOP = 2 ** 31 - 1


@functools.lru_cache(maxsize=None)
def crafted_cases():
    """name -> sequences; what each is there for is its name"""
    rng = np.random.default_rng(300)
    a, b, c = 7, 8, 9
    return {
        "a b b: two masks, one tuple": [[a, b, b], [a, b, b], [a, b]],
        "a a a a a a: many masks, one tuple per length": [[a] * 6, [a] * 6, [a] * 3],
        "twice far apart in one sequence counts once": [[1, 2] + [50 + i for i in range(20)] + [1, 2], [1, 3, 2], [9, 1, 5, 5, 2, 4]],
        "frequency 1, 2 and 3: exactly beta - 1 and exactly beta": [[1, 2, 3, 4, 5, 6], [1, 2, 3, 4], [1, 2], [5, 6, 1]],
        "lengths 0, 1 and 2": [[], [4], [4, 5], [], [4, 5], [5], [5, 4]],
        "300 ids over 3 letters": [rng.integers(1, 4, 300).tolist(), [1, 2, 3, 1, 2, 3], [3, 3, 1]],
        "ids at 2^31 - 1": [[TOP, 5, TOP], [TOP, TOP], [5, TOP - 1, TOP], [TOP - 1, TOP]],
    }


@functools.lru_cache(maxsize=None)
def random_cases(n=200):
    """(sequences, alpha, beta): alphabets 2-30, lengths from {0, 1, 2, 3, 7, 15, 40}, 1-8 sequences"""
    rng = np.random.default_rng(20240)
    out = []
    for _ in range(n):
        V, S = int(rng.integers(2, 31)), int(rng.integers(1, 9))
        seqs = [rng.integers(1, V + 1, int(rng.choice([0, 1, 2, 3, 7, 15, 40]))).tolist() for _ in range(S)]
        out.append((seqs, int(rng.choice(ALPHAS)), int(rng.choice(BETAS))))
    return out


@functools.lru_cache(maxsize=None)
def load_fixture():
    """(sequences, the fixture's result list at alpha 5, beta 2)"""
    z = np.load(GOLD)
    ids, off = z["ids"].astype(np.int64).tolist(), z["off"].tolist()
    seqs = [ids[a:b] for a, b in zip(off[:-1], off[1:])]
    want = [[int(v) for v in row if v] + [int(f)] for row, f in zip(z["pat_ids"].tolist(), z["pat_freq"].tolist())]
    assert int(z["alpha"]) == 5 and int(z["beta"]) == 2
    return seqs, want


@functools.lru_cache(maxsize=None)
def numpy_result(key, alpha, beta):
    """the numpy backend's list for a crafted case (by name), a random case (by index) or the fixture ("toys", or ("toys", n) for its
    first n sequences) — computed once, shared by the tests of both backends, never modified"""
    from dr4sr_amd.mine import mine_patterns
    return mine_patterns(sequences_of_key(key), alpha, beta, backend="numpy")


def sequences_of_key(key):
    if key == "toys":
        return load_fixture()[0]
    if isinstance(key, tuple):
        return load_fixture()[0][:key[1]]
    return crafted_cases()[key] if isinstance(key, str) else random_cases()[key][0]


def test_numpy_equals_brute_force_on_crafted_cases():
    for name, seqs in crafted_cases().items():
        for alpha in ALPHAS:
            for beta in BETAS:
                want = brute_force(seqs, alpha, beta)
                assert numpy_result(name, alpha, beta) == want, (name, alpha, beta)
                assert all(type(v) is int for p in want for v in p)
    # the cases show what their names say
    got = {tuple(p[:-1]): p[-1] for p in numpy_result("a b b: two masks, one tuple", 5, 1)}
    assert got == {(7, 8): 3, (7, 8, 8): 2, (8, 8): 2}
    assert numpy_result("a a a a a a: many masks, one tuple per length", 5, 2) == [[7, 7, 3], [7, 7, 7, 3], [7, 7, 7, 7, 2], [7, 7, 7, 7, 7, 2]]
    far = {tuple(p[:-1]): p[-1] for p in numpy_result("twice far apart in one sequence counts once", 5, 1)}
    assert far[(1, 2)] == 3 and [1, 2, 2] in numpy_result("twice far apart in one sequence counts once", 3, 2)        # 1 5 5 2 is out of reach 2
    f = "frequency 1, 2 and 3: exactly beta - 1 and exactly beta"
    assert [p for p in numpy_result(f, 2, 3)] == [[1, 2, 3]] and [3, 4, 2] in numpy_result(f, 2, 2) and [3, 4, 2] not in numpy_result(f, 2, 3)
    assert numpy_result("lengths 0, 1 and 2", 5, 1) == [[4, 5, 2], [5, 4, 1]]
    assert [TOP, TOP, 2] in numpy_result("ids at 2^31 - 1", 3, 2) and [TOP - 1, TOP, 2] in numpy_result("ids at 2^31 - 1", 3, 2)
    long = numpy_result("300 ids over 3 letters", 10, 1)
    assert max(len(p) for p in long) == 11 and len(long) > 3 ** 6


def test_numpy_equals_brute_force_on_random_cases():
    used = set()
    for i, (seqs, alpha, beta) in enumerate(random_cases()):
        assert numpy_result(i, alpha, beta) == brute_force(seqs, alpha, beta), (i, seqs, alpha, beta)
        used.add((alpha, beta))
    assert len(used) == len(ALPHAS) * len(BETAS)
    # the order: frequency descending, then ids ascending, a prefix before its extensions
    got = numpy_result("a a a a a a: many masks, one tuple per length", 6, 1)
    assert got == sorted(got, key=lambda p: (-p[-1], tuple(p[:-1])))


def test_numpy_reproduces_the_toys_fixture():
    seqs, want = load_fixture()
    assert len(seqs) == 19412 and sum(len(s) for s in seqs) == 128773 and max(len(s) for s in seqs) == 548
    got = numpy_result("toys", 5, 2)
    assert got == want
    assert len(got) == 19726 and [sum(len(p) - 1 == k for p in got) for k in (2, 3, 4, 5)] == [18041, 1549, 128, 8]
    assert got[0][-1] == 64 == max(p[-1] for p in got) and min(p[-1] for p in got) == 2
    from dr4sr_amd.mine import candidate_count, pack
    ids, off = pack(seqs)
    assert candidate_count(off, 5) == 1033039 and candidate_count(off, 8) == 5505439
    # a chunk boundary of the numpy backend changes nothing (the fixture spans many blocks at 1 << 12 candidates each)
    from dr4sr_amd import mine
    whole = mine._CHUNK_CANDIDATES
    try:
        mine._CHUNK_CANDIDATES, mine._MERGE_ROWS = 1 << 12, 1 << 10
        assert mine.mine_patterns(seqs[:600], 5, 2, backend="numpy") == numpy_result(("toys", 600), 5, 2)
    finally:
        mine._CHUNK_CANDIDATES, mine._MERGE_ROWS = whole, 1 << 23


def test_mined_list_feeds_the_pairs_stage():
    from dr4sr_amd.pairs import match_and_choose, matches_numpy, pattern_rows, pattern_values
    seqs = [s for s in load_fixture()[0] if len(s) <= 64][:1500]
    from dr4sr_amd.mine import mine_patterns
    mined = mine_patterns(seqs, 5, 2, backend="numpy")
    values = pattern_values(mined)
    assert len(mined) > 100 and all(2 <= len(v) <= 5 for v in values) and len({tuple(v) for v in values}) == len(values)
    rows = pattern_rows(values)
    assert len(rows) == len(values) and sorted(r[3] for r in rows) == sorted(len(v) - 1 for v in values)
    mi, mj = matches_numpy(seqs, values)
    per_pattern = np.bincount(mj, minlength=len(values))
    freq = np.array([p[-1] for p in mined])
    assert np.all(per_pattern >= freq)                           # an occurrence inside a window is a subsequence
    n_match, chosen = match_and_choose(seqs, values, seed=3, backend="numpy")
    assert int(n_match.sum()) == mi.size and chosen.shape == (len(seqs), 10) and int(chosen.max()) < len(values)


def test_refusals():
    from dr4sr_amd.mine import mine_patterns
    ok = [[1, 2, 3], [1, 2]]
    for alpha in (1, 11, 0, -3, 2.5):
        with pytest.raises(ValueError, match="alpha"):
            mine_patterns(ok, alpha, 2, backend="numpy")
    for beta in (0, -1, 0.5):
        with pytest.raises(ValueError, match="beta"):
            mine_patterns(ok, 5, beta, backend="numpy")
    for bad in (0, -4, 2 ** 31):
        with pytest.raises(ValueError, match="ids must lie in"):
            mine_patterns([[1, 2], [3, bad]], 5, 2, backend="numpy")
    with pytest.raises(ValueError, match="4096"):
        mine_patterns([[1, 2], [1] * 4097], 5, 2, backend="numpy")
    for backend in ("torch", "seq2pat", None):
        with pytest.raises(ValueError, match="backend"):
            mine_patterns(ok, 5, 2, backend=backend)
    with pytest.raises(ValueError, match="alpha"):               # refused before any device is touched
        mine_patterns(ok, 11, 2, backend="hip")
    assert mine_patterns([[1] * 4096, [1, 1]], 2, 2, backend="numpy") == [[1, 1, 2]]
    assert mine_patterns([], 5, 1, backend="numpy") == [] and mine_patterns([[], [3]], 5, 1, backend="numpy") == []
    from dr4sr_amd.pairs import build_pretraining_dataset
    with pytest.raises(ValueError, match="miner"):
        build_pretraining_dataset("/nonexistent", miner="spmf")


def test_cli_mines_without_seq2pat(tmp_path):
    """--miner numpy: patterns.pth and seq-pat-pair.pth from seq2pat_data.pth + train.pth alone, with no `sequential` to import"""
    from test_pairs_cpu import load_fixture as pairs_fixture
    z, train, seqs, values, mined = pairs_fixture()
    train, seqs = train[:400], [[int(v) for v in s] for s in seqs[:400]]
    torch.save(train, tmp_path / "train.pth")
    torch.save(seqs, tmp_path / "seq2pat_data.pth")
    block = tmp_path / "block" / "sequential"                      # any import of `sequential` in the child processes raises
    block.mkdir(parents=True)
    (block / "__init__.py").write_text("raise ImportError('sequential is blocked in this test')\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(block.parent), ROOT]))
    r = subprocess.run([sys.executable, "-m", "dr4sr_amd.pairs", "--root_path", str(tmp_path), "--backend", "numpy", "--miner", "numpy",
                        "--alpha", "4", "--beta", "2", "--seed", "6"], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-600:]
    assert r.stdout.split() == [str(tmp_path / "patterns.pth"), str(tmp_path / "seq-pat-pair.pth")]
    from dr4sr_amd.mine import mine_patterns
    from dr4sr_amd.pairs import match_and_choose, pair_list, pattern_rows, pattern_values
    want = mine_patterns(seqs, 4, 2, backend="numpy")
    vals = pattern_values(want)
    assert len(want) > 50 and torch.load(tmp_path / "patterns.pth") == pattern_rows(vals) + train
    _, chosen = match_and_choose(seqs, vals, seed=6, backend="numpy")
    assert torch.load(tmp_path / "seq-pat-pair.pth") == pair_list(seqs, vals, chosen)
    r = subprocess.run([sys.executable, "-m", "dr4sr_amd.pairs", "--root_path", str(tmp_path), "--backend", "numpy"], capture_output=True,
                       text=True, env=env, cwd=ROOT)                # the default miner does import it, and says what to do instead
    assert r.returncode != 0 and "sequential is blocked" in r.stderr and "--patterns_file" in r.stderr, r.stderr[-600:]
    # the miner's own command line writes what --patterns_file accepts
    out = tmp_path / "mined.pth"
    r = subprocess.run([sys.executable, "-m", "dr4sr_amd.mine", "--root_path", str(tmp_path), "--backend", "numpy", "--alpha", "4",
                        "--out", str(out)], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.split() == [str(out)], r.stderr[-600:]
    assert torch.load(out) == want
    os.remove(tmp_path / "seq-pat-pair.pth")
    r = subprocess.run([sys.executable, "-m", "dr4sr_amd.pairs", "--root_path", str(tmp_path), "--backend", "numpy", "--seed", "6",
                        "--patterns_file", str(out)], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0 and torch.load(tmp_path / "seq-pat-pair.pth") == pair_list(seqs, vals, chosen), r.stderr[-600:]


def test_lib_binds_mine_entry_points():
    from dr4sr_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 10 and lib.dr4sr_abi_version() == 10
    wb = lib.dr4sr_mine_workspace_bytes
    assert wb(1000, 10, 5, 4096) == 4096 * 12 and wb(1000, 10, 5, 1) == 32
    assert wb(1000, 10, 5, 0) == 32768 * 12                       # 1000 * 15 pairs -> the first power of two at or above 30 000
    assert wb(0, 0, 5, 0) == 256 * 12 and wb(128773, 19412, 10, 0) == (1 << 27) * 12
    assert wb(1000, 10, 11, 0) == -2 and wb(1000, 10, 1, 0) == -2
    assert wb(-1, 10, 5, 0) == -1 and wb(10, -1, 5, 0) == -1 and wb(1 << 31, 1, 5, 0) == -1 and wb(10, 1, 5, 3) == -1
    assert wb(10, 1, 5, -2) == -1 and wb(10, 1, 5, 1 << 31) == -1 and wb(1 << 30, 1, 10, 256) == -1
    p = C.c_void_p(4096)                                           # never dereferenced by the host-side checks
    big = 1 << 40

    def call(ids=p, off=p, n_ids=100, n_seq=9, alpha=5, beta=2, slots=0, ws=p, nb=big, out_ids=p, out_freq=p, cap=50, n_out=p, status=p):
        return lib.dr4sr_mine_patterns(ids, off, n_ids, n_seq, alpha, beta, slots, ws, nb, out_ids, out_freq, cap, n_out, status, None)
    assert call(alpha=11) == -2 and call(alpha=1) == -2            # DR4SR_E_SHAPE
    for kw in ({"ids": None}, {"off": None}, {"out_ids": None}, {"out_freq": None}, {"n_out": None}, {"status": None}, {"n_ids": -1},
               {"n_seq": -1}, {"beta": 0}, {"cap": -1}, {"slots": 6}, {"slots": 1 << 31}, {"n_ids": 1 << 31}):
        assert call(**kw) == -1, kw                                # DR4SR_E_ARG
    assert call(ws=None) == -3 and call(nb=wb(100, 9, 5, 0) - 1) == -3 and call(slots=64, nb=64 * 12 - 1) == -3      # DR4SR_E_WS
