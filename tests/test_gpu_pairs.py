"""The regenerator's pre-training pairs on the MI355X (csrc/pairs.hip through dr4sr_pairs_match): the match relation against the
reference's (tests/golden/pairs_toys.npz), exact equality with the numpy restatement, independence of chunking and of the batch, edge
shapes, and the stage 1 files end to end."""
import os
import sys

import numpy as np
import pytest
import torch

from test_pairs_cpu import check_selection, golden_matches, load_fixture

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def synthetic_case(n_seq, n_pat):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from pairs_bench import sample_patterns, toys_sequences
    seqs = toys_sequences(n_seq, seed=77)
    patterns = sample_patterns(seqs, n_pat, seed=5)
    assert sum(len(set(s)) < len(s) for s in seqs) >= n_seq // 16 and sum(len(set(p)) < len(p) for p in patterns) >= n_pat // 60
    return seqs, patterns


def test_hip_matches_the_reference_relation():
    from dr4sr_amd.pairs import match_and_choose
    z, train, seqs, values, mined = load_fixture()
    per = golden_matches(z, len(seqs))
    n_match, chosen = match_and_choose(seqs, values, seed=5, backend="hip")
    assert n_match.dtype == np.int32 and chosen.dtype == np.int32 and chosen.shape == (len(seqs), 10)
    assert n_match.tolist() == [len(s) for s in per]
    check_selection(chosen, per)
    # every matching pattern of every row, not only the ten chosen: with the list cut into 256 interleaved slices no row has more than ten
    # matches per slice, so each call lists all of them, and their union is the whole relation
    got = [set() for _ in seqs]
    for r in range(256):
        n, c = match_and_choose(seqs, values[r::256], seed=r, backend="hip")
        assert int(n.max()) <= 10 and np.array_equal((c >= 0).sum(1), n)
        for i in np.nonzero(n)[0].tolist():
            got[i] |= {r + 256 * k for k in c[i, :n[i]].tolist()}
    assert got == per
    assert same(match_and_choose(seqs, values, seed=5, backend="numpy"), (n_match, chosen))


def test_hip_equals_numpy_on_toys_shaped_data():
    from dr4sr_amd.pairs import match_and_choose
    seqs, patterns = synthetic_case(4096, 30000)
    hip = match_and_choose(seqs, patterns, seed=(9 << 32) | 4, backend="hip")
    ref = match_and_choose(seqs, patterns, seed=(9 << 32) | 4, backend="numpy")
    assert same(hip, ref)
    assert (ref[0] > 10).sum() > 100 and (ref[0] == 0).sum() > 0 and ref[0].max() > 50          # the inputs cover all the classes


def test_result_is_independent_of_chunking_and_batch():
    from dr4sr_amd.pairs import match_and_choose
    seqs, patterns = synthetic_case(1500, 12000)               # 1 500 is not a multiple of the 32-row tile
    one = match_and_choose(seqs, patterns, seed=21, backend="hip")
    assert same(one, match_and_choose(seqs, patterns, seed=21, backend="hip"))
    assert same(one, match_and_choose(seqs, patterns, seed=21, backend="hip", seq_chunk=333))
    for c in (1, 3, 7, 64):                                     # the pattern list forced into c chunks per tile
        assert same(one, match_and_choose(seqs, patterns, seed=21, backend="hip", n_chunks=c)), c
    for i in (0, 31, 32, 700, 1499, int(np.argmax(one[0]))):
        n1, c1 = match_and_choose([seqs[i]], patterns, seed=21, backend="hip", seq_index0=i)
        assert int(n1[0]) == int(one[0][i]) and np.array_equal(c1[0], one[1][i]), i
    # the pattern list split by the caller: counts add up, and the ten chosen are the ten smallest of the parts' choices
    lo = match_and_choose(seqs, patterns[:5000], seed=21, backend="hip")
    hi = match_and_choose(seqs, patterns[5000:], seed=21, backend="hip", pat_index0=5000)
    assert np.array_equal(lo[0] + hi[0], one[0])
    assert all(set(one[1][i].tolist()) <= set(lo[1][i].tolist()) | set(hi[1][i].tolist()) for i in range(len(seqs)))
    other = match_and_choose(seqs, patterns, seed=22, backend="hip")
    assert np.array_equal(other[0], one[0]) and not np.array_equal(other[1], one[1])


def test_edge_shapes():
    from dr4sr_amd.pairs import match_and_choose
    z, train, seqs, values, mined = load_fixture()
    full = [s for s in seqs if len(s) == 51][0]
    for S in (1, 31, 33):                                       # one row, tail tiles
        assert same(match_and_choose(seqs[:S], values, seed=1, backend="hip"), match_and_choose(seqs[:S], values, seed=1, backend="numpy")), S
    n, c = match_and_choose(seqs[:40], [values[0]], seed=1, backend="hip")             # P = 1
    assert same((n, c), match_and_choose(seqs[:40], [values[0]], seed=1, backend="numpy")) and set(c[:, 1:].ravel().tolist()) == {-1}
    n, c = match_and_choose([full, full[:50], full[1:]], [list(full), full[:50], [full[0], full[0]]], seed=1, backend="hip")
    assert n.tolist() == [2, 1, 0] and sorted(c[0, :2].tolist()) == [0, 1] and c[1].tolist() == [1] + [-1] * 9    # a pattern equal to a whole row
    n, c = match_and_choose(seqs[:70], [], seed=1, backend="hip")                      # P = 0
    assert n.tolist() == [0] * 70 and set(c.ravel().tolist()) == {-1}
    n, c = match_and_choose([], values[:10], seed=1, backend="hip")
    assert n.shape == (0,) and c.shape == (0, 10)
    n, c = match_and_choose([[5, 6, 5]] * 3, [[5, 5], [6, 6], [5, 6, 5, 5], [7] * 70, [5, 6, 5]], seed=1, backend="hip")
    assert n.tolist() == [2] * 3 and all(sorted(r[:2]) == [0, 4] and r[2:] == [-1] * 8 for r in c.tolist())


def test_device_refuses_bad_offsets_without_reading_them():
    """offsets are not checked on the host: on the device a pattern whose offsets are not monotonic inside [0, n_ids] matches nothing"""
    import ctypes as C
    from dr4sr_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda")
    seq = torch.tensor([[1, 2, 3, 4]], dtype=torch.int32, device=dev)
    ln = torch.tensor([4], dtype=torch.int32, device=dev)
    ids = torch.tensor([1, 2, 3, 4, 2, 3], dtype=torch.int32, device=dev)
    off = torch.tensor([0, 2, 1, 4, 9, 6], dtype=torch.int64, device=dev)       # patterns: [1,2] ok, (2,1) backwards, [2,3,4] ok, (4,9) past the end, (9,6)
    nb = int(lib.dr4sr_pairs_workspace_bytes(1, 5, 0))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    n = torch.empty(1, dtype=torch.int32, device=dev)
    ch = torch.empty(1, 10, dtype=torch.int32, device=dev)
    _lib.check(lib.dr4sr_pairs_match(_lib.ptr(seq), _lib.ptr(ln), 1, 4, _lib.ptr(ids), _lib.ptr(off), 5, 6, C.c_uint64(3), 0, 0, 0,
                                     C.c_void_p(ws.data_ptr()), nb, _lib.ptr(n), _lib.ptr(ch), _lib.cur_stream()), "dr4sr_pairs_match")
    assert n.tolist() == [2] and sorted(ch[0, :2].tolist()) == [0, 2] and ch[0, 2:].tolist() == [-1] * 8


def test_build_pretraining_dataset_hip_equals_numpy(tmp_path):
    from dr4sr_amd.pairs import build_pretraining_dataset
    z, train, seqs, values, mined = load_fixture()
    out = {}
    for backend in ("hip", "numpy"):
        root = tmp_path / backend
        root.mkdir()
        torch.save(train, root / "train.pth")
        p, q = build_pretraining_dataset(str(root), patterns=mined, seed=13, backend=backend)
        out[backend] = (torch.load(p), torch.load(q))
    assert out["hip"][0] == out["numpy"][0] and out["hip"][1] == out["numpy"][1]
    per = golden_matches(z, len(seqs))
    assert len(out["hip"][1]) == sum(min(10, len(m)) for m in per)
