"""The pattern miner on the MI355X (csrc/mine.hip through dr4sr_mine_patterns): exact equality with the numpy backend on the crafted and
random cases of tests/test_mine_cpu.py and on the toys fixture, independence of the table's size and of the run, the defined error path of
a table that is too small, the C ABI's return codes, an output buffer smaller than the result, and stage 1 end to end."""
import ctypes as C
import os
import time

import numpy as np
import pytest
import torch

from test_mine_cpu import ALPHAS, BETAS, crafted_cases, load_fixture, numpy_result, random_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hip(seqs, alpha, beta, **kw):
    from dr4sr_amd.mine import mine_patterns
    return mine_patterns(seqs, alpha, beta, backend="hip", **kw)


def pow2_at_least(n):
    s = 1
    while s < n:
        s <<= 1
    return s


def test_hip_equals_numpy_on_crafted_and_random_cases():
    for name, seqs in crafted_cases().items():
        for alpha in ALPHAS:
            for beta in BETAS:
                got = hip(seqs, alpha, beta)
                assert got == numpy_result(name, alpha, beta), (name, alpha, beta)
                assert all(type(v) is int for p in got for v in p)
    for i, (seqs, alpha, beta) in enumerate(random_cases()):
        assert hip(seqs, alpha, beta) == numpy_result(i, alpha, beta), (i, seqs, alpha, beta)


def test_hip_equals_numpy_on_the_toys_fixture():
    seqs, want = load_fixture()
    assert hip(seqs, 5, 2) == want == numpy_result("toys", 5, 2)
    assert hip(seqs, 3, 3) == numpy_result("toys", 3, 3)
    assert hip(seqs, 8, 2) == numpy_result("toys", 8, 2)


def test_many_two_id_sequences_and_no_candidates():
    rng = np.random.default_rng(8)
    seqs = rng.integers(1, 40, (5000, 2)).tolist()                # 5 000 sequences of 2 ids: one candidate each, many workgroups
    from _mine_ref import brute_force
    for alpha, beta in ((2, 1), (5, 3), (10, 4)):
        assert hip(seqs, alpha, beta) == brute_force(seqs, alpha, beta), (alpha, beta)
    assert hip([[1], [2], [], [3]], 5, 1) == [] and hip([], 5, 1) == [] and hip([[], []], 2, 1) == []
    assert hip([[4, 4]], 2, 1) == [[4, 4, 1]] and hip([[4, 4]], 2, 2) == []


def test_result_is_independent_of_the_table_and_of_the_run():
    from dr4sr_amd.mine import candidate_count, mine_hip_raw, pack
    name = "300 ids over 3 letters"
    for key, seqs, alpha in ((("toys", 2000), load_fixture()[0][:2000], 5), (name, crafted_cases()[name], 6)):
        want = numpy_result(key, alpha, 2)
        distinct = len(numpy_result(key, alpha, 1))
        tight = pow2_at_least(distinct)                           # the fullest table that still holds every tuple: long probe chains
        ids, off = pack(seqs)
        _, _, stats = mine_hip_raw(ids, off, alpha, 2, tight)
        assert stats["distinct_tuples"] == distinct and stats["table_slots"] == tight and stats["load_factor"] > 0.5
        assert stats["mean_probe_length"] >= 1.0 and candidate_count(off, alpha) >= distinct
        first = hip(seqs, alpha, 2, table_slots=tight)
        assert first == want, key
        assert hip(seqs, alpha, 2, table_slots=tight) == first                    # two runs
        assert hip(seqs, alpha, 2, table_slots=4 * tight) == first                # two sizes
        assert hip(seqs, alpha, 2) == first                                       # the default size


def test_a_table_that_is_too_small_is_a_defined_error():
    from dr4sr_amd._lib import Dr4srError
    seqs = load_fixture()[0][:2000]
    distinct = len(numpy_result(("toys", 2000), 5, 1))
    assert distinct > 4096
    t0 = time.perf_counter()
    for slots in (1, 64, pow2_at_least(distinct) // 2):
        with pytest.raises(Dr4srError, match="table of %d slots" % slots):
            hip(seqs, 5, 2, table_slots=slots)
    assert time.perf_counter() - t0 < 5.0                          # probing is bounded by the table's size: the calls return promptly
    assert hip(seqs, 5, 2) == numpy_result(("toys", 2000), 5, 2)   # and the next call is unaffected


def raw_call(seqs, alpha, beta, cap, rows, slots=0, ws_short=0, **over):
    """dr4sr_mine_patterns with out buffers of `rows` rows filled with -7; -> (rc, n_out, out_ids, out_freq, status)"""
    from dr4sr_amd import _lib
    from dr4sr_amd.mine import pack
    lib = _lib.load()
    dev = torch.device("cuda")
    ids, off = pack(seqs)
    d_ids, d_off = torch.from_numpy(ids).to(dev), torch.from_numpy(off).to(dev)
    nb = int(lib.dr4sr_mine_workspace_bytes(ids.size, len(seqs), min(max(alpha, 2), 10), slots))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    out_ids = torch.full((rows, max(alpha, 1)), -7, dtype=torch.int32, device=dev)
    out_freq = torch.full((rows,), -7, dtype=torch.int32, device=dev)
    n_out = torch.full((1,), -7, dtype=torch.int32, device=dev)
    status = torch.full((4,), -7, dtype=torch.int64, device=dev)
    a = dict(ids=_lib.ptr(d_ids), off=_lib.ptr(d_off), ws=C.c_void_p(ws.data_ptr()), out_ids=_lib.ptr(out_ids), out_freq=_lib.ptr(out_freq),
             n_out=_lib.ptr(n_out), status=_lib.ptr(status))
    a.update(over)
    rc = lib.dr4sr_mine_patterns(a["ids"], a["off"], ids.size, len(seqs), alpha, beta, slots, a["ws"], nb - ws_short, a["out_ids"], a["out_freq"],
                                 cap, a["n_out"], a["status"], _lib.cur_stream())
    torch.cuda.synchronize()
    return rc, int(n_out), out_ids.cpu().numpy(), out_freq.cpu().numpy(), status.tolist()


def test_return_codes_and_a_short_output_buffer():
    from dr4sr_amd import _lib
    lib = _lib.load()
    seqs = load_fixture()[0][:500]
    want = numpy_result(("toys", 500), 5, 1)
    assert len(want) > 300
    assert lib.dr4sr_mine_workspace_bytes(100, 9, 11, 0) == -2 and lib.dr4sr_mine_workspace_bytes(-1, 9, 5, 0) == -1
    assert raw_call(seqs, 5, 1, 10, 16, ws_short=1)[0] == -3       # DR4SR_E_WS; nothing was launched: the buffers keep their fill
    assert raw_call(seqs, 11, 1, 10, 16)[:2] == (-2, -7)           # DR4SR_E_SHAPE
    for name in ("ids", "off", "out_ids", "out_freq", "n_out", "status"):
        rc, n, oi, of, st = raw_call(seqs, 5, 1, 10, 16, **{name: None})
        assert rc == -1 and (name == "n_out" or n == -7) and set(of.tolist()) == {-7}, name       # DR4SR_E_ARG
    assert raw_call(seqs, 5, 1, 10, 16, ws=None)[0] == -3
    # cap below the result: n_out holds the whole count, the first cap rows are patterns of the result, nothing is written past them
    cap, rows = 100, 160
    rc, n, oi, of, st = raw_call(seqs, 5, 1, cap, rows)
    assert rc == 0 and n == len(want) and st[0] == 0 and st[1] == len(want) and st[3] == 0
    assert set(oi[cap:].ravel().tolist()) == {-7} and set(of[cap:].tolist()) == {-7}
    all_rows = {tuple(p[:-1]) + (0,) * (6 - len(p)): p[-1] for p in want}
    got = {tuple(r): f for r, f in zip(oi[:cap].tolist(), of[:cap].tolist())}
    assert len(got) == cap and all(all_rows.get(r) == f for r, f in got.items())
    rc, n, oi, of, st = raw_call(seqs, 5, 1, len(want), len(want) + 8)
    assert rc == 0 and n == len(want) and {tuple(r): f for r, f in zip(oi[:n].tolist(), of[:n].tolist())} == all_rows
    rc, n, oi, of, st = raw_call(seqs, 5, 1, 0, 4)                  # cap 0: counted only
    assert rc == 0 and n == len(want) and set(of.tolist()) == {-7}
    # the Python wrapper sizes its second call by the counter
    from dr4sr_amd.mine import canonical, mine_hip_raw, pack
    ids2d, freq, stats = mine_hip_raw(*pack(seqs), 5, 1, cap=7)
    assert stats["calls"] == 2 and canonical(ids2d, freq) == want


def test_build_pretraining_dataset_with_the_hip_miner(tmp_path):
    from dr4sr_amd.pairs import build_pretraining_dataset
    from test_pairs_cpu import load_fixture as pairs_fixture
    z, train, seqs, values, mined = pairs_fixture()
    train, seqs = train[:400], [[int(v) for v in s] for s in seqs[:400]]
    out = {}
    for miner in ("hip", "numpy"):
        root = tmp_path / miner
        root.mkdir()
        torch.save(train, root / "train.pth")
        torch.save(seqs, root / "seq2pat_data.pth")
        p, q = build_pretraining_dataset(str(root), alpha=5, beta=2, seed=13, backend=miner, miner=miner)
        out[miner] = (torch.load(p), torch.load(q))
    assert out["hip"][0] == out["numpy"][0] and out["hip"][1] == out["numpy"][1]
    assert len(out["hip"][0]) > len(train) and len(out["hip"][1]) > 0
