"""The 16-row d = 64 token-tile kernels with their parameter vectors requested at kernel entry (csrc/linear.hip EntryParams: the biases of
this thread's epilogue columns, gamma / beta of this thread's float4) and the scorer's table adds issued from the backward half of k_post_mid
(TableAdds).  Both changes move loads and atomics, not arithmetic, so what can go wrong is an index: a bias of another column block, gamma
of another float4, the positive row's coefficient on the negative row.  The bench's initialisation (zero biases, unit gamma) shows none of
these; every engine here carries biases of size 0.2 and LayerNorm weights spread over 0.4 .. 1.8 with offsets of size 0.3.

  1. the fused step against the 19-launch DR4SR_NO_FUSE step (row passes and epilogues of the at-scale loads-in-place forms), T = 1, 15, 16,
     17, 33 and 129 tokens, p = 0 and 0.5, default and deterministic mode, fwd_bwd and train_steps, and the MetaModel-weighted launch:
     relerr < 2e-5 on the loss and every gradient (the bound of tests/test_gpu_step_boundary.py; worst case measured on the parent
     library: NOTEBOOK "Parameter loads at kernel entry")
  2. the table gradient with 4 item ids (every row positive and negative target of several tokens of one tile and of both tiles): default
     mode (the moved adds) against the deterministic owner path; targets in the pad tail, n_valid exact
  3. stale state: a 20-token step behind a 300-token step in one workspace; the evaluation forward with the saved-state areas prefilled
  4. two fwd_bwd calls from one RNG step are bit-equal in deterministic mode

Builds that fail these tests (NOTEBOOK, same section): the bias of the neighbouring column block (w + 4 (i + 1) in bias_cols_load) fails
every case of group 1; dpos / dneg exchanged in TableAdds::issue fails group 2 and the default-mode cases of group 1."""
import ctypes as C
import math

import pytest
import torch

from test_gpu_fwd_state_reuse import D, F, H, NL, relerr
from test_gpu_step_boundary import TOL, _assert_close, _grads, _offsets, _perm_plan, _rows

pytestmark = pytest.mark.gpu

L = 50
N_ITEMS = 300
# token counts 1, 15, 16, 17, 33, 129: a sequence across the seam at token 16 (17, 33, 129), one of length L (129), one tile exactly (16)
LENGTHS = {1: [1], 15: [7, 8], 16: [10, 6], 17: [9, 8], 33: [12, 10, 11], 129: [50, 29, 50]}
assert all(sum(v) == k for k, v in LENGTHS.items())


def _params(n_items, seed=12):
    from test_gpu_parity import _random_params
    g = torch.Generator().manual_seed(seed + 1000)
    p = _random_params(n_items, D, F, NL, L=L, seed=seed)
    for n in p:
        if n.endswith(("norm1.weight", "norm2.weight")):
            p[n] = 0.4 + 1.4 * torch.rand(p[n].shape, generator=g)
        elif n.endswith(("norm1.bias", "norm2.bias")):
            p[n] = 0.3 * torch.randn(p[n].shape, generator=g)
        elif n.endswith("bias"):
            p[n] = 0.2 * torch.randn(p[n].shape, generator=g)
    return p


def test_parameters_are_far_from_the_bench_initialisation():
    p = _params(N_ITEMS)
    biases = [n for n in p if n.endswith("bias") and "norm" not in n]
    assert len(biases) == 4 * NL                             # in_proj, out_proj, linear1, linear2
    assert all(float(p[n].abs().min()) > 0.0 and float(p[n].std()) > 0.1 for n in biases)
    for n in p:
        if n.endswith(("norm1.weight", "norm2.weight")):
            assert float(p[n].std()) > 0.3 and len(set(p[n].tolist())) == D
        if n.endswith(("norm1.bias", "norm2.bias")):
            assert float(p[n].std()) > 0.2


def _engine(B, dev, n_items=N_ITEMS, p_drop=0.5, lr=1e-3):
    from dr4sr_amd.engine import SasrecEngine
    eng = SasrecEngine(n_items, L, D, H, F, NL, 1e-12, p_drop, B, dev, seed=77, lr=lr)
    eng.load_named(_params(n_items))
    return eng


def _inputs(dev, lengths, n_items=N_ITEMS, seed=8):
    data = tuple(t.to(dev) for t in _rows(lengths, L, n_items, seed=seed))
    neg = torch.randint(1, n_items, (len(lengths), L), generator=torch.Generator().manual_seed(seed + 1)).to(dev)
    return data, neg


def _weighting(dev, B):
    from dr4sr_amd import _lib
    phi = (0.1 * torch.randn(int(_lib.load().dr4sr_meta_param_count(D)), generator=torch.Generator().manual_seed(1))).to(dev)
    return phi, torch.arange(1, B + 1, dtype=torch.int64, device=dev)


def _run(eng, data, neg, path, weighting=None):
    from dr4sr_amd import _lib
    B = int(data[2].numel())
    if path == "train_steps":
        eng.train_steps(_perm_plan(eng, data, neg, B), 1)
    elif path == "weighted":
        plan = eng.make_plan(data[0], data[1], data[2], neg_item=neg, sample_neg=False)
        mw = _lib.MetaWeighting()
        mw.phi, mw.user_id, mw.tau = weighting[0].data_ptr(), weighting[1].data_ptr(), 1.0
        _lib.check(_lib.load().dr4sr_sasrec_fwd_bwd_weighted(C.byref(plan), C.byref(mw), _lib.cur_stream()), "dr4sr_sasrec_fwd_bwd_weighted")
    else:
        eng.fwd_bwd(eng.make_plan(data[0], data[1], data[2], neg_item=neg, sample_neg=False))
    return _grads(eng)


# ------------------------------------------------------------------------------------------------ 1. fused against the 19-launch step
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("path", ["fwd_bwd", "train_steps", "weighted"])
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("T", sorted(LENGTHS))
def test_fused_step_equals_unfused_step(monkeypatch, T, p, path, det):
    if det:
        monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    dev = torch.device("cuda", 0)
    lengths = LENGTHS[T]
    data, neg = _inputs(dev, lengths)
    wt = _weighting(dev, len(lengths)) if path == "weighted" else None
    fused = _run(_engine(len(lengths), dev, p_drop=p), data, neg, path, wt)
    monkeypatch.setenv("DR4SR_NO_FUSE", "1")
    unfused = _run(_engine(len(lengths), dev, p_drop=p), data, neg, path, wt)
    _assert_close(fused, unfused, T, "T %d p %.1f %s det %d" % (T, p, path, det))


# ------------------------------------------------------------------------------------------------ 2. table gradient under collisions
CN = 5                                                       # ids 1 .. 4
C_LENGTHS = [20, 13]                                         # 33 tokens: tiles 0, 1 and one token of tile 2


def _collision_batch(dev, tail):
    """token t of the packed batch: positive target 1 + t % 4, negative 1 + (t + t // 4) % 4 — every id four times positive and four times
    negative target in each full tile, and for the first four tokens of a tile both at once"""
    idx, tgt, sl = _rows(C_LENGTHS, L, CN, seed=21)
    neg = torch.randint(1, CN, (len(C_LENGTHS), L), generator=torch.Generator().manual_seed(22))
    t = 0
    for i, k in enumerate(C_LENGTHS):
        for pos in range(k):
            tgt[i, pos], neg[i, pos] = 1 + t % 4, 1 + (t + t // 4) % 4
            t += 1
    if tail:                                                 # valid targets behind the sequences' ends: loss terms and n_valid only
        tgt[0, 20:27] = torch.tensor([1, 0, 2, 3, 0, 4, 1])
        tgt[1, 49] = 2
    return (idx.to(dev), tgt.to(dev), sl.to(dev)), neg.to(dev), int((tgt != 0).sum())


def test_collision_batch_reuses_every_row_inside_and_across_tiles():
    (idx, tgt, sl), neg, _ = _collision_batch(torch.device("cpu"), False)
    flat_t = torch.cat([tgt[i, :k] for i, k in enumerate(C_LENGTHS)])
    flat_n = torch.cat([neg[i, :k] for i, k in enumerate(C_LENGTHS)])
    for tile in (flat_t[:16], flat_t[16:32]):
        for item in range(1, CN):
            assert int((tile == item).sum()) >= 2, (item, tile)
    for item in range(1, CN):                               # positive AND negative target inside tile 0 and inside tile 1
        assert all(bool((flat_t[s] == item).any()) and bool((flat_n[s] == item).any()) for s in (slice(0, 16), slice(16, 32)))


@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_table_gradient_equals_the_owner_path(monkeypatch, p, tail):
    dev = torch.device("cuda", 0)
    data, neg, n_want = _collision_batch(dev, tail)
    assert n_want == sum(C_LENGTHS) + (6 if tail else 0)
    atomics = _run(_engine(len(C_LENGTHS), dev, n_items=CN, p_drop=p), data, neg, "fwd_bwd")
    monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    owner = _run(_engine(len(C_LENGTHS), dev, n_items=CN, p_drop=p), data, neg, "fwd_bwd")
    assert atomics[2] == owner[2] == n_want, (atomics[2], owner[2], n_want)
    print("loss atomics %.7f owner %.7f" % (atomics[1], owner[1]))
    assert math.isfinite(owner[1]) and abs(atomics[1] - owner[1]) < TOL * abs(owner[1])
    dE_a, dE_o = atomics[0]["item_embedding.weight"], owner[0]["item_embedding.weight"]
    assert bool(torch.isfinite(dE_a).all()) and float(dE_o[0].abs().max()) == 0.0
    assert all(float(dE_o[i].abs().max()) > 0.0 for i in range(1, CN))
    rows = [relerr(dE_a[i], dE_o[i]) for i in range(1, CN)]
    print("dE relerr %.2e, per row" % relerr(dE_a, dE_o), ["%.2e" % e for e in rows])
    assert relerr(dE_a, dE_o) < TOL and max(rows) < TOL


# ------------------------------------------------------------------------------------------------ 3. stale state
def _long_short(dev):
    long_, short = [50] * 6, [3, 17]                         # 300 tokens, then 20
    return _inputs(dev, long_, seed=30), _inputs(dev, short, seed=32), long_, short


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("path", ["fwd_bwd", "train_steps"])
def test_short_step_behind_a_long_step(monkeypatch, path, det):
    """20 tokens behind 300 in one workspace (lr = 0: the parameters stay) against a fresh engine at the same RNG step: bitwise in deterministic
    mode, within the bound of group 1 in default mode"""
    if det:
        monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    dev = torch.device("cuda", 0)
    (dx, nx), (dy, ny), long_, short = _long_short(dev)
    e1 = _engine(len(long_), dev, lr=0.0)
    _run(e1, dx, nx, path)
    got = _run(e1, dy, ny, path)
    assert int(e1.state[3]) == 2
    e2 = _engine(len(long_), dev, lr=0.0)
    e2.state[3] = 1
    want = _run(e2, dy, ny, path)
    _assert_close(got, want, sum(short), "stale %s det %d" % (path, det))
    if det:
        assert got[1] == want[1]
        for k, v in want[0].items():
            assert torch.equal(got[0][k], v), k


def test_evaluation_forward_ignores_prefilled_saved_state(monkeypatch):
    """training = 0 on an engine with p = 0.5 whose saved-state areas (row state, keep words) hold NaN / a pattern: the queries are those of a
    clean engine bit for bit (no atomics in the forward), and the DR4SR_NO_FUSE forward's within the bound"""
    from dr4sr_amd import _lib
    dev = torch.device("cuda", 0)
    lengths = LENGTHS[129]
    data, _ = _inputs(dev, lengths)

    def queries(prefill):
        eng = _engine(len(lengths), dev)
        plan = eng.make_plan(data[0], data[1], data[2])
        if prefill:
            for w in _offsets(eng, plan)[0]:
                for name, (o, n) in w.items():
                    if name in ("attn_keep", "row_keep"):
                        eng.workspace[o:o + n].fill_(0xA5)
                    else:
                        eng.workspace[o:o + n].view(torch.float32).fill_(float("nan"))
        q = eng.encode(plan, False, _lib.POOL_ORIGIN)
        torch.cuda.synchronize()
        return q.clone()

    q_clean, q_fill = queries(False), queries(True)
    assert bool(torch.isfinite(q_clean).all()) and float(q_clean.abs().max()) > 0.0
    assert torch.equal(q_fill, q_clean)
    monkeypatch.setenv("DR4SR_NO_FUSE", "1")
    e = relerr(q_fill, queries(False))
    print("evaluation queries relerr %.2e" % e)
    assert e < TOL


# ------------------------------------------------------------------------------------------------ 4. repeatability
@pytest.mark.parametrize("T", [17, 129])
def test_two_calls_from_one_rng_step_are_bit_equal(monkeypatch, T):
    monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    dev = torch.device("cuda", 0)
    lengths = LENGTHS[T]
    data, neg = _inputs(dev, lengths)
    eng = _engine(len(lengths), dev)
    plan = eng.make_plan(data[0], data[1], data[2], neg_item=neg, sample_neg=False)
    eng.fwd_bwd(plan)
    torch.cuda.synchronize()
    g1, (l1, n1) = eng.grads.clone(), eng.loss_and_count()
    eng.state[3] = 0
    eng.fwd_bwd(plan)
    torch.cuda.synchronize()
    assert int(eng.state[3]) == 1 and n1 == T
    assert eng.loss_and_count() == (l1, n1)
    assert bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0.0
    assert torch.equal(eng.grads, g1)
