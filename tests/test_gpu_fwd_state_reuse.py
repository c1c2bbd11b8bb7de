"""State that the latency-regime step hands from its forward work to its backward work — row-pass activations and dropout keep decisions
carried in registers across the two halves of k_post_mid, keep bits stored by k_post_fwd for k_post_bwd (csrc/linear.hip RowCarry,
row_keep_saved) — must belong to THIS step's batch.  The parity suite checks one batch per engine; these cases run a batch right behind
ANOTHER one (more tokens, longer sequences) in the same workspace and ask for the result a fresh engine gives.

Deterministic mode (DR4SR_DETERMINISTIC=1), dropout 0.5, d = 64: every reduction has a fixed order, so "equal" means bitwise.
The last case runs the default (fp32-atomic) mode on shapes the fuzz does not pin, fused step against the 19-launch DR4SR_NO_FUSE step, which
regenerates every dropout decision with Philox: relerr < 2e-5, the tolerance tests/test_gpu_r2_paths.py uses between two forms of one step."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

N_ITEMS, L, D, H, F, NL = 1500, 50, 64, 2, 128, 2


def relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / max(1e-12, float(b.abs().max())))


def _rows(lengths, seed):
    """dataset-shaped tensors (in_item_id, item_id, seqlen) with the given valid lengths, ids in 1..N_ITEMS-1"""
    g = torch.Generator().manual_seed(seed)
    n = len(lengths)
    idx, tgt = torch.zeros(n, L, dtype=torch.long), torch.zeros(n, L, dtype=torch.long)
    for i, k in enumerate(lengths):
        idx[i, :k] = torch.randint(1, N_ITEMS, (k,), generator=g)
        tgt[i, :k] = torch.randint(1, N_ITEMS, (k,), generator=g)
    return idx, tgt, torch.tensor(lengths, dtype=torch.long)


def _batch_xy(B):
    """X: B long sequences (40..50 tokens); Y: B short ones of mixed lengths whose token count is not a multiple of 16"""
    g = torch.Generator().manual_seed(5)
    lx = torch.randint(40, 51, (B,), generator=g).tolist()
    ly = torch.randint(1, 21, (B,), generator=g).tolist()
    ly[0], ly[1], ly[2] = 1, 17, 16
    if sum(ly) % 16 == 0:
        ly[3] += 1
    assert sum(ly) % 16 != 0 and sum(ly) < sum(lx) // 2
    return lx, ly


def _engine(B, dev, p_drop=0.5, lr=1e-3):
    from test_gpu_parity import _random_params
    from dr4sr_amd.engine import SasrecEngine
    eng = SasrecEngine(N_ITEMS, L, D, H, F, NL, 1e-12, p_drop, B, dev, seed=77, lr=lr)
    eng.load_named(_random_params(N_ITEMS, D, F, NL, seed=12))
    return eng


def _perm_plan(eng, data, B, counter):
    """plan over the 2 B dataset rows: batch k of the permutation = rows [k B, (k + 1) B) — batch 0 is X, batch 1 is Y"""
    dev = eng.device
    perm = torch.arange(2 * B, dtype=torch.int64, device=dev)
    neg = torch.zeros(B, L, dtype=torch.int64, device=dev)
    return eng.make_plan(data[0], data[1], data[2], rows=torch.zeros(B, dtype=torch.int64, device=dev), neg_item=neg, sample_neg=True,
                         perm_sel=(perm, B, 0, counter))


def _result(eng):
    torch.cuda.synchronize()
    loss, n = eng.loss_and_count()
    return eng.grads.clone(), loss, n


def _assert_same(got, want):
    g1, l1, n1 = got
    g2, l2, n2 = want
    assert n1 == n2 and n1 > 0
    assert l1 == l2, (l1, l2)
    assert bool(torch.isfinite(g2).all()) and float(g2.abs().max()) > 0.0
    assert torch.equal(g1, g2), "max |diff| %.3e" % float((g1 - g2).abs().max())


@pytest.mark.parametrize("path", ["train_steps", "prepared", "fwd_bwd"])
def test_step_behind_a_larger_batch_equals_a_fresh_engine(monkeypatch, path):
    """Engine 1 runs a step on X, then a step on Y with the parameters at their initial values and the same RNG step; engine 2 (fresh
    workspace) runs only Y's step: gradients, loss and n_valid bitwise equal.
      train_steps: two consecutive steps of one call, Y prepared inside X's optimizer launch; lr = 0, so Adam leaves the parameters bit
                   for bit where they were (the moments move, no gradient reads them)
      prepared:    the same launches through the two-call API, with parameters, moments and step counter reset by hand in between
      fwd_bwd:     both steps prepared by k_prep"""
    monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    dev = torch.device("cuda", 0)
    B = 48
    lx, ly = _batch_xy(B)
    data = tuple(t.to(dev) for t in _rows(lx + ly, seed=3))
    lr = 0.0 if path == "train_steps" else 1e-3

    e1 = _engine(B, dev, lr=lr)
    p0 = e1.params.clone()
    c1 = torch.zeros(1, dtype=torch.int32, device=dev)
    plan1 = _perm_plan(e1, data, B, c1)
    if path == "train_steps":
        e1.train_steps(plan1, 2)
        assert torch.equal(e1.params, p0)
    elif path == "prepared":
        e1.fwd_bwd(plan1)
        e1.adam_step_prepare_next(plan1)                 # Adam of X's step + prep of Y (batch selection, scan, RNG step) in one launch
        e1.params.copy_(p0); e1.adam_m.zero_(); e1.adam_v.zero_(); e1.state[0] = 0
        e1.fwd_bwd_prepared(plan1)
    else:
        e1.fwd_bwd(plan1)
        e1.adam_step(plan1)
        e1.params.copy_(p0); e1.adam_m.zero_(); e1.adam_v.zero_(); e1.state[0] = 0
        e1.fwd_bwd(plan1)
    got = _result(e1)
    assert int(c1) == 2 and int(e1.state[3]) == 2
    assert got[2] <= sum(ly)

    e2 = _engine(B, dev, lr=lr)
    c2 = torch.ones(1, dtype=torch.int32, device=dev)    # the permutation's batch 1 = Y
    e2.state[3] = 1                                      # ... at the RNG step engine 1 ran it with
    plan2 = _perm_plan(e2, data, B, c2)
    if path == "train_steps":
        e2.train_steps(plan2, 1)
    else:
        e2.fwd_bwd(plan2)
    want = _result(e2)
    assert int(e2.state[3]) == 2
    _assert_same(got, want)


def test_weighted_step_behind_a_larger_batch_equals_a_fresh_engine(monkeypatch):
    """the MetaModel-weighted launch (k_post_mid<.., META>) on one pair of batches"""
    from dr4sr_amd import _lib
    monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    dev = torch.device("cuda", 0)
    B = 48
    lx, ly = _batch_xy(B)
    bx = tuple(t.to(dev) for t in _rows(lx, seed=3))
    by = tuple(t.to(dev) for t in _rows(ly, seed=4))
    lib = _lib.load()
    n_phi = int(lib.dr4sr_meta_param_count(D))
    phi = (0.1 * torch.randn(n_phi, generator=torch.Generator().manual_seed(1))).to(dev)
    uid = torch.arange(1, B + 1, dtype=torch.int64, device=dev)
    neg = torch.randint(1, N_ITEMS, (B, L), generator=torch.Generator().manual_seed(2)).to(dev)

    def weighted(eng, b):
        plan = eng.make_plan(b[0], b[1], b[2], neg_item=neg, sample_neg=False)
        mw = _lib.MetaWeighting()
        mw.phi, mw.user_id, mw.tau = phi.data_ptr(), uid.data_ptr(), 1.0
        _lib.check(lib.dr4sr_sasrec_fwd_bwd_weighted(C.byref(plan), C.byref(mw), _lib.cur_stream()), "dr4sr_sasrec_fwd_bwd_weighted")

    e1 = _engine(B, dev)
    weighted(e1, bx)
    weighted(e1, by)
    got = _result(e1)
    e2 = _engine(B, dev)
    e2.state[3] = 1
    weighted(e2, by)
    _assert_same(got, _result(e2))


def test_evaluation_forward_behind_a_training_step_equals_a_fresh_engine(monkeypatch):
    """training = 0 writes and reads no saved dropout state: the queries of Y right after a training step on X, bitwise"""
    from dr4sr_amd import _lib
    monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    dev = torch.device("cuda", 0)
    B = 48
    lx, ly = _batch_xy(B)
    bx = tuple(t.to(dev) for t in _rows(lx, seed=3))
    by = tuple(t.to(dev) for t in _rows(ly, seed=4))
    e1 = _engine(B, dev)
    e1.fwd_bwd(e1.make_plan(bx[0], bx[1], bx[2]))
    q1 = e1.encode(e1.make_plan(by[0], by[1], by[2]), False, _lib.POOL_ORIGIN)
    e2 = _engine(B, dev)
    q2 = e2.encode(e2.make_plan(by[0], by[1], by[2]), False, _lib.POOL_ORIGIN)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(q2).all()) and float(q2.abs().max()) > 0.0
    assert torch.equal(q1, q2)


_SHAPES = {
    "all_length_1": [1] * 40,
    "one_50_token_sequence_over_four_tiles": [3, 5, 2, 50, 4, 1, 7, 2, 6],      # tokens 10..59: tiles 0, 1, 2 and 3
    "B1": [23],
    "B7": [4, 50, 1, 16, 17, 9, 33],
}


@pytest.mark.parametrize("shape", sorted(_SHAPES))
def test_fused_step_equals_unfused_step_on_odd_shapes(monkeypatch, shape):
    """default (atomic) mode, dropout 0.5: the fused step — state carried and saved by the forward — against the DR4SR_NO_FUSE step of a second
    engine at the same RNG step"""
    dev = torch.device("cuda", 0)
    lengths = _SHAPES[shape]
    B = len(lengths)
    b = tuple(t.to(dev) for t in _rows(lengths, seed=8))
    neg = torch.randint(1, N_ITEMS, (B, L), generator=torch.Generator().manual_seed(9)).to(dev)

    def step():
        eng = _engine(B, dev)
        eng.fwd_bwd(eng.make_plan(b[0], b[1], b[2], neg_item=neg, sample_neg=False))
        torch.cuda.synchronize()
        loss, n = eng.loss_and_count()
        return {k: v.clone() for k, v in eng.normalized_grads().items()}, loss, n

    g_f, loss_f, n_f = step()
    monkeypatch.setenv("DR4SR_NO_FUSE", "1")
    g_u, loss_u, n_u = step()
    assert n_f == n_u == sum(lengths)
    print("%s: loss fused %.7f unfused %.7f" % (shape, loss_f, loss_u))
    assert abs(loss_f - loss_u) < 2e-5 * abs(loss_u)
    for k, v in g_u.items():
        e = relerr(g_f[k], v)
        print("%s: %s relerr %.2e" % (shape, k, e))
        assert e < 2e-5, (k, e)
