"""Weight gradients of the latency-regime step with the tokens split over the waves of a workgroup (csrc/linear.hip wgrad_ksplit_body,
k_wgrad_blk<D, F, 2>): one workgroup owns a [64 x 32] block of one weight gradient and a contiguous chunk of one XCD's share of the
tokens, wave w takes the token pairs w, w + 4, ... of it, the four partial blocks are summed through LDS and added with atomics.

Reference: the same step under DR4SR_DETERMINISTIC=1, which computes the weight gradients by another path (whole jobs on the bf16x3 matrix
cores per 64-token tile, partial blocks summed in a fixed order by k_wgrad_det_reduce).  Every gradient of the encoder layers (weights,
biases, LayerNorm) is compared with relerr < TOL = 2e-5 (tests/test_gpu_step_boundary.py's measure and bound); the table gradients are
printed.  Shapes: the token counts at which a split over waves (pairs, four waves), over XCD shares (multiples of 64 tokens) and over
rectangular blocks (linear1 [F x D], linear2 [D x F]) can go wrong.

Measured, worst relerr over the encoder gradients of all cases: 1.67e-5 (T = 1, F = 256, p = 0.5), the same figure with the parent commit's
library: it is the reference path's bf16x3 rounding (NOTEBOOK "Weight gradients: tokens split over the waves")."""
import ctypes as C
import math

import pytest
import torch

from test_gpu_fwd_state_reuse import H, N_ITEMS, NL, relerr

pytestmark = pytest.mark.gpu

TOL = 2e-5

# name -> (L, lengths).  T = 1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 129: one share (64 tokens) and its neighbours, odd tails, fewer pairs than
# waves.  T400: 8 rows of 50, shares of 64 tokens, the last XCD's share is empty.  T461: every share holds tokens (32 pairs each, 8 per wave),
# the last one 13 (odd tail).  T299: about 300 tokens, 64-token shares, XCDs 5..7 without tokens
SHAPES = {"T1": (50, [1]), "T2": (50, [2]), "T3": (50, [1, 2]), "T15": (50, [15]), "T16": (50, [16]), "T17": (50, [17]), "T63": (50, [50, 13]),
          "T64_L64": (64, [64]), "T65": (50, [50, 15]), "T127": (50, [50, 50, 27]), "T129": (50, [50, 50, 29]),
          "T299": (50, [50, 50, 50, 50, 50, 49]), "T400": (50, [50] * 8), "T461": (50, [50] * 9 + [11])}


def _engine(B, dev, F, L=50, p_drop=0.5, lr=1e-3, D=64):
    from test_gpu_parity import _random_params
    from dr4sr_amd.engine import SasrecEngine
    eng = SasrecEngine(N_ITEMS, L, D, H, F, NL, 1e-12, p_drop, B, dev, seed=77, lr=lr)
    eng.load_named(_random_params(N_ITEMS, D, F, NL, L=L, seed=12))
    return eng


def _rows(lengths, L, seed):
    g = torch.Generator().manual_seed(seed)
    n = len(lengths)
    idx, tgt = torch.zeros(n, L, dtype=torch.long), torch.zeros(n, L, dtype=torch.long)
    for i, k in enumerate(lengths):
        idx[i, :k] = torch.randint(1, N_ITEMS, (k,), generator=g)
        tgt[i, :k] = torch.randint(1, N_ITEMS, (k,), generator=g)
    return idx, tgt, torch.tensor(lengths, dtype=torch.long)


def _inputs(dev, L, lengths, seed=8):
    data = tuple(t.to(dev) for t in _rows(lengths, L, seed))
    neg = torch.randint(1, N_ITEMS, (len(lengths), L), generator=torch.Generator().manual_seed(seed + 1)).to(dev)
    return data, neg


def _perm_plan(eng, data, neg, B, **kw):
    dev = eng.device
    perm = torch.arange(B, dtype=torch.int64, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    return eng.make_plan(data[0], data[1], data[2], rows=torch.zeros(B, dtype=torch.int64, device=dev), neg_item=neg, sample_neg=False,
                         perm_sel=(perm, B, 0, counter), **kw)


def _grads(eng):
    torch.cuda.synchronize()
    loss, n = eng.loss_and_count()
    return {k: v.clone() for k, v in eng.normalized_grads().items()}, loss, n


def _assert_close(got, want, n_want, tag):
    g_g, loss_g, n_g = got
    g_w, loss_w, n_w = want
    assert n_g == n_w == n_want, (n_g, n_w, n_want)
    assert math.isfinite(loss_g) and abs(loss_g - loss_w) <= TOL * abs(loss_w), (loss_g, loss_w)
    enc = [k for k in g_w if ".transformer_layer." in k]
    assert enc and any(float(g_w[k].abs().max()) > 0.0 for k in enc)
    worst = 0.0
    for k, v in g_w.items():
        assert bool(torch.isfinite(g_g[k]).all()), k
        e = relerr(g_g[k], v)
        print("%s: %s relerr %.2e" % (tag, k, e))
        if k in enc:
            worst = max(worst, e)
    print("%s: worst encoder relerr %.2e" % (tag, worst))
    for k in enc:
        e = relerr(g_g[k], g_w[k])
        assert e < TOL, (tag, k, e)


def _step(dev, L, lengths, F, p, data, neg, path="fwd_bwd", D=64, **kw):
    B = len(lengths)
    eng = _engine(B, dev, F, L=L, p_drop=p, D=D)
    if path == "train_steps":
        eng.train_steps(_perm_plan(eng, data, neg, B, **kw), 1)
    else:
        eng.fwd_bwd(eng.make_plan(data[0], data[1], data[2], neg_item=neg, sample_neg=False, **kw))
    return _grads(eng)


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("DF", [(64, 128), (64, 256), (128, 128)])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_default_step_equals_deterministic_step(monkeypatch, shape, DF, p):
    dev = torch.device("cuda", 0)
    L, lengths = SHAPES[shape]
    data, neg = _inputs(dev, L, lengths)
    got = _step(dev, L, lengths, DF[1], p, data, neg, D=DF[0])
    monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    want = _step(dev, L, lengths, DF[1], p, data, neg, D=DF[0])
    _assert_close(got, want, sum(lengths), "%s D %d F %d p %.1f" % (shape, DF[0], DF[1], p))


# 40 rows, 1 033 tokens, capacity 2 000 tokens: shares of 192 tokens, XCD 5 holds 73 (odd tail), XCDs 6 and 7 none
B40 = [1 + (i * 37) % 50 for i in range(39)] + [27]


@pytest.mark.parametrize("hint", [1, 1000, 2000])
def test_token_ranges_come_from_the_batch_not_from_the_hint(monkeypatch, hint):
    """expected_tokens far below, near and far above what the batch holds: the chunks are cut from state[T] on the device"""
    dev = torch.device("cuda", 0)
    assert sum(B40) == 1033
    data, neg = _inputs(dev, 50, B40)
    got = _step(dev, 50, B40, 128, 0.5, data, neg, expected_tokens=hint)
    monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    want = _step(dev, 50, B40, 128, 0.5, data, neg, expected_tokens=hint)
    _assert_close(got, want, sum(B40), "hint %d" % hint)


def _weighted(eng, b, neg, phi, uid):
    from dr4sr_amd import _lib
    plan = eng.make_plan(b[0], b[1], b[2], neg_item=neg, sample_neg=False)
    mw = _lib.MetaWeighting()
    mw.phi, mw.user_id, mw.tau = phi.data_ptr(), uid.data_ptr(), 1.0
    _lib.check(_lib.load().dr4sr_sasrec_fwd_bwd_weighted(C.byref(plan), C.byref(mw), _lib.cur_stream()), "dr4sr_sasrec_fwd_bwd_weighted")


@pytest.mark.parametrize("path", ["fwd_bwd", "train_steps", "weighted"])
def test_small_step_behind_a_larger_one_reads_no_stale_rows(monkeypatch, path):
    """8 rows of 40..50 tokens, then 2 rows of 3 and 17 in the same workspace (lr = 0): the rows past T = 20 hold the first step's operands"""
    from dr4sr_amd import _lib
    dev = torch.device("cuda", 0)
    lx, ly = torch.randint(40, 51, (8,), generator=torch.Generator().manual_seed(5)).tolist(), [3, 17]
    bx, negx = _inputs(dev, 50, lx)
    by, negy = _inputs(dev, 50, ly)
    phi = (0.1 * torch.randn(int(_lib.load().dr4sr_meta_param_count(64)), generator=torch.Generator().manual_seed(1))).to(dev)
    uid = torch.arange(1, 9, dtype=torch.int64, device=dev)

    def run():
        eng = _engine(8, dev, 128, lr=0.0)
        if path == "train_steps":
            eng.train_steps(_perm_plan(eng, bx, negx, 8), 1)
            eng.train_steps(_perm_plan(eng, by, negy, 2), 1)
        elif path == "weighted":
            _weighted(eng, bx, negx, phi, uid)
            _weighted(eng, by, negy, phi, uid)
        else:
            eng.fwd_bwd(eng.make_plan(bx[0], bx[1], bx[2], neg_item=negx, sample_neg=False))
            eng.fwd_bwd(eng.make_plan(by[0], by[1], by[2], neg_item=negy, sample_neg=False))
        assert int(eng.state[3]) == 2
        return _grads(eng)

    got = run()
    monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    _assert_close(got, run(), sum(ly), "stale " + path)


def test_three_train_steps_equal_three_deterministic_steps(monkeypatch):
    """train_steps(plan, 3) on T = 461 with lr = 0 (the parameters stay, so the two modes see the same step three times over): the gradients
    the third step of the graph leaves — zeroed between the steps, dropout of RNG step 3"""
    dev = torch.device("cuda", 0)
    L, lengths = SHAPES["T461"]
    data, neg = _inputs(dev, L, lengths)

    def run():
        eng = _engine(len(lengths), dev, 128, L=L, lr=0.0)
        eng.train_steps(_perm_plan(eng, data, neg, len(lengths)), 3)
        torch.cuda.synchronize()
        assert int(eng.state[0]) == 3 and int(eng.state[3]) == 3
        return _grads(eng)

    got = run()
    monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    _assert_close(got, run(), sum(lengths), "train_steps 3")
