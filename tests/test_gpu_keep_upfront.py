"""The KU forms of the latency-regime step (csrc/linear.hip: row_keep_word, k_post_fwd<.., KB>, k_post_mid<.., KU>): the three row passes of
a forward body take their dropout decisions from one 16-bit word that two Philox calls per thread and an exchange between the lanes of a pair
produce ahead of the passes.

  1. fused step against the 19-launch DR4SR_NO_FUSE step of a second engine at the same RNG step.  The unfused kernels regenerate every
     decision with drop4 inside the pass that uses it, so a wrong nibble, a swapped partner or a shifted call index changes half of a mask:
     relerr < 2e-5, the tolerance tests/test_gpu_r2_paths.py and tests/test_gpu_fwd_state_reuse.py use between two forms of one step.
     (Measured: <= 3.4e-6; builds that hand over the wrong nibble, or swap j = 0 and j = 1, fail every case of this group.)
  2. the pad tail of k_post_mid's scorer, sample_neg = True: the whole [B, L] negative buffer against
     oracle.cl4srec_oracle.neg_sample_mirror — the tokens' own positions are written by the tokens' lanes, the pad positions by the lanes
     of the sequence's last token —, and a batch with valid targets behind seqlen against the unfused step.

Engine as tests/test_gpu_fwd_state_reuse.py builds it: N = 1 500, d = 64, F = 128, 2 layers."""
import ctypes as C

import pytest
import torch

from test_gpu_fwd_state_reuse import D, F, H, N_ITEMS, NL, _engine, _rows, relerr

pytestmark = pytest.mark.gpu

TOL = 2e-5
LENGTHS = {"1": [1], "16": [16], "15_2": [15, 2], "50": [50], "B7": [4, 50, 1, 16, 17, 9, 33]}


def _grads(eng):
    torch.cuda.synchronize()
    loss, n = eng.loss_and_count()
    return {k: v.clone() for k, v in eng.normalized_grads().items()}, loss, n


def _assert_close(fused, unfused, n_want, tag):
    g_f, loss_f, n_f = fused
    g_u, loss_u, n_u = unfused
    assert n_f == n_u == n_want, (n_f, n_u, n_want)
    print("%s: loss fused %.7f unfused %.7f" % (tag, loss_f, loss_u))
    assert abs(loss_f - loss_u) < TOL * abs(loss_u)
    assert any(float(v.abs().max()) > 0.0 for v in g_u.values())
    for k, v in g_u.items():
        e = relerr(g_f[k], v)
        print("%s: %s relerr %.2e" % (tag, k, e))
        assert e < TOL, (k, e)


def _step(dev, lengths, p, path, neg, data):
    B = len(lengths)
    eng = _engine(B, dev, p_drop=p)
    if path == "fwd_bwd":
        eng.fwd_bwd(eng.make_plan(data[0], data[1], data[2], neg_item=neg, sample_neg=False))
    else:
        perm = torch.arange(B, dtype=torch.int64, device=dev)
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        plan = eng.make_plan(data[0], data[1], data[2], rows=torch.zeros(B, dtype=torch.int64, device=dev), neg_item=neg, sample_neg=False,
                             perm_sel=(perm, B, 0, counter))
        eng.train_steps(plan, 1)
    return _grads(eng)


def _inputs(dev, lengths):
    data = tuple(t.to(dev) for t in _rows(lengths, seed=8))
    neg = torch.randint(1, N_ITEMS, (len(lengths), 50), generator=torch.Generator().manual_seed(9)).to(dev)
    return data, neg


@pytest.mark.parametrize("path", ["fwd_bwd", "train_steps"])
@pytest.mark.parametrize("shape", sorted(LENGTHS))
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_fused_step_equals_unfused_step(monkeypatch, p, shape, path):
    dev = torch.device("cuda", 0)
    lengths = LENGTHS[shape]
    data, neg = _inputs(dev, lengths)
    fused = _step(dev, lengths, p, path, neg, data)
    monkeypatch.setenv("DR4SR_NO_FUSE", "1")
    unfused = _step(dev, lengths, p, path, neg, data)
    _assert_close(fused, unfused, sum(lengths), "p %.1f %s %s" % (p, shape, path))


def test_fused_step_equals_unfused_step_deterministic_mode(monkeypatch):
    monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    dev = torch.device("cuda", 0)
    lengths = LENGTHS["B7"]
    data, neg = _inputs(dev, lengths)
    fused = _step(dev, lengths, 0.5, "fwd_bwd", neg, data)
    monkeypatch.setenv("DR4SR_NO_FUSE", "1")
    unfused = _step(dev, lengths, 0.5, "fwd_bwd", neg, data)
    _assert_close(fused, unfused, sum(lengths), "deterministic B7")


def test_weighted_fused_step_equals_unfused_layers(monkeypatch):
    """the MetaModel-weighted launch: k_post_mid<.., META, .., KU> behind k_post_fwd<.., KB>, against the same entry point under DR4SR_NO_FUSE —
    unfused layer kernels and the k_post_mid form that regenerates the decisions inside its passes"""
    from dr4sr_amd import _lib
    dev = torch.device("cuda", 0)
    lengths = LENGTHS["B7"]
    B = len(lengths)
    data, neg = _inputs(dev, lengths)
    lib = _lib.load()
    phi = (0.1 * torch.randn(int(lib.dr4sr_meta_param_count(D)), generator=torch.Generator().manual_seed(1))).to(dev)
    uid = torch.arange(1, B + 1, dtype=torch.int64, device=dev)

    def step():
        eng = _engine(B, dev)
        plan = eng.make_plan(data[0], data[1], data[2], neg_item=neg, sample_neg=False)
        mw = _lib.MetaWeighting()
        mw.phi, mw.user_id, mw.tau = phi.data_ptr(), uid.data_ptr(), 1.0
        _lib.check(lib.dr4sr_sasrec_fwd_bwd_weighted(C.byref(plan), C.byref(mw), _lib.cur_stream()), "dr4sr_sasrec_fwd_bwd_weighted")
        return _grads(eng)

    fused = step()
    monkeypatch.setenv("DR4SR_NO_FUSE", "1")
    _assert_close(fused, step(), sum(lengths), "weighted B7")


# ------------------------------------------------------------------------------------------------ pad tail of the scorer
def _engine_L(B, L, dev):
    from test_gpu_parity import _random_params
    from dr4sr_amd.engine import SasrecEngine
    eng = SasrecEngine(N_ITEMS, L, D, H, F, NL, 1e-12, 0.5, B, dev, seed=77)
    eng.load_named(_random_params(N_ITEMS, D, F, NL, L=L, seed=12))
    return eng


def _rows_L(lengths, L, seed, fill_targets=False):
    g = torch.Generator().manual_seed(seed)
    n = len(lengths)
    idx, tgt = torch.zeros(n, L, dtype=torch.long), torch.zeros(n, L, dtype=torch.long)
    for i, k in enumerate(lengths):
        idx[i, :k] = torch.randint(1, N_ITEMS, (k,), generator=g)
        tgt[i, :k] = torch.randint(1, N_ITEMS, (k,), generator=g)
    if fill_targets:                                       # valid targets behind seqlen too
        tgt = torch.randint(1, N_ITEMS, (n, L), generator=g)
    return idx, tgt, torch.tensor(lengths, dtype=torch.long)


@pytest.mark.parametrize("B,L", [(4, 49), (3, 50), (2, 64)])
def test_sampled_negatives_equal_mirror_at_every_position(B, L):
    """(4, 49): b L mod 4 takes all four values, so a sequence's elements start at every offset inside a Philox call; L = 64: 63 pad positions
    behind a one-token sequence, four trips of the 16 lanes.  Every rotation of the lengths over the rows; the buffer starts at -1."""
    from dr4sr_amd import _lib
    from oracle import cl4srec_oracle as CO
    dev = torch.device("cuda", 0)
    ls = [1, 2, 3, L - 3, L - 1, L]
    eng = _engine_L(B, L, dev)
    neg = torch.empty(B, L, dtype=torch.int64, device=dev)
    for r in range(len(ls)):
        lengths = [ls[(b + r) % len(ls)] for b in range(B)]
        data = tuple(t.to(dev) for t in _rows_L(lengths, L, seed=20 + r))
        neg.fill_(-1)
        eng.fwd_bwd(eng.make_plan(data[0], data[1], data[2], neg_item=neg, sample_neg=True))
        torch.cuda.synchronize()
        step = int(eng.state[_lib.STATE_RNGSTEP])
        want = torch.from_numpy(CO.neg_sample_mirror(B * L, N_ITEMS, eng.seed, step)).reshape(B, L)
        got = neg.cpu()
        bad = (got != want).nonzero().tolist()
        assert not bad, (lengths, step, bad[:8])
        assert eng.loss_and_count()[1] == sum(lengths)


def test_valid_targets_behind_seqlen_count_as_in_the_unfused_step(monkeypatch):
    """a valid target at a pad position adds 2 ln 2 to the loss and 1 to n_valid (zero query row): n_valid exact, loss within 2e-5"""
    dev = torch.device("cuda", 0)
    lengths, L = LENGTHS["B7"], 50
    B = len(lengths)
    data = tuple(t.to(dev) for t in _rows_L(lengths, L, seed=31, fill_targets=True))

    def step():
        eng = _engine(B, dev)
        neg = torch.full((B, L), -1, dtype=torch.int64, device=dev)
        eng.fwd_bwd(eng.make_plan(data[0], data[1], data[2], neg_item=neg, sample_neg=True))
        torch.cuda.synchronize()
        loss, n = eng.loss_and_count()
        return loss, n, neg.cpu()

    loss_f, n_f, neg_f = step()
    monkeypatch.setenv("DR4SR_NO_FUSE", "1")
    loss_u, n_u, neg_u = step()
    print("loss fused %.7f unfused %.7f n %d %d" % (loss_f, loss_u, n_f, n_u))
    assert n_f == n_u == B * L
    assert abs(loss_f - loss_u) < TOL * abs(loss_u)
    assert torch.equal(neg_f, neg_u)
