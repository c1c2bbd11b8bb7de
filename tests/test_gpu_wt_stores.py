"""Write-through stores (csrc/common.h st4_wt: raw-buffer stores with the sc1 bit through a resource that covers exactly the destination
array) in k_adam's sweep; the row passes of the 16-row token-tile kernels were measured with them and keep their plain stores (NOTEBOOK
"Write-through stores"), groups 1 and 2 stay as their regression cases.  The arithmetic is the parent's; what can go wrong is addressing — a
wrong base, offset or record count makes a store vanish or land in a neighbouring array, and the rows >= T guard may fail — so the cases sit
at the edges of the tiles and of the arrays:

  1. the fused step (fwd_bwd, then train_steps(plan, 3)) against the DR4SR_NO_FUSE step at T = 1, 15, 16, 17, 33, 49 tokens, d = 64 and 128,
     p = 0 and 0.5: loss, every parameter gradient, and parameters / moments after three steps, relerr < 2e-5 (the bound of
     tests/test_gpu_step_boundary.py and tests/test_gpu_keep_upfront.py for this pair of forms).  The engines of this group run Adam with
     eps = 1e-2 at lr = 1e-3.  With the default eps = 1e-8 the update lr m / (sqrt(v) + eps) is lr sign(g) in the first steps, so an element
     whose gradient is at the level of the atomics' summation-order noise moves by +lr in one form and -lr in the other: the PARENT library
     measured relerr 9.6e-4 on the stepped parameters (9.7e-4 this tree), 1.05e-4 on the third step's gradients, 2.0e-5 on adam_m, while
     the first step's gradients agree to 1.2e-6.  With eps = 1e-2 the update is Lipschitz in the gradient with constant lr / eps = 0.1 and
     the bound applies to parameters and moments as it does to gradients; an element with |g| >= eps still moves by >= lr / 2 per step,
     19 times the bound relative to the largest parameter, so a store that vanishes is seen.
  2. sentinels: the row arrays dr4sr_sasrec_workspace_offsets names, and the padding behind them, hold 0xFF bytes (a NaN as fp32) before one
     fwd_bwd at T = 17 in a B = 4, L = 12 plan (48 rows): rows < T of the float arrays the first layer's k_post_fwd stores are finite, rows >= T
     and the 256 bytes behind the last valid row of EVERY array still hold the pattern bit for bit.  (The last layer's k_post_mid<16, 64, ...>
     stores none of them — tests/test_gpu_step_boundary.py group 3 — so there the whole array keeps the pattern.)
  3. k_adam through the flat entry point (dr4sr_adam_flat), two steps on random P, G, M, V, against a float64 restatement of the formula in
     the kernel's header comment; n = 4 (one float4: no second group of the paired loop), 4 (256 * 256 + 3) (a partial second group) and an
     engine's own n above 2 * 4 * 256 * 256 (a full second group and a third pass).  Parent library on these inputs: worst relerr
     1.657e-7 (adam_m at the engine's n; 4.8e-8 at n = 4, 1.06e-7 at n = 262 156); the bound is twice that, 3.314e-7.  And with a prep attached (adam_step_prepare_next: the launch also zeroes the gradient words
     it has consumed — the LAST optimizer launch of train_steps carries no prep and leaves the gradient) every word of the gradient buffer,
     tail included, is zero afterwards.
  4. DR4SR_DETERMINISTIC=1, T = 33, d = 64: two runs give bitwise equal gradients, parameters and moments."""
import numpy as np
import pytest
import torch

from test_gpu_fwd_state_reuse import H, N_ITEMS, NL, relerr

pytestmark = pytest.mark.gpu

TOL = 2e-5
F = 128
PARENT_WORST_ADAM = 1.657e-7    # parent library, group 3 (docstring)
ADAM_EPS_FUSED = 1e-2           # group 1 (docstring)
ADAM_TOL = 2.0 * PARENT_WORST_ADAM
LENGTHS = {1: [1], 15: [15], 16: [16], 17: [9, 8], 33: [17, 16], 49: [2, 47]}


def _engine(D, B, dev, L=50, p_drop=0.5, n_items=N_ITEMS, adam_eps=1e-8):
    from test_gpu_parity import _random_params
    from dr4sr_amd.engine import SasrecEngine
    eng = SasrecEngine(n_items, L, D, H, F, NL, 1e-12, p_drop, B, dev, seed=77, lr=1e-3, adam_eps=adam_eps)
    eng.load_named(_random_params(n_items, D, F, NL, L=L, seed=12))
    return eng


def _inputs(dev, L, lengths):
    from test_gpu_step_boundary import _rows
    data = tuple(t.to(dev) for t in _rows(lengths, L, N_ITEMS, seed=8))
    neg = torch.randint(1, N_ITEMS, (len(lengths), L), generator=torch.Generator().manual_seed(9)).to(dev)
    return data, neg


def _run(dev, D, p, lengths, L=50, adam_eps=ADAM_EPS_FUSED):
    """fwd_bwd, then three train_steps on the same rows, of a fresh engine under the switches in force"""
    from test_gpu_step_boundary import _perm_plan
    B = len(lengths)
    data, neg = _inputs(dev, L, lengths)
    eng = _engine(D, B, dev, L=L, p_drop=p, adam_eps=adam_eps)
    eng.fwd_bwd(eng.make_plan(data[0], data[1], data[2], neg_item=neg, sample_neg=False))
    torch.cuda.synchronize()
    loss, n = eng.loss_and_count()
    out = {"loss": torch.tensor([loss]), "n": n}
    out.update({"grad " + k: v.clone() for k, v in eng.normalized_grads().items()})
    eng.train_steps(_perm_plan(eng, data, neg, B), 3)
    torch.cuda.synchronize()
    assert int(eng.state[0]) == 3
    out.update({"params": eng.params.clone(), "adam_m": eng.adam_m.clone(), "adam_v": eng.adam_v.clone()})
    out.update({"grad3 " + k: v.clone() for k, v in eng.normalized_grads().items()})
    return out


# ------------------------------------------------------------------------------------------------ 1. fused step against DR4SR_NO_FUSE
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", sorted(LENGTHS))
def test_fused_step_equals_unfused_step(monkeypatch, T, D, p):
    dev = torch.device("cuda", 0)
    lengths = LENGTHS[T]
    assert sum(lengths) == T
    fused = _run(dev, D, p, lengths)
    monkeypatch.setenv("DR4SR_NO_FUSE", "1")
    unfused = _run(dev, D, p, lengths)
    assert fused["n"] == unfused["n"] == T
    worst = 0.0
    for k, want in unfused.items():
        if k == "n":
            continue
        assert bool(torch.isfinite(fused[k]).all()), k
        e = relerr(fused[k], want)
        worst = max(worst, e)
        print("T %d d %d p %.1f: %s relerr %.2e" % (T, D, p, k, e))
    print("T %d d %d p %.1f: worst relerr %.2e" % (T, D, p, worst))
    assert float(unfused["params"].abs().max()) > 0.0 and float(unfused["adam_v"].abs().max()) > 0.0
    for k, want in unfused.items():
        if k != "n":
            assert relerr(fused[k], want) < TOL, (k, relerr(fused[k], want))


# ------------------------------------------------------------------------------------------------ 2. sentinels
PATTERN = 0xFF
_ROW_BYTES = {"attn_keep": H * 2 * 4, "u1": 64 * 4, "st1": 2 * 4, "a": F * 4, "u2": 64 * 4, "st2": 2 * 4, "row_keep": 16 * 2}
_FLOAT = ("u1", "st1", "a", "u2", "st2")


def test_rows_beyond_T_and_the_bytes_behind_each_array_are_untouched():
    from test_gpu_step_boundary import _offsets
    dev = torch.device("cuda", 0)
    L, lengths = 12, [1, 2, 2, 12]
    T, Tmax = sum(lengths), len(lengths) * L
    assert T == 17
    data, neg = _inputs(dev, L, lengths)
    eng = _engine(64, len(lengths), dev, L=L)
    plan = eng.make_plan(data[0], data[1], data[2], neg_item=neg, sample_neg=False)
    layers, rec = _offsets(eng, plan)
    spans = []
    for l, w in enumerate(layers):
        for name, (o, n) in w.items():
            assert n == Tmax * _ROW_BYTES[name], (name, n)
            end = min((o + n + 255) // 256 * 256, rec)       # the array and the alignment padding behind it
            spans.append((l, name, o, end))
            eng.workspace[o:end].fill_(PATTERN)
    eng.fwd_bwd(plan)
    torch.cuda.synchronize()
    assert eng.loss_and_count()[1] == T
    for l, name, o, end in spans:
        rb = _ROW_BYTES[name]
        valid_end = o + T * rb
        tail = eng.workspace[valid_end:end]
        assert bool((tail == PATTERN).all()), \
            "layer %d %s: %d bytes behind row T - 1 were written" % (l, name, int((tail != PATTERN).sum()))
        head = eng.workspace[o:valid_end]
        if l == NL - 1:                                      # the fused last layer stores none of them
            assert bool((head == PATTERN).all()), "layer %d %s" % (l, name)
        elif name in _FLOAT:
            assert bool(torch.isfinite(head.view(torch.float32)).all()), "layer %d %s: rows < T not all stored" % (l, name)


# ------------------------------------------------------------------------------------------------ 3. k_adam
def _adam_ref(P, G, M, V, n_valid, lr, b1, b2, eps, wd, steps):
    lr, b1, b2, eps, wd = (float(np.float32(x)) for x in (lr, b1, b2, eps, wd))
    p, g0, m, v = (x.double().cpu() for x in (P, G, M, V))
    for t in range(1, steps + 1):
        g = g0 / n_valid + wd * p
        m = m + (g - m) * (1.0 - b1)
        v = b2 * v + (1.0 - b2) * g * g
        p = p - lr / (1.0 - b1 ** t) * m / (v.sqrt() / (1.0 - b2 ** t) ** 0.5 + eps)
    return p, m, v


def _engine_n(dev):
    return _engine(64, 4, dev, n_items=12000).n_params          # about the headline model's 833 k parameters


@pytest.mark.parametrize("which", ["one_float4", "partial_second_group", "engine"])
def test_adam_flat_equals_the_float64_formula(which):
    from dr4sr_amd import _lib, ops
    dev = torch.device("cuda", 0)
    n = {"one_float4": 4, "partial_second_group": 4 * (256 * 256 + 3), "engine": _engine_n(dev)}[which]
    assert n % 4 == 0 and (which != "engine" or n > 2 * 4 * 256 * 256)
    g = torch.Generator().manual_seed(21)
    P = (0.1 * torch.randn(n, generator=g)).to(dev)
    G = torch.zeros(n + _lib.GRAD_TAIL)
    G[:n] = torch.randn(n, generator=g)
    n_valid = 7.0
    G[n] = n_valid
    G = G.to(dev)
    M = (0.01 * torch.randn(n, generator=g)).to(dev)
    V = (1e-4 + 1e-2 * torch.rand(n, generator=g)).to(dev)
    lr, b1, b2, eps, wd = 1e-3, 0.9, 0.999, 1e-8, 0.01
    want = _adam_ref(P, G[:n], M, V, n_valid, lr, b1, b2, eps, wd, 2)
    state = torch.zeros(_lib.STATE_WORDS, dtype=torch.int32, device=dev)
    G0 = G.clone()
    for _ in range(2):
        ops.fused_adam_(P, G, M, V, state, lr, b1, b2, eps, wd)
    torch.cuda.synchronize()
    assert int(state[0]) == 2
    assert torch.equal(G, G0)                                # no prep attached: the gradient stays
    worst = 0.0
    for name, got, w in zip(("params", "adam_m", "adam_v"), (P, M, V), want):
        e = relerr(got, w)
        worst = max(worst, e)
        print("adam n %d: %s relerr %.3e" % (n, name, e))
    print("adam n %d: worst relerr %.3e (bound %.3e)" % (n, worst, ADAM_TOL))
    assert worst < ADAM_TOL, (worst, ADAM_TOL)


def test_adam_with_a_prep_attached_leaves_the_gradient_buffer_zero():
    from test_gpu_step_boundary import _perm_plan
    dev = torch.device("cuda", 0)
    lengths = LENGTHS[33]
    data, neg = _inputs(dev, 50, lengths)
    eng = _engine(64, len(lengths), dev, n_items=12000)      # n > 4 * 256 * 256: both groups of the paired loop, and a third pass
    assert eng.n_params > 2 * 4 * 256 * 256
    plan = _perm_plan(eng, data, neg, len(lengths))
    p0 = eng.params.clone()
    eng.fwd_bwd(plan)
    torch.cuda.synchronize()
    assert int((eng.grads != 0).sum()) > 1000 and float(eng.grads[eng.n_params]) == 33.0
    eng.grads[:eng.n_params].add_(1.0).clamp_(min=0.5)       # no word is zero by itself (untouched table rows have zero gradients)
    eng.adam_step_prepare_next(plan)
    torch.cuda.synchronize()
    assert int(eng.state[0]) == 1 and not torch.equal(eng.params, p0)
    nz = torch.nonzero(eng.grads.view(torch.int32))
    assert nz.numel() == 0, "%d gradient words not zeroed, first at %d of %d" % (nz.numel(), int(nz[0]), eng.grads.numel())


# ------------------------------------------------------------------------------------------------ 4. deterministic mode
def test_deterministic_mode_is_bitwise_reproducible(monkeypatch):
    monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    dev = torch.device("cuda", 0)
    a = _run(dev, 64, 0.5, LENGTHS[33], adam_eps=1e-8)
    b = _run(dev, 64, 0.5, LENGTHS[33], adam_eps=1e-8)
    assert float(a["params"].abs().max()) > 0.0
    for k, v in a.items():
        if k != "n":
            assert np.array_equal(v.cpu().numpy(), b[k].cpu().numpy()), k
