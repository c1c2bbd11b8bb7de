"""The step boundary of the latency-regime step (d = 64, 16-row tiles), three pieces of state that cross it:

  1. Adam's bias corrections, cached one step ahead (csrc/prep_body.h adam_bc_write, csrc/step.hip k_adam<ADAM, BC>): the prep of step t — the
     prep workgroup of the previous optimizer launch, or the k_prep at the head of a dr4sr_sasrec_train_steps graph — leaves
     {t, lr, b1, b2, step_size, inv_sqrt_bc2} in slot t & 1 of a record (the last 256 bytes of the plan's workspace carve-up), and the
     optimizer launches that carry a prep take the pair when the key is theirs bit for bit.  The eager dr4sr_adam_step evaluates the two
     pow() inline as before: in deterministic mode (bit-equal gradients) parameters and moments of the two forms must be bitwise equal.
  2. the attention keep decisions k_post_fwd<.., KB> stores per (token, head) for k_post_bwd<.., KB> (csrc/attn_tile.h keep_store /
     keep_load), against the DR4SR_NO_FUSE step, which regenerates every decision with Philox: relerr < 2e-5, the bound
     tests/test_gpu_keep_upfront.py uses for the same pair of forms.  (Builds with the heads swapped in the store, or lo / hi swapped in the
     load, fail the cases of this group; see NOTEBOOK.)
  3. u1 / st1 / a / u2 / st2 of the LAST layer, which the forward half of k_post_mid<16, 64, ...> no longer stores: prefilled with NaN, the
     step's result must not change."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from test_gpu_fwd_state_reuse import D, F, H, N_ITEMS, NL, relerr

pytestmark = pytest.mark.gpu

TOL = 2e-5
BC_SLOT_WORDS = 8                                           # csrc/prep_body.h DR4SR_BC_SLOT_WORDS


# ------------------------------------------------------------------------------------------------ helpers
_OFF_NAMES = ("attn_keep", "u1", "st1", "a", "u2", "st2", "row_keep")     # include/dr4sr_hip.h DR4SR_WS_OFF_*; [7] = the record


def _offsets(eng, plan):
    """(per layer {name: (byte offset, bytes)}, byte offset of the bias-correction record) of THIS plan's workspace carve-up, asked from the
    library (dr4sr_sasrec_workspace_offsets) under the switches in force: deterministic mode carves more in front of the layers"""
    from dr4sr_amd import _lib
    lib = _lib.load()
    T = plan.B * eng.L
    size = {"attn_keep": T * H * 2 * 4, "u1": T * D * 4, "st1": T * 2 * 4, "a": T * F * 4, "u2": T * D * 4, "st2": T * 2 * 4, "row_keep": T * 16 * 2}
    end = int(lib.dr4sr_sasrec_workspace_bytes(C.byref(plan)))
    layers, rec = [], None
    for l in range(NL):
        out = (C.c_int64 * 8)()
        _lib.check(lib.dr4sr_sasrec_workspace_offsets(C.byref(plan), l, out), "dr4sr_sasrec_workspace_offsets")
        w = {n: (int(out[i]), size[n]) for i, n in enumerate(_OFF_NAMES)}
        assert all(0 <= o and o % 256 == 0 and o + n <= end for o, n in w.values()), w
        layers.append(w)
        rec = int(out[7])
    assert rec == end - 256                              # the record is the last thing carved
    spans = sorted(v for w in layers for v in w.values())
    assert all(a[0] + a[1] <= b[0] for a, b in zip(spans, spans[1:])), "buffers overlap"
    return layers, rec


def _engine(B, dev, n_items=N_ITEMS, L=50, p_drop=0.5, lr=1e-3):
    from test_gpu_parity import _random_params
    from dr4sr_amd.engine import SasrecEngine
    eng = SasrecEngine(n_items, L, D, H, F, NL, 1e-12, p_drop, B, dev, seed=77, lr=lr)
    eng.load_named(_random_params(n_items, D, F, NL, L=L, seed=12))
    return eng


def _rows(lengths, L, n_items, seed):
    g = torch.Generator().manual_seed(seed)
    n = len(lengths)
    idx, tgt = torch.zeros(n, L, dtype=torch.long), torch.zeros(n, L, dtype=torch.long)
    for i, k in enumerate(lengths):
        idx[i, :k] = torch.randint(1, n_items, (k,), generator=g)
        tgt[i, :k] = torch.randint(1, n_items, (k,), generator=g)
    return idx, tgt, torch.tensor(lengths, dtype=torch.long)


def _perm_plan(eng, data, neg, B):
    """the same B rows in every step (perm = 0..B-1), selected on the device as dr4sr_sasrec_train_steps needs it"""
    dev = eng.device
    perm = torch.arange(B, dtype=torch.int64, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    return eng.make_plan(data[0], data[1], data[2], rows=torch.zeros(B, dtype=torch.int64, device=dev), neg_item=neg, sample_neg=False,
                         perm_sel=(perm, B, 0, counter))


# ------------------------------------------------------------------------------------------------ 1. bias-correction cache
BN, BL, BB = 50, 8, 4
B_LENGTHS = [8, 3, 1, 5]


def _bc_setup(dev, lr=1e-3):
    eng = _engine(BB, dev, n_items=BN, L=BL, lr=lr)
    data = tuple(t.to(dev) for t in _rows(B_LENGTHS, BL, BN, seed=3))
    neg = torch.randint(1, BN, (BB, BL), generator=torch.Generator().manual_seed(4)).to(dev)
    return eng, data, neg


def _opt_state(eng):
    torch.cuda.synchronize()
    return eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone(), int(eng.state[0])


def _assert_opt_equal(got, want):
    assert got[3] == want[3], (got[3], want[3])
    for name, a, b in zip(("params", "adam_m", "adam_v"), got[:3], want[:3]):
        assert bool(torch.isfinite(b).all()) and float(b.abs().max()) > 0.0, name
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()), "%s: max |diff| %.3e" % (name, float((a - b).abs().max()))


def _with_lr(plan, lr):
    q = type(plan).from_buffer_copy(plan)
    q.lr = lr
    return q


def _eager(eng, plan, n):
    for _ in range(n):
        eng.fwd_bwd(plan)
        eng.adam_step(plan)                                # no prep rides on it: bias corrections inline


@pytest.mark.parametrize("split", [(5,), (3, 2)])
def test_train_steps_equal_eager_steps(monkeypatch, split):
    """five optimizer steps: every launch but the last of a graph reads the record (written by k_prep at the head of each graph, then by the
    prep workgroup of the launch before).  (3, 2): the k_prep of the second graph keys t = 4."""
    monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    dev = torch.device("cuda", 0)
    e1, data, neg = _bc_setup(dev)
    p0 = e1.params.clone()
    plan1 = _perm_plan(e1, data, neg, BB)
    for n in split:
        e1.train_steps(plan1, n)
    got = _opt_state(e1)
    assert not torch.equal(got[0], p0)
    e2, _, _ = _bc_setup(dev)
    _eager(e2, _perm_plan(e2, data, neg, BB), 5)
    _assert_opt_equal(got, _opt_state(e2))
    assert got[3] == 5


@pytest.mark.parametrize("path", ["train_steps", "prepared"])
def test_changed_learning_rate_rejects_the_stale_record(monkeypatch, path):
    """prepared: the optimizer launch of step 2 wrote the record of step 3 under the old learning rate; step 3's launch carries the new one and
    must evaluate the corrections itself.  train_steps: the second call's k_prep rewrites the record under the new rate."""
    monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    dev = torch.device("cuda", 0)
    e1, data, neg = _bc_setup(dev, lr=1e-3)
    plan = _perm_plan(e1, data, neg, BB)
    if path == "train_steps":
        e1.train_steps(plan, 2)
        e1.train_steps(_with_lr(plan, 3e-3), 1)
    else:
        e1.fwd_bwd(plan)
        e1.adam_step_prepare_next(plan)
        e1.fwd_bwd_prepared(plan)
        e1.adam_step_prepare_next(plan)                    # record of t = 3 keyed by lr = 1e-3
        plan3 = _with_lr(plan, 3e-3)                       # (the same rows / counter tensors: step 3 is already prepared)
        e1.fwd_bwd_prepared(plan3)
        e1.adam_step_prepare_next(plan3)                   # t = 3, lr = 3e-3
    got = _opt_state(e1)
    e2, _, _ = _bc_setup(dev, lr=1e-3)
    plan2 = _perm_plan(e2, data, neg, BB)
    _eager(e2, plan2, 2)
    _eager(e2, _with_lr(plan2, 3e-3), 1)
    _assert_opt_equal(got, _opt_state(e2))
    assert got[3] == 3


def test_poisoned_step_is_skipped_and_the_next_steps_equal_eager(monkeypatch):
    """step 2 of 4 carries a poison word: parameters, moments and state[STEP] stay, its prep workgroup keys the record with t = 2 AGAIN, and
    steps 3 and 4 (optimizer steps 2 and 3) equal an eager continuation"""
    monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    dev = torch.device("cuda", 0)

    def run(eng, plan, fused):
        for i in range(4):
            if fused and i > 0:
                eng.fwd_bwd_prepared(plan)
            else:
                eng.fwd_bwd(plan)
            if i == 1:
                before = _opt_state(eng)
                eng.grads[eng.n_params + 2] = 1.0
            if fused:
                eng.adam_step_prepare_next(plan)
            else:
                eng.adam_step(plan)
            if i == 1:
                after = _opt_state(eng)
                assert after[3] == before[3] == 1
                for a, b in zip(after[:3], before[:3]):
                    assert torch.equal(a, b)
        return _opt_state(eng)

    e1, data, neg = _bc_setup(dev)
    got = run(e1, _perm_plan(e1, data, neg, BB), True)
    e2, _, _ = _bc_setup(dev)
    want = run(e2, _perm_plan(e2, data, neg, BB), False)
    _assert_opt_equal(got, want)
    assert got[3] == 3


def _want_pair(lr, b1, b2, t):
    lr, b1, b2 = float(np.float32(lr)), float(np.float32(b1)), float(np.float32(b2))
    return np.float32(lr / (1.0 - b1 ** t)), np.float32(1.0 / math.sqrt(1.0 - b2 ** t))


@pytest.mark.parametrize("step0", [0, 1, 998])
def test_cached_pair_equals_float64_expressions(step0):
    """two steps from state[STEP] = step0: k_prep writes the record of t = step0 + 1, the prep workgroup of the first optimizer launch the
    record of t = step0 + 2 (slot t & 1 each) — t = 1, 2, 3 and 999, 1000 over the three cases"""
    dev = torch.device("cuda", 0)
    eng, data, neg = _bc_setup(dev)
    plan = _perm_plan(eng, data, neg, BB)
    _, rec_off = _offsets(eng, plan)
    eng.workspace[rec_off:rec_off + 256].zero_()
    eng.state[0] = step0
    eng.train_steps(plan, 2)
    torch.cuda.synchronize()
    assert int(eng.state[0]) == step0 + 2
    rec = eng.workspace[rec_off:rec_off + 4 * 2 * BC_SLOT_WORDS].cpu().numpy()
    for t in (step0 + 1, step0 + 2):
        slot = rec[4 * BC_SLOT_WORDS * (t & 1):][:24]
        key_t = int(slot[:4].view(np.int32)[0])
        lr, b1, b2, ss, isq = slot[4:24].view(np.float32).tolist()
        assert key_t == t, (key_t, t)
        assert (np.float32(lr), np.float32(b1), np.float32(b2)) == (np.float32(eng.lr), np.float32(eng.betas[0]), np.float32(eng.betas[1]))
        want = _want_pair(eng.lr, eng.betas[0], eng.betas[1], t)
        print("t %d: step_size %.9g (want %.9g) inv_sqrt_bc2 %.9g (want %.9g)" % (t, ss, want[0], isq, want[1]))
        assert np.float32(ss) == want[0] and np.float32(isq) == want[1]


@pytest.mark.parametrize("inline", [False, True])
def test_two_phase_prep_writes_the_record(monkeypatch, inline):
    """more than 1 024 rows: the next step's prep is spread over the optimizer launch and finished by k_prep_phase2_bc (or, DR4SR_PREP2_INLINE,
    by the last workgroup of the launch, which passes its own t) — the record of t = 2 comes from there, that of t = 1 from k_prep; three
    such steps equal three eager steps bitwise in deterministic mode"""
    if inline:
        monkeypatch.setenv("DR4SR_PREP2_INLINE", "1")
    dev = torch.device("cuda", 0)
    B = 1100
    lengths = [1 + (i * 7) % BL for i in range(B)]
    data = tuple(t.to(dev) for t in _rows(lengths, BL, BN, seed=3))
    neg = torch.randint(1, BN, (B, BL), generator=torch.Generator().manual_seed(4)).to(dev)
    eng = _engine(B, dev, n_items=BN, L=BL)
    plan = _perm_plan(eng, data, neg, B)
    _, rec_off = _offsets(eng, plan)
    eng.workspace[rec_off:rec_off + 256].zero_()
    eng.train_steps(plan, 2)
    torch.cuda.synchronize()
    assert int(eng.state[0]) == 2
    rec = eng.workspace[rec_off:rec_off + 4 * 2 * BC_SLOT_WORDS].cpu().numpy()
    for t in (1, 2):
        slot = rec[4 * BC_SLOT_WORDS * (t & 1):][:24]
        assert int(slot[:4].view(np.int32)[0]) == t
        ss, isq = slot[16:24].view(np.float32).tolist()
        want = _want_pair(eng.lr, eng.betas[0], eng.betas[1], t)
        assert np.float32(ss) == want[0] and np.float32(isq) == want[1], (t, ss, isq, want)
    monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    e1 = _engine(B, dev, n_items=BN, L=BL)
    e1.train_steps(_perm_plan(e1, data, neg, B), 3)
    e2 = _engine(B, dev, n_items=BN, L=BL)
    _eager(e2, _perm_plan(e2, data, neg, B), 3)
    _assert_opt_equal(_opt_state(e1), _opt_state(e2))


# ------------------------------------------------------------------------------------------------ 2. saved attention keep bits
LENGTHS = {"1": (50, [1]), "16": (50, [16]), "17": (50, [17]), "15_1_16_2": (50, [15, 1, 16, 2]), "50": (50, [50]), "3_50_1": (50, [3, 50, 1]),
           "64_L64": (64, [64]), "B7": (50, [4, 50, 1, 16, 17, 9, 33])}          # B7: 130 tokens, no multiple of 16


def _grads(eng):
    torch.cuda.synchronize()
    loss, n = eng.loss_and_count()
    return {k: v.clone() for k, v in eng.normalized_grads().items()}, loss, n


def _assert_close(fused, unfused, n_want, tag):
    g_f, loss_f, n_f = fused
    g_u, loss_u, n_u = unfused
    assert n_f == n_u == n_want, (n_f, n_u, n_want)
    print("%s: loss fused %.7f unfused %.7f" % (tag, loss_f, loss_u))
    assert math.isfinite(loss_f) and abs(loss_f - loss_u) < TOL * abs(loss_u)
    assert any(float(v.abs().max()) > 0.0 for v in g_u.values())
    for k, v in g_u.items():
        assert bool(torch.isfinite(g_f[k]).all()), k
        e = relerr(g_f[k], v)
        print("%s: %s relerr %.2e" % (tag, k, e))
        assert e < TOL, (k, e)


def _inputs(dev, L, lengths):
    data = tuple(t.to(dev) for t in _rows(lengths, L, N_ITEMS, seed=8))
    neg = torch.randint(1, N_ITEMS, (len(lengths), L), generator=torch.Generator().manual_seed(9)).to(dev)
    return data, neg


def _step(dev, L, lengths, p, path, neg, data, prefill=None):
    B = len(lengths)
    eng = _engine(B, dev, L=L, p_drop=p)
    plan = _perm_plan(eng, data, neg, B) if path == "train_steps" else eng.make_plan(data[0], data[1], data[2], neg_item=neg, sample_neg=False)
    if prefill:
        prefill(eng, plan)
    if path == "train_steps":
        eng.train_steps(plan, 1)
    else:
        eng.fwd_bwd(plan)
    return _grads(eng), eng, plan


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("path", ["fwd_bwd", "train_steps"])
@pytest.mark.parametrize("shape", sorted(LENGTHS))
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_fused_step_equals_unfused_step(monkeypatch, p, shape, path, det):
    if det:
        monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    dev = torch.device("cuda", 0)
    L, lengths = LENGTHS[shape]
    data, neg = _inputs(dev, L, lengths)
    fused = _step(dev, L, lengths, p, path, neg, data)[0]
    monkeypatch.setenv("DR4SR_NO_FUSE", "1")
    unfused = _step(dev, L, lengths, p, path, neg, data)[0]
    _assert_close(fused, unfused, sum(lengths), "p %.1f %s %s det %d" % (p, shape, path, det))


def _xy():
    g = torch.Generator().manual_seed(5)
    return torch.randint(40, 51, (8,), generator=g).tolist(), [3, 17]


@pytest.mark.parametrize("path", ["train_steps", "prepared", "weighted"])
def test_short_step_behind_a_larger_batch_reads_no_stale_keep_words(monkeypatch, path):
    """a step of 8 long rows, then a step of 2 short rows in the same workspace (lr = 0: the parameters stay), against the DR4SR_NO_FUSE step
    of a fresh engine at the same RNG step"""
    from dr4sr_amd import _lib
    dev = torch.device("cuda", 0)
    lx, ly = _xy()
    bx, negx = _inputs(dev, 50, lx)
    by, negy = _inputs(dev, 50, ly)
    lib = _lib.load()
    phi = (0.1 * torch.randn(int(lib.dr4sr_meta_param_count(D)), generator=torch.Generator().manual_seed(1))).to(dev)
    uid = torch.arange(1, 9, dtype=torch.int64, device=dev)

    def weighted(eng, b, neg):
        plan = eng.make_plan(b[0], b[1], b[2], neg_item=neg, sample_neg=False)
        mw = _lib.MetaWeighting()
        mw.phi, mw.user_id, mw.tau = phi.data_ptr(), uid.data_ptr(), 1.0
        _lib.check(lib.dr4sr_sasrec_fwd_bwd_weighted(C.byref(plan), C.byref(mw), _lib.cur_stream()), "dr4sr_sasrec_fwd_bwd_weighted")

    e1 = _engine(8, dev, lr=0.0)
    if path == "train_steps":
        e1.train_steps(_perm_plan(e1, bx, negx, 8), 1)
        e1.train_steps(_perm_plan(e1, by, negy, 2), 1)
    elif path == "prepared":
        e1.fwd_bwd(_perm_plan(e1, bx, negx, 8))
        plan_y = _perm_plan(e1, by, negy, 2)
        e1.adam_step_prepare_next(plan_y)                  # Adam of X's step + prep of Y in one launch
        e1.fwd_bwd_prepared(plan_y)
    else:
        weighted(e1, bx, negx)
        weighted(e1, by, negy)
    got = _grads(e1)
    assert int(e1.state[3]) == 2
    monkeypatch.setenv("DR4SR_NO_FUSE", "1")
    e2 = _engine(8, dev, lr=0.0)
    e2.state[3] = 1
    if path == "weighted":
        weighted(e2, by, negy)
    else:
        e2.fwd_bwd(e2.make_plan(by[0], by[1], by[2], neg_item=negy, sample_neg=False))
    _assert_close(got, _grads(e2), sum(ly), "stale " + path)


PATTERN = 0xA5


def _fill_keep(eng, plan):
    layers, _ = _offsets(eng, plan)
    for w in layers:
        o, n = w["attn_keep"]
        eng.workspace[o:o + n].fill_(PATTERN)


def _keep_untouched(eng, plan):
    layers, _ = _offsets(eng, plan)
    torch.cuda.synchronize()
    return all(bool((eng.workspace[o:o + n] == PATTERN).all()) for o, n in (w["attn_keep"] for w in layers))


@pytest.mark.parametrize("det", [False, True])
def test_without_dropout_nothing_is_stored_and_the_step_equals_the_unfused_step(monkeypatch, det):
    """p = 0: no KB launch — the keep area keeps its pattern — and the step is the DR4SR_NO_FUSE step's"""
    if det:
        monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    dev = torch.device("cuda", 0)
    L, lengths = LENGTHS["B7"]
    data, neg = _inputs(dev, L, lengths)
    fused, eng, plan = _step(dev, L, lengths, 0.0, "fwd_bwd", neg, data, prefill=_fill_keep)
    assert _keep_untouched(eng, plan)
    monkeypatch.setenv("DR4SR_NO_FUSE", "1")
    _assert_close(fused, _step(dev, L, lengths, 0.0, "fwd_bwd", neg, data)[0], sum(lengths), "p 0")


@pytest.mark.parametrize("det", [False, True])
def test_evaluation_stores_nothing_and_equals_the_unfused_forward(monkeypatch, det):
    """training = 0 on an engine with p = 0.5: queries equal to the DR4SR_NO_FUSE forward's within 2e-5 (relerr), keep area untouched; with
    dropout the same engine's training step DOES rewrite the area (the pattern check can fail)"""
    from dr4sr_amd import _lib
    if det:
        monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    dev = torch.device("cuda", 0)
    L, lengths = LENGTHS["B7"]
    data, neg = _inputs(dev, L, lengths)
    eng = _engine(len(lengths), dev)
    plan = eng.make_plan(data[0], data[1], data[2], neg_item=neg, sample_neg=False)
    _fill_keep(eng, plan)
    q = eng.encode(plan, False, _lib.POOL_ORIGIN)
    assert _keep_untouched(eng, plan)
    eng.fwd_bwd(plan)
    assert not _keep_untouched(eng, plan)
    monkeypatch.setenv("DR4SR_NO_FUSE", "1")
    e2 = _engine(len(lengths), dev)
    q2 = e2.encode(e2.make_plan(data[0], data[1], data[2], neg_item=neg, sample_neg=False), False, _lib.POOL_ORIGIN)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(q).all()) and float(q2.abs().max()) > 0.0
    e = relerr(q, q2)
    print("evaluation queries relerr %.2e" % e)
    assert e < TOL


# ------------------------------------------------------------------------------------------------ 3. dead stores of the fused last layer
def _nan_last_layer(eng, plan):
    layers, _ = _offsets(eng, plan)
    for name in ("u1", "st1", "a", "u2", "st2"):
        o, n = layers[NL - 1][name]
        eng.workspace[o:o + n].view(torch.float32).fill_(float("nan"))


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("path", ["fwd_bwd", "train_steps"])
@pytest.mark.parametrize("shape", sorted(LENGTHS))
def test_last_layer_row_state_is_neither_stored_nor_read(monkeypatch, shape, path, det):
    """the cases of test_fused_step_equals_unfused_step at p = 0.5 — eight length lists, both paths, default and deterministic mode (the DET
    instantiations of k_post_mid) — with u1 / st1 / a / u2 / st2 of the last layer holding NaN before the fused step: finite gradients and
    loss, equal to the unfused step's, and the buffers still hold NaN afterwards (nothing stored them)"""
    if det:
        monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    dev = torch.device("cuda", 0)
    L, lengths = LENGTHS[shape]
    data, neg = _inputs(dev, L, lengths)
    fused, eng, plan = _step(dev, L, lengths, 0.5, path, neg, data, prefill=_nan_last_layer)
    layers, _ = _offsets(eng, plan)
    for name in ("u1", "st1", "a", "u2", "st2"):
        o, n = layers[NL - 1][name]
        assert bool(torch.isnan(eng.workspace[o:o + n].view(torch.float32)).all()), name
    monkeypatch.setenv("DR4SR_NO_FUSE", "1")
    unfused = _step(dev, L, lengths, 0.5, path, neg, data)[0]
    _assert_close(fused, unfused, sum(lengths), "nan %s %s det %d" % (shape, path, det))
