"""The cross-lane primitives of csrc/common.h without LDS traffic (DPP row rotations / shifts / quad permutes, v_permlane16_swap,
v_permlane32_swap) against the shuffle forms they replaced in the d = 64 latency kernels: dr4sr_lane_probe (include/dr4sr_hip_probes.h, csrc/probe.hip) runs both forms of
every primitive on the same inputs, loaded straight into the reduction.

Inputs: 4 blocks x 256 lanes.  Every 16-lane group has its own base magnitude — the 64 bases cover 2^-20 .. 2^18 — and its lanes spread over
two binades above it with mixed signs, so that almost every add of a butterfly rounds and the pairing order shows in the low bits.  Blocks
0 and 1 are finite normals only; block 2 also holds +-0 and denormals; block 3 also +-inf and NaN.

How well the inputs discriminate (test_inputs_discriminate_pairing_orders, CPU): emulating the 16-lane butterfly in the wrong step order
(1, 2, 4, 8) changes the bits of 22 of the 32 groups of blocks 0 and 1 (0.6875); pairing lane i with 7 - i in the first step of the 8-lane
form changes 32 of the 64 groups (0.5).

Deliberately wrong builds of csrc/common.h run against this file (not committed), cases of the two device tests that fail:
  - the 16-lane sum with a rotation by 4 as its first step:     both tests fail for group16_sum and for every sum built on it (wave_sum, and
                                                                 a 32-lane sum the probe still had then): 6 of 16 cases
  - group8_sum pairing lane i with 7 - i (row_half_mirror):     both tests fail for group8_sum: 2 of 16 cases
"""
import numpy as np
import pytest
import torch

N_BLOCKS, BLOCK = 4, 256
N = N_BLOCKS * BLOCK
FINITE = 2 * BLOCK            # blocks 0, 1: finite normals only (the numpy emulation is compared there)

# primitive -> (group size, butterfly offsets in the function's order, numpy op)
BUTTERFLIES = {
    "group16_sum": (16, (8, 4, 2, 1), np.add),
    "group8_sum": (8, (4, 2, 1), np.add),
    "wave_sum": (64, (32, 16, 8, 4, 2, 1), np.add),
    "xg_sum": (64, (16, 32), np.add),
    "fold": (64, (16, 32), np.add),
}


def _inputs():
    rng = np.random.default_rng(20261020)
    spread = 2.0
    base = np.repeat(np.linspace(-20.0, 20.0 - spread, N // 16), 16).reshape(-1, 16)[rng.permutation(N // 16)].reshape(-1)
    v = (np.exp2(base + rng.uniform(0.0, spread, N)) * rng.choice([-1.0, 1.0], N)).astype(np.float32)
    assert np.all(np.isfinite(v)) and np.all(np.abs(v) >= np.finfo(np.float32).tiny)
    lane = np.arange(N)
    b2, b3 = 2 * BLOCK, 3 * BLOCK
    v[b2 + 3:b3:16] = 0.0
    v[b2 + 9:b3:32] = -0.0
    v[b2 + 5:b3:16] = np.float32(1e-41)                 # denormals
    v[b2 + 12:b3:32] = np.float32(-3e-39)
    # max over the four rows with +0 and -0 tied for it, in both orders (lane 9 of waves 0 and 1 of block 2; rows 0 and 2 hold -0 already)
    v[b2 + 16 + 9], v[b2 + 48 + 9] = 0.0, -abs(v[b2 + 48 + 9])
    v[b2 + 64 + 16 + 9], v[b2 + 64 + 48 + 9] = -abs(v[b2 + 64 + 16 + 9]), 0.0
    # block 3, 16-lane groups g = 0..15 (four per wave): wave 0 holds +inf only, wave 1 -inf only (sums stay infinite at every width), wave 2
    # +inf and -inf in different groups and in the two halves of one group, wave 3 a NaN, an infinite group beside it, and both signs in one
    # 8-lane group
    for g, lane_, x in ((0, 2, np.inf), (5, 11, -np.inf), (6, 0, -np.inf), (8, 1, np.inf), (9, 14, -np.inf), (10, 3, np.inf), (10, 12, -np.inf),
                        (12, 6, np.inf), (13, 7, np.nan), (14, 1, np.inf), (14, 5, -np.inf)):
        v[b3 + 16 * g + lane_] = x
    u = rng.integers(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32)
    return v, u, lane


def _butterfly(v, offs, op):
    lane = np.arange(v.size)
    for o in offs:
        v = op(v, v[lane ^ o]).astype(np.float32)
    return v


def test_inputs_discriminate_pairing_orders():
    """(CPU) the finite blocks tell a wrong pairing order from the right one: the shares the module docstring states"""
    v = _inputs()[0][:FINITE]
    right = _butterfly(v, (8, 4, 2, 1), np.add).view(np.uint32).reshape(-1, 16)
    wrong = _butterfly(v, (1, 2, 4, 8), np.add).view(np.uint32).reshape(-1, 16)
    assert np.all(right == right[:, :1]), "a butterfly leaves one value in all lanes of a group"
    share16 = float((right != wrong).any(axis=1).mean())
    lane = np.arange(v.size)
    mirrored = _butterfly((v + v[(lane & ~7) | (7 - (lane & 7))]).astype(np.float32), (2, 1), np.add).view(np.uint32).reshape(-1, 8)
    right8 = _butterfly(v, (4, 2, 1), np.add).view(np.uint32).reshape(-1, 8)
    share8 = float((right8 != mirrored).any(axis=1).mean())
    print(f"wrong step order changes {share16:.4f} of the 16-lane groups; i <-> 7 - i changes {share8:.4f} of the 8-lane groups")
    assert share16 >= 0.5 and share16 == 0.6875
    assert share8 == 0.5


@pytest.fixture(scope="module")
def probe_out():
    from dr4sr_amd import _lib
    dev = torch.device("cuda", 0)
    v, u, _ = _inputs()
    tin = torch.from_numpy(v).to(dev)
    tu = torch.from_numpy(u.view(np.int32)).to(dev)
    out = torch.zeros(len(_lib.LANE_PROBE_NAMES) * 2 * N, dtype=torch.int32, device=dev)
    fn = _lib.probe("dr4sr_lane_probe")
    assert fn(None, None, None, N, None) == -1 and fn(_lib.ptr(tin), _lib.ptr(tu), _lib.ptr(out), N - 1, None) == -1
    _lib.check(fn(_lib.ptr(tin), _lib.ptr(tu), _lib.ptr(out), N, _lib.cur_stream()), "dr4sr_lane_probe")
    torch.cuda.synchronize()
    o = out.cpu().numpy().view(np.uint32).reshape(len(_lib.LANE_PROBE_NAMES), 2, N)
    return {name: (o[q, 0].copy(), o[q, 1].copy()) for q, name in enumerate(_lib.LANE_PROBE_NAMES)}


PRIMS = ("group16_sum", "group8_sum", "wave_sum", "xg_max", "xg_sum", "fold", "xor1")


@pytest.mark.gpu
@pytest.mark.parametrize("name", PRIMS)
def test_shipped_form_is_bitwise_the_shuffle_form(probe_out, name):
    """primary check, on the device: every lane of the shipped form equals the *_ref shuffle form as uint32; where the reference is NaN
    (inf - inf, NaN inputs: block 3) both are NaN — payloads are not compared"""
    got, ref = probe_out[name]
    if name == "xor1":
        assert np.array_equal(got, ref)
        return
    ref_nan, got_nan = np.isnan(ref.view(np.float32)), np.isnan(got.view(np.float32))
    print(f"{name}: {int((got != ref).sum())} lanes differ as uint32, {int(ref_nan.sum())} reference lanes are NaN")
    assert np.array_equal(ref_nan, got_nan)
    assert np.array_equal(got[~ref_nan], ref[~ref_nan])
    assert ref_nan[:FINITE].sum() == 0 and np.all(np.isfinite(ref.view(np.float32)[:3 * BLOCK]))
    if name != "xg_max":
        assert ref_nan.sum() > 0 and np.isinf(ref.view(np.float32)).sum() > 0, "block 3 must reach the special values"


@pytest.mark.gpu
@pytest.mark.parametrize("name", PRIMS)
def test_both_forms_are_the_numpy_butterfly(probe_out, name):
    """secondary check, finite normal inputs (blocks 0, 1): both device forms against a numpy float32 emulation of the butterfly,
    v = v + v[lane ^ o] for o in the function's order"""
    v, u, lane = _inputs()
    got, ref = probe_out[name]
    if name == "xor1":
        want = u[lane ^ 1]
        assert np.array_equal(got, want) and np.array_equal(ref, want)
        return
    x = v[:FINITE]
    if name == "xg_max":
        l = lane[:FINITE]
        want = np.maximum(np.maximum(x, x[l ^ 16]), np.maximum(x[l ^ 32], x[l ^ 48]))
    else:
        _, offs, op = BUTTERFLIES[name]
        want = _butterfly(x, offs, op)
    want = want.view(np.uint32)
    assert np.array_equal(ref[:FINITE], want), "the shuffle reference is not the emulated butterfly"
    assert np.array_equal(got[:FINITE], want)


def _ragged_step(tokens):
    from test_gpu_parity import _random_params
    from dr4sr_amd import _lib
    from dr4sr_amd.engine import SasrecEngine
    dev = torch.device("cuda", 0)
    N_ITEMS, L, D, H, F, NL = 500, 50, 64, 2, 128, 2
    sl = []
    left = tokens
    while left > 0:
        sl.append(min(L, left))
        left -= sl[-1]
    B = len(sl)
    gen = torch.Generator().manual_seed(tokens)
    sl = torch.tensor(sl)
    idx = torch.zeros(B, L, dtype=torch.long)
    tgt = torch.zeros(B, L, dtype=torch.long)
    for i in range(B):
        idx[i, :sl[i]] = torch.randint(1, N_ITEMS, (int(sl[i]),), generator=gen)
        tgt[i, :sl[i]] = torch.randint(1, N_ITEMS, (int(sl[i]),), generator=gen)
    neg = torch.randint(1, N_ITEMS, (B, L), generator=gen)
    eng = SasrecEngine(N_ITEMS, L, D, H, F, NL, 1e-12, 0.5, B, dev, seed=2023)
    eng.load_named(_random_params(N_ITEMS, D, F, NL, seed=6))
    plan = eng.make_plan(idx.to(dev), tgt.to(dev), sl.to(dev), neg_item=neg.contiguous().to(dev), sample_neg=False)
    runs = []
    rng0 = eng.state[_lib.STATE_RNGSTEP:_lib.STATE_RNGSTEP + 1].clone()
    for _ in range(2):
        eng.state[_lib.STATE_RNGSTEP:_lib.STATE_RNGSTEP + 1].copy_(rng0)          # the same dropout masks in both runs
        eng.fwd_bwd(plan)
        torch.cuda.synchronize()
        loss, n = eng.loss_and_count()
        runs.append((eng.grads.clone(), loss, n))
    return runs, int(sl.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("tokens", [1, 17, 129])
def test_ragged_tiles_replay_bit_equal(monkeypatch, tokens):
    """one token, one token past a 16-row tile, one past eight tiles (p = 0.5, deterministic mode): two fwd_bwd of the same plan in one
    process are bit-equal — a reduction that read lanes outside its group at a ragged tile would pick up what the previous launch left"""
    monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    (g1, l1, n1), (g2, l2, n2) = _ragged_step(tokens)[0]
    assert n1 == n2 == tokens
    assert np.float32(l1).view(np.uint32) == np.float32(l2).view(np.uint32) and np.isfinite(l1)
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32))
    assert bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0.0
