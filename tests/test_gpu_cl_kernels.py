"""Unit tests of csrc/cl.hip and of the negative samplers, each kernel against a definition outside it.

  1. k_cl_augment, bit for bit against its host mirror (oracle/cl4srec_oracle.py augment_mirror; the mirror's DISTRIBUTION is checked by
     tests/test_cl_augment_cpu.py), through all four entry points.
  2. k_infonce_fwd / k_infonce_bwd against float64 torch (CO.infonce on the valid rows, gradients from autograd).  Tolerance: the
     convention of tests/test_gpu_regen_score.py: |HIP - float64| <= 16 x err32, err32 = max |fp32 torch on the CPU - float64| of the
     same quantity on the same inputs, computed here; what is exactly 0 in float64 is exactly 0 from the kernel.
     The unit has a floor of half an fp32 ulp of the largest value (the issue's err32 alone is ill-defined for a quantity of one or
     two elements: a single rounding, anywhere between 0 and half an ulp).  stats[1], an fp32 atomic sum whose last ulps depend on
     the order of the atomics, is held to the float64 sum of the kernel's own loss_row by a bound on its additions that holds in any
     order.  Every case prints its units, errors and ratios.  One run on the MI355X gave at most: loss_row 2.13, lse 10.2 (B = 1,
     D = 128), dxi 2.12, dxj 2.52 units of the 16 allowed; stats[1] 0.22 of its bound.
  3. the step glue (dr4sr_cl_prepare*, dr4sr_cl_scalars*, dr4sr_infonce_bwd_scaled) against the formulas of their header comments.
  4. dr4sr_neg_sample* and the in-step negatives of the SASRec, GRU4Rec and FMLP steps against neg_sample_mirror / fmlp_neg_mirror.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from dr4sr_amd import _lib
from oracle import cl4srec_oracle as CO

pytestmark = pytest.mark.gpu

DEV = "cuda"
E_ARG, E_SHAPE = -1, -2
PARAMS = ((0.2, 0.7, 0.2), (1.0, 1.0, 1.0), (0.01, 0.01, 0.01))          # (tau, gamma, beta)
SEEDS = (2023, (1 << 40) + 77)
MASK_IDS = (1000, 2 ** 40 + 5)


def lib():
    return _lib.load()


def dev(a, dtype=torch.int64):
    return torch.as_tensor(np.asarray(a)).to(dtype).to(DEV).contiguous()


def sync_check(rc, what):
    _lib.check(rc, what)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 1. augmentation
def aug_batch(rows, L, seed):
    """rows sequences of L columns, every column filled (the columns behind a sequence's length are copied or dropped, never used);
    lengths from [1, L], and where there are rows enough one each of 0, 1, 2, L and L + 3 (clamped by the kernel)"""
    g = np.random.default_rng(seed)
    seq = g.integers(1, 900, (rows, L))
    sl = g.integers(1, L + 1, rows)
    if rows >= 5:
        sl[[0, 1, 2, 3, rows - 1]] = [0, 1, 2, L, L + 3]
    return seq.astype(np.int64), sl.astype(np.int64)


def run_augment(entry, seq, sl, mode, prm, mask_id, seed, s, rows=None):
    """[(view, length)] of call number s (and s + 1 for the two-view entry points) through entry point `entry`"""
    B, L = (len(rows) if rows is not None else seq.shape[0]), seq.shape[1]
    seq_d, sl_d = dev(seq), dev(sl)
    keep = seq_d.clone(), sl_d.clone()
    outs = [(torch.full((B, L), -1, dtype=torch.int64, device=DEV), torch.full((B,), -1, dtype=torch.int64, device=DEV)) for _ in range(2)]
    (o1, l1), (o2, l2) = outs
    p, args = _lib.ptr, (B, L, mode, *prm, mask_id, seed)
    step_dev = torch.tensor([s - 3], dtype=torch.int32, device=DEV)            # *step_dev + offset = s
    if entry == "host":
        rc, n = lib().dr4sr_cl_augment(p(seq_d), p(sl_d), p(o1), p(l1), *args, s, _lib.cur_stream()), 1
    elif entry == "dev":
        rc, n = lib().dr4sr_cl_augment_dev(p(seq_d), p(sl_d), p(o1), p(l1), *args, p(step_dev), 3, _lib.cur_stream()), 1
    elif entry == "two":
        rc, n = lib().dr4sr_cl_augment2_dev(p(seq_d), p(sl_d), p(o1), p(l1), p(o2), p(l2), *args, p(step_dev), 3, _lib.cur_stream()), 2
    else:
        rows_d = dev(rows)
        rc, n = lib().dr4sr_cl_augment2_rows_dev(p(seq_d), p(sl_d), p(rows_d), p(o1), p(l1), p(o2), p(l2), *args, p(step_dev), 3,
                                                 _lib.cur_stream()), 2
    sync_check(rc, entry)
    assert torch.equal(seq_d, keep[0]) and torch.equal(sl_d, keep[1]) and int(step_dev) == s - 3          # inputs unchanged
    return [(o.cpu(), l.cpu()) for o, l in outs[:n]]


def assert_views_equal_mirror(entry, seq, sl, mode, prm, mask_id, seed, s, rows=None):
    got = run_augment(entry, seq, sl, mode, prm, mask_id, seed, s, rows)
    for k, (view, length) in enumerate(got):
        out, out_len, _ = CO.augment_mirror(seq, sl, mode, *prm, mask_id, seed, s + k, rows=rows)
        what = (entry, seq.shape, mode, prm, mask_id, seed, s + k)
        assert torch.equal(view, torch.from_numpy(out)), what
        assert torch.equal(length, torch.from_numpy(out_len)), what


@pytest.mark.parametrize("L", [1, 7, 50, 64])
@pytest.mark.parametrize("B", [1, 15, 16, 17, 300])
def test_augment_equals_mirror_bit_for_bit(B, L):
    """B: one partial 16-sequence workgroup, exactly one, one and a remainder, many; every mode with every parameter triple"""
    seq, sl = aug_batch(B, L, 100 * B + L)
    for mode in range(4):
        for prm in PARAMS:
            assert_views_equal_mirror("host", seq, sl, mode, prm, MASK_IDS[0], SEEDS[0], 5 + mode)


@pytest.mark.parametrize("B,L", [(17, 50), (300, 64)])
def test_augment_entry_points_seeds_and_mask_ids(B, L):
    """entry point, seed and mask id varied one at a time; the rows form on a dataset of 500 rows addressed through a rows vector
    that is not monotonic and holds a duplicate"""
    seq, sl = aug_batch(B, L, 7 * B + L)
    data, data_len = aug_batch(500, L, 11 * B + L)
    rows = np.random.default_rng(B).permutation(500)[:B].astype(np.int64)
    rows[[1, 4, 7, 10, 13]] = [499, 2, 0, 3, 1]             # the dataset rows of length L + 3, 2, 0, L and 1 are in the batch
    rows[-1] = rows[0]
    assert sorted(data_len[rows[[1, 4, 7, 10, 13]]].tolist()) == [0, 1, 2, L, L + 3]
    assert (np.diff(rows) < 0).any() and (np.diff(rows) > 0).any()
    for mode in range(4):
        for entry in ("host", "dev", "two"):
            assert_views_equal_mirror(entry, seq, sl, mode, PARAMS[0], MASK_IDS[0], SEEDS[0], 40)
        assert_views_equal_mirror("rows", data, data_len, mode, PARAMS[0], MASK_IDS[0], SEEDS[0], 40, rows=rows)
        assert_views_equal_mirror("host", seq, sl, mode, PARAMS[0], MASK_IDS[0], SEEDS[1], 40)
        assert_views_equal_mirror("host", seq, sl, mode, PARAMS[0], MASK_IDS[1], SEEDS[0], 40)


def test_augment_argument_checks():
    one = torch.full((4, 64), -1, dtype=torch.int64, device=DEV)
    p, st = _lib.ptr(one), _lib.cur_stream()
    tail = (0.2, 0.7, 0.2, 10, 0, 0, st)
    assert lib().dr4sr_cl_augment(p, p, p, p, 4, 65, 0, *tail) == E_ARG
    assert lib().dr4sr_cl_augment(p, p, p, p, 4, 0, 0, *tail) == E_ARG
    assert lib().dr4sr_cl_augment(p, p, p, p, 4, 50, 4, *tail) == E_ARG
    out, out_len = torch.full((4, 50), -1, dtype=torch.int64, device=DEV), torch.full((4,), -1, dtype=torch.int64, device=DEV)
    assert lib().dr4sr_cl_augment(p, p, _lib.ptr(out), _lib.ptr(out_len), 0, 50, 0, *tail) == 0           # empty batch: nothing written
    torch.cuda.synchronize()
    assert bool((out == -1).all()) and bool((out_len == -1).all())


# ------------------------------------------------------------------------------------------------ 2. InfoNCE
FACTOR = 16.0
# The unit of a quantity is err32 = max |fp32 torch - float64| over its elements, but never less than half an fp32 ulp of the largest
# float64 value: that is the error a correctly rounded fp32 result may have.  Over hundreds of elements err32 lies well above this floor;
# for a quantity of one or two elements (lse at B = 1, 2) err32 is a single rounding that falls anywhere between 0 and half an ulp, and a
# bound of 16 times it would measure that luck (lse at B = 1, D = 128: torch lands 0.1 ulp from float64, the kernel's chain of 32 MFMA
# accumulations 5 ulp, as lse does in every other case).
ULP_FLOOR = 0.5


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def infonce_inputs(B, D, scale, p_valid, seed):
    g = torch.Generator().manual_seed(seed)
    xi, xj = torch.randn(B, D, generator=g) * 0.5 * scale, torch.randn(B, D, generator=g) * 0.5 * scale
    valid = torch.rand(B, generator=g) < p_valid
    return xi, xj, valid


def infonce_reference(xi, xj, valid, T, dtype):
    """{loss_row, lse, sum, dxi, dxj} of the valid rows' InfoNCE in `dtype` on the CPU; invalid rows are 0 everywhere.
    loss_row[i] = lse[i] - logits[i][i]; the gradients are those of sum(loss_row) (the kernel's, at scale 1)"""
    B = xi.shape[0]
    a, b = xi.to(dtype).requires_grad_(True), xj.to(dtype).requires_grad_(True)
    out = {k: torch.zeros(B, dtype=dtype) for k in ("loss_row", "lse")}
    nv = int(valid.sum())
    if nv:
        av, bv = a[valid], b[valid]
        rows = CO.infonce(av, bv, T, reduce=False) * nv
        rows.sum().backward()
        logits = torch.cat([av @ bv.T, (av @ av.T).masked_fill(torch.eye(nv, dtype=torch.bool), float("-inf"))], -1) / T
        out["loss_row"][valid], out["lse"][valid] = rows.detach(), torch.logsumexp(logits.detach(), -1)
    out["sum"] = out["loss_row"].sum().reshape(1)
    out["dxi"] = a.grad if a.grad is not None else torch.zeros_like(xi, dtype=dtype)
    out["dxj"] = b.grad if b.grad is not None else torch.zeros_like(xj, dtype=dtype)
    return {k: v.detach() for k, v in out.items()}


def hip_infonce_fwd(xi, xj, valid, T):
    B, D = xi.shape
    xi_d, xj_d = xi.to(DEV), xj.to(DEV)
    v_d = None if valid is None else valid.to(torch.uint8).to(DEV)
    lse, loss_row = (torch.full((B + 1,), float("nan"), device=DEV) for _ in range(2))         # one guard element behind each
    stats = torch.zeros(2, device=DEV)
    sync_check(lib().dr4sr_infonce_fwd(_lib.ptr(xi_d), _lib.ptr(xj_d), _lib.ptr(v_d), B, D, T, _lib.ptr(lse), _lib.ptr(loss_row),
                                       _lib.ptr(stats), _lib.cur_stream()), "dr4sr_infonce_fwd")
    assert bool(torch.isnan(lse[B])) and bool(torch.isnan(loss_row[B]))
    return xi_d, xj_d, v_d, lse[:B].contiguous(), loss_row[:B], stats


def hip_infonce_bwd(xi_d, xj_d, v_d, T, lse, scale):
    B, D = xi_d.shape
    dxi, dxj = torch.zeros(B, D, device=DEV), torch.zeros(B, D, device=DEV)
    sc = None if scale is None else torch.tensor([scale], dtype=torch.float32, device=DEV)
    sync_check(lib().dr4sr_infonce_bwd(_lib.ptr(xi_d), _lib.ptr(xj_d), _lib.ptr(v_d), B, D, T, _lib.ptr(lse), _lib.ptr(sc), _lib.ptr(dxi),
                                       _lib.ptr(dxj), _lib.cur_stream()), "dr4sr_infonce_bwd")
    return dxi, dxj


def within(name, case, hip, r64, r32, scale=1.0):
    """|hip - scale r64| <= 16 units, unit = max(err32, half an ulp of the largest value), and exact zeros where float64 has exact zeros;
    prints err32, the unit, the error and error / unit"""
    hip = hip.detach().cpu().double()
    want, have32 = r64 * scale, (r32 * np.float32(scale)).double()
    err32, err, top = float((have32 - want).abs().max()), float((hip - want).abs().max()), float(want.abs().max())
    unit = max(err32, ULP_FLOOR * ulp32(top)) if top > 0 else 0.0
    ratio = err / unit if unit > 0 else (0.0 if err == 0 else float("inf"))
    print(f"{case} {name}: err32 {err32:.3e}  unit {unit:.3e}  |HIP - f64| {err:.3e}  ratio {ratio:.2f}  (max |f64| {top:.3e})")
    assert bool(torch.isfinite(hip).all()), (case, name)
    assert bool((hip[want == 0] == 0).all()), (case, name, "exact zeros")
    return err <= FACTOR * unit, f"{case} {name}: ratio {ratio:.2f} > {FACTOR:.0f}", unit


def stats_sum_is_the_sum_of_loss_row(case, stats, loss_row, r64, n_valid, row_unit):
    """stats[1] is the fp32 sum of the kernel's own loss_row: per row tile a four-level shuffle tree over its 16 rows, then one atomic add
    per tile in whatever order the tiles arrive, so its last ulps change from launch to launch.  Against the float64 sum of those very
    rows every one of these additions errs by at most 2^-24 of the sum of |loss_row| (the rows are >= 0, so no partial sum exceeds it):
    |stats[1] - sum| <= (tiles + 5) 2^-24 sum |loss_row| whatever the order (4 for the tree, 1 for second-order terms).  A dropped,
    doubled or misplaced row moves the sum by a whole loss_row, 1e4 times this bound.  The float64 sum of the kernel's rows is in turn
    within n_valid x 16 units of the reference's, by the bound loss_row meets row by row; err32 of the scalar itself is one rounding of
    torch's pairwise sum (0.04 .. 0.2 ulp in these cases) and bounds nothing"""
    own = loss_row.detach().cpu().double()
    tiles = (own.numel() + 15) // 16
    bound = (tiles + 5) * 2.0 ** -24 * float(own.abs().sum())
    err = abs(float(stats[1]) - float(own.sum()))
    print(f"{case} stats[1]: |stats[1] - f64 sum of the kernel's loss_row| {err:.3e}  bound {bound:.3e}  "
          f"(|f64 sum of loss_row - reference| {abs(float(own.sum()) - float(r64['sum'])):.3e})")
    assert err <= bound, (case, err, bound)
    assert abs(float(own.sum()) - float(r64["sum"])) <= n_valid * FACTOR * row_unit, case


def check_infonce(case, xi, xj, valid, T, use_valid=True):
    """forward and both backward scales of one case against float64; `valid` a bool [B] tensor; use_valid=False passes NULL"""
    B = xi.shape[0]
    mask = valid if use_valid else torch.ones(B, dtype=torch.bool)
    r64, r32 = (infonce_reference(xi, xj, mask, T, dt) for dt in (torch.float64, torch.float32))
    xi_d, xj_d, v_d, lse, loss_row, stats = hip_infonce_fwd(xi, xj, valid if use_valid else None, T)
    res = [within("loss_row", case, loss_row, r64["loss_row"], r32["loss_row"]), within("lse", case, lse, r64["lse"], r32["lse"])]
    assert float(stats[0]) == float(mask.sum()), case
    if res[0][0]:
        stats_sum_is_the_sum_of_loss_row(case, stats, loss_row, r64, int(mask.sum()), res[0][2])
    s037 = float(torch.tensor(0.37, dtype=torch.float32))
    for scale in (s037, None):
        dxi, dxj = hip_infonce_bwd(xi_d, xj_d, v_d, T, lse, scale)
        tag = "" if scale is None else " x0.37"
        res.append(within("dxi" + tag, case, dxi, r64["dxi"], r32["dxi"], 1.0 if scale is None else scale))
        res.append(within("dxj" + tag, case, dxj, r64["dxj"], r32["dxj"], 1.0 if scale is None else scale))
    bad = [msg for ok, msg, _ in res if not ok]
    assert not bad, bad
    return r64, (lse, loss_row, stats)


@pytest.mark.parametrize("use_valid", [True, False])
@pytest.mark.parametrize("B", [1, 2, 15, 16, 17, 37, 130, 257])
@pytest.mark.parametrize("D", [64, 128])
def test_infonce_against_float64(D, B, use_valid):
    """B: a single row (its only logit is the positive: loss 0); below, at and above the 16-row tile; 257 = 17 row tiles, 34 column
    tiles for the forward's 16 waves.  N(0, 0.5^2) inputs, T = 1, 85 % valid with row 0 valid; and valid = NULL"""
    xi, xj, valid = infonce_inputs(B, D, 1.0, 0.85, 1000 + B + D)
    valid[0] = True
    check_infonce(f"D={D} B={B} valid={'85%' if use_valid else 'NULL'}", xi, xj, valid, 1.0, use_valid)


@pytest.mark.parametrize("B,scale,T,p_valid", [(130, 1.5, 0.2, 0.85), (257, 1.0, 0.1, 0.5)])
@pytest.mark.parametrize("D", [64, 128])
def test_infonce_sharp_logits_against_float64(D, B, scale, T, p_valid):
    """logits of several hundred: the online log-sum-exp and the fast exponential carry the result; err32 scales with the case"""
    xi, xj, valid = infonce_inputs(B, D, scale, p_valid, 2000 + B + D)
    valid[0] = True
    check_infonce(f"D={D} B={B} T={T} inputs x{scale}", xi, xj, valid, T)


@pytest.mark.parametrize("D", [64, 128])
def test_infonce_sparse_valid_masks(D):
    """10 % valid; a whole row tile and column tile of invalid rows; one valid row in the last tile (loss 0, all gradients 0);
    no valid row at all (everything 0, nothing NaN)"""
    xi, xj, valid = infonce_inputs(40, D, 1.0, 0.10, 3000 + D)
    valid[0] = True
    check_infonce(f"D={D} B=40 10% valid", xi, xj, valid, 1.0)
    xi, xj, valid = infonce_inputs(48, D, 1.0, 2.0, 3100 + D)
    valid[16:32] = False
    check_infonce(f"D={D} B=48 rows 16..31 invalid", xi, xj, valid, 1.0)
    xi, xj, valid = infonce_inputs(33, D, 1.0, -1.0, 3200 + D)
    valid[32] = True
    r64, (lse, loss_row, stats) = check_infonce(f"D={D} B=33 only row 32 valid", xi, xj, valid, 1.0)
    assert float(r64["loss_row"].abs().max()) == 0 and float(r64["dxi"].abs().max()) == 0 and float(r64["dxj"].abs().max()) == 0
    assert stats.tolist() == [1.0, 0.0] and float(loss_row.abs().max()) == 0
    xi, xj, valid = infonce_inputs(20, D, 1.0, -1.0, 3300 + D)
    r64, (lse, loss_row, stats) = check_infonce(f"D={D} B=20 no valid row", xi, xj, valid, 1.0)
    assert stats.tolist() == [0.0, 0.0] and float(lse.abs().max()) == 0 and float(loss_row.abs().max()) == 0


def test_infonce_argument_checks():
    one = torch.zeros(8 * 128, device=DEV)
    p, st = _lib.ptr(one), _lib.cur_stream()
    assert lib().dr4sr_infonce_fwd(p, p, None, 8, 96, 1.0, p, p, p, st) == E_SHAPE
    assert lib().dr4sr_infonce_bwd(p, p, None, 8, 96, 1.0, p, None, p, p, st) == E_SHAPE
    assert lib().dr4sr_infonce_bwd_scaled(p, p, None, 8, 96, 1.0, p, p, p, 0.1, 0, p, p, st) == E_SHAPE
    assert lib().dr4sr_infonce_fwd(p, p, None, 8, 64, 0.0, p, p, p, st) == E_ARG
    assert lib().dr4sr_infonce_bwd(p, p, None, 8, 64, 0.0, p, None, p, p, st) == E_ARG
    assert lib().dr4sr_infonce_fwd(p, p, None, 0, 64, 1.0, p, p, p, st) == E_ARG
    assert lib().dr4sr_infonce_bwd(p, p, None, 0, 64, 1.0, p, None, p, p, st) == E_ARG
    torch.cuda.synchronize()
    assert float(one.abs().max()) == 0


# ------------------------------------------------------------------------------------------------ 3. step glue
@pytest.mark.parametrize("B", [1, 255, 256, 257])
def test_cl_prepare_in_its_three_forms(B):
    """valid = (seqlen != 1) (through rows too), stats = 0, zero[0..nzero) = 0 and nothing behind it, *step_dev += step_add once;
    nzero = 256 * 512 + 3 is more than the 512 blocks of the largest grid cover in one pass"""
    g = np.random.default_rng(B)
    sl = g.integers(0, 6, B)
    sl[:3] = [1, 0, 2][:min(B, 3)]
    data_len = g.integers(0, 4, 400)
    rows = g.permutation(400)[:B]
    rows[-1] = rows[0]
    p, st = _lib.ptr, _lib.cur_stream()
    for nzero in (0, 1, 256 * 512 + 3):
        for form in ("batch", "rows", "rows_step"):
            valid = torch.full((B + 8,), 9, dtype=torch.uint8, device=DEV)
            stats = torch.full((3,), 7.0, device=DEV)
            zero = torch.full((nzero + 1,), 5.0, device=DEV)
            step_dev = torch.tensor([41], dtype=torch.int32, device=DEV)
            if form == "batch":
                lens, want = dev(sl), sl != 1
                rc = lib().dr4sr_cl_prepare(p(lens), B, p(valid), p(stats), p(zero), nzero, st)
            else:
                lens, rows_d, want = dev(data_len), dev(rows), data_len[rows] != 1
                if form == "rows":
                    rc = lib().dr4sr_cl_prepare_rows(p(lens), p(rows_d), B, p(valid), p(stats), p(zero), nzero, st)
                else:
                    rc = lib().dr4sr_cl_prepare_rows_step(p(lens), p(rows_d), B, p(valid), p(stats), p(zero), nzero, p(step_dev), 3, st)
            sync_check(rc, form)
            what = (B, nzero, form)
            assert valid[:B].cpu().numpy().tolist() == want.astype(np.uint8).tolist() and bool((valid[B:] == 9).all()), what
            assert stats.tolist() == [0.0, 0.0, 7.0], what
            assert float(zero[:nzero].abs().max()) == 0 if nzero else True, what
            assert float(zero[nzero]) == 5.0, what
            assert int(step_dev) == (44 if form == "rows_step" else 41), what


def f32(*v):
    return torch.tensor(v, dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("rows", [23.0, 0.0])
def test_cl_scalars_against_their_formulas(rows):
    """scale = cl_weight n_valid / rows, loss = loss_sum / n_valid + cl_weight stats[1] / rows; rows = 0: scale 0, the main term only"""
    clw = float(np.float32(0.1))
    tail, stats = f32(412.0, 655.25), f32(rows, 81.5 if rows else 0.0)
    scale, loss = f32(-1.0), f32(-1.0)
    p, st = _lib.ptr, _lib.cur_stream()
    sync_check(lib().dr4sr_cl_scalars(p(tail), p(stats), clw, p(scale), p(loss), st), "dr4sr_cl_scalars")
    want_scale = clw * 412.0 / rows if rows else 0.0
    want_loss = 655.25 / 412.0 + (clw * 81.5 / rows if rows else 0.0)
    assert abs(float(scale) - want_scale) <= 1e-6 * abs(want_scale) and abs(float(loss) - want_loss) <= 1e-6 * abs(want_loss)
    only = f32(-1.0)
    sync_check(lib().dr4sr_cl_scalars(p(tail), p(stats), clw, None, p(only), st), "dr4sr_cl_scalars")         # either output may be NULL
    assert float(only) == float(loss)
    assert lib().dr4sr_cl_scalars(p(tail), p(stats), clw, None, None, st) == E_ARG
    # the data-parallel form: n_valid is the sum of n_parts counts stride apart; the contrastive share of the loss goes into tail_local[1]
    parts = torch.full((3 * 5,), 1e6, device=DEV)
    parts[0], parts[5], parts[10] = 100.0, 212.0, 100.0
    local = f32(212.0, 330.5, 9.0)
    before = local.clone()
    sync_check(lib().dr4sr_cl_scalars_dp(p(parts), 3, 5, p(stats), clw, p(scale), p(local), st), "dr4sr_cl_scalars_dp")
    assert abs(float(scale) - want_scale) <= 1e-6 * abs(want_scale)
    if rows:
        want_tail = 330.5 + clw * 81.5 / rows * 212.0
        assert abs(float(local[1]) - want_tail) <= 1e-6 * want_tail and float(local[0]) == 212.0 and float(local[2]) == 9.0
    else:
        assert float(scale) == 0.0 and torch.equal(local, before)                                             # tail_local unchanged


@pytest.mark.parametrize("fold", [0, 1])
@pytest.mark.parametrize("B,D", [(37, 64), (130, 128)])
def test_infonce_bwd_scaled_computes_the_step_scalars_itself(B, D, fold):
    """scale = cl_weight tail[0] / stats[0] inside the launch: the gradients meet the float64 bound of the plain backward; fold: tail[1]
    grows by cl_weight stats[1] / stats[0] tail[0]; tail[0] never changes"""
    xi, xj, valid = infonce_inputs(B, D, 1.0, 0.85, 4000 + B)
    valid[0] = True
    r64, r32 = (infonce_reference(xi, xj, valid, 1.0, dt) for dt in (torch.float64, torch.float32))
    xi_d, xj_d, v_d, lse, _, stats = hip_infonce_fwd(xi, xj, valid, 1.0)
    clw = float(np.float32(0.1))
    tail = f32(412.0, 655.25)
    before = tail.clone()
    dxi, dxj = torch.zeros(B, D, device=DEV), torch.zeros(B, D, device=DEV)
    p = _lib.ptr
    sync_check(lib().dr4sr_infonce_bwd_scaled(p(xi_d), p(xj_d), p(v_d), B, D, 1.0, p(lse), p(tail), p(stats), clw, fold, p(dxi), p(dxj),
                                              _lib.cur_stream()), "dr4sr_infonce_bwd_scaled")
    s0, s1 = (float(v) for v in stats.tolist())
    assert s0 == float(valid.sum())
    scale = clw * 412.0 / s0
    case = f"bwd_scaled D={D} B={B} fold={fold}"
    res = [within("dxi", case, dxi, r64["dxi"], r32["dxi"], scale), within("dxj", case, dxj, r64["dxj"], r32["dxj"], scale)]
    assert all(ok for ok, _, _ in res), [m for ok, m, _ in res if not ok]
    assert float(tail[0]) == 412.0
    if fold:
        want = 655.25 + clw * s1 / s0 * 412.0
        assert abs(float(tail[1]) - want) <= 1e-6 * want and float(tail[1]) > 655.25
    else:
        assert torch.equal(tail, before)


@pytest.mark.parametrize("fold", [0, 1])
def test_infonce_bwd_scaled_without_a_valid_row(fold):
    xi, xj, valid = infonce_inputs(20, 64, 1.0, -1.0, 4100)
    xi_d, xj_d, v_d, lse, _, stats = hip_infonce_fwd(xi, xj, valid, 1.0)
    tail = f32(412.0, 655.25)
    before = tail.clone()
    dxi, dxj = torch.zeros(20, 64, device=DEV), torch.zeros(20, 64, device=DEV)
    p = _lib.ptr
    sync_check(lib().dr4sr_infonce_bwd_scaled(p(xi_d), p(xj_d), p(v_d), 20, 64, 1.0, p(lse), p(tail), p(stats), 0.1, fold, p(dxi), p(dxj),
                                              _lib.cur_stream()), "dr4sr_infonce_bwd_scaled")
    assert stats.tolist() == [0.0, 0.0] and torch.equal(tail, before)
    assert float(dxi.abs().max()) == 0 and float(dxj.abs().max()) == 0


# ------------------------------------------------------------------------------------------------ 4. negative samplers
@pytest.mark.parametrize("n_items", [2, 37, 12102])
def test_neg_sample_equals_mirror_bit_for_bit(n_items):
    n, seed, step = 200003, (1 << 35) + 99, 6                  # n: no multiple of 4 (a Philox call) or of 256 (a workgroup)
    want = torch.from_numpy(CO.neg_sample_mirror(n, n_items, seed, step))
    out = torch.full((n + 1,), -1, dtype=torch.int64, device=DEV)
    sync_check(lib().dr4sr_neg_sample(_lib.ptr(out), n, n_items, seed, step, _lib.cur_stream()), "dr4sr_neg_sample")
    assert torch.equal(out[:n].cpu(), want) and int(out[n]) == -1
    step_dev = torch.tensor([step], dtype=torch.int32, device=DEV)
    out2 = torch.full((n + 1,), -1, dtype=torch.int64, device=DEV)
    sync_check(lib().dr4sr_neg_sample_dev(_lib.ptr(out2), n, n_items, seed, _lib.ptr(step_dev), _lib.cur_stream()), "dr4sr_neg_sample_dev")
    assert torch.equal(out2, out) and int(step_dev) == step
    assert int(want.min()) == 1 and int(want.max()) == n_items - 1              # n_items = 2: every id is 1


def left_aligned_batch(B, L, N, seed):
    g = np.random.default_rng(seed)
    sl = g.integers(1, L + 1, B)
    sl[:2] = [1, L]
    keep = np.arange(L)[None, :] < sl[:, None]
    ids, tgt = g.integers(1, N, (B, L)) * keep, g.integers(1, N, (B, L)) * keep
    return dev(ids), dev(tgt), dev(sl), keep


def fill_params(eng, seed):
    g = torch.Generator().manual_seed(seed)
    for name, v in eng.views.items():
        v.copy_(torch.ones(v.shape) if ("norm" in name.lower() and name.endswith("weight")) else 0.05 * torch.randn(v.shape, generator=g))
    eng.views["item_embedding.weight"][0] = 0


def assert_two_steps_draw_the_mirror(eng, plan, neg, mirror, keep=None):
    """after each of two fwd_bwd calls the caller's buffer holds the mirror's ids of the step's state[RNGSTEP] (where keep is set)"""
    seen = []
    for _ in range(2):
        neg.fill_(-1)
        eng.fwd_bwd(plan)
        torch.cuda.synchronize()
        step = int(eng.state[_lib.STATE_RNGSTEP])
        got, want = neg.cpu().numpy().reshape(-1), mirror(step)
        sel = slice(None) if keep is None else keep.reshape(-1)
        assert (got[sel] == want[sel]).all(), (type(eng).__name__, step)
        seen.append((step, got[sel].copy()))
    assert seen[1][0] == seen[0][0] + 1 and not (seen[0][1] == seen[1][1]).all()


@pytest.mark.parametrize("form", ["latency", "scale"])
def test_sasrec_step_negatives_equal_mirror(monkeypatch, form):
    from dr4sr_amd.engine import SasrecEngine
    if form == "scale":
        monkeypatch.setenv("DR4SR_FORCE_SCALE", "1")
    B, L, N = 37, 50, 300
    ids, tgt, sl, keep = left_aligned_batch(B, L, N, 5)
    eng = SasrecEngine(N, L, 64, 2, 128, 1, 1e-12, 0.0, B, DEV, seed=(1 << 33) + 5)
    fill_params(eng, 1)
    neg = torch.zeros(B, L, dtype=torch.int64, device=DEV)
    plan = eng.make_plan(ids, tgt, sl, neg_item=neg, sample_neg=True)
    forms = eng.lib.dr4sr_sasrec_at_scale(C.byref(plan))                  # bit 0: the at-scale token-tile kernels (include/dr4sr_hip.h)
    assert forms >= 0 and bool(forms & 1) == (form == "scale"), forms
    assert_two_steps_draw_the_mirror(eng, plan, neg, lambda step: CO.neg_sample_mirror(B * L, N, eng.seed, step), keep)


def test_gru4rec_step_negatives_equal_mirror():
    from dr4sr_amd.gru_engine import GruEngine
    B, L, N = 37, 50, 300
    ids, tgt, sl, keep = left_aligned_batch(B, L, N, 6)
    eng = GruEngine(N, L, 64, 128, 1, 0.0, B, DEV, seed=77)
    fill_params(eng, 2)
    neg = torch.zeros(B, L, dtype=torch.int64, device=DEV)
    plan = eng.make_plan(ids, tgt, sl, neg_item=neg, sample_neg=True)
    assert_two_steps_draw_the_mirror(eng, plan, neg, lambda step: CO.neg_sample_mirror(B * L, N, eng.seed, step), keep)


def test_fmlp_step_negatives_equal_mirror():
    from dr4sr_amd.fmlp_engine import FmlpEngine
    B, L, N = 33, 20, 300
    g = np.random.default_rng(7)
    sl = g.integers(1, L + 1, B)
    ids = g.integers(1, N, (B, L)) * (np.arange(L)[None, :] >= L - sl[:, None])           # right-aligned rows, one target each
    eng = FmlpEngine(N, L, 64, 256, 1, 1e-12, 0.0, B, DEV, seed=78)
    fill_params(eng, 3)
    neg = torch.zeros(B, dtype=torch.int64, device=DEV)
    plan = eng.make_plan(dev(ids), dev(g.integers(1, N, B)), neg_item=neg, sample_neg=True)
    assert_two_steps_draw_the_mirror(eng, plan, neg, lambda step: CO.fmlp_neg_mirror(B, N, eng.seed, step))
