"""Distribution of the draws of csrc/cl.hip k_cl_augment, on their host mirror (oracle/cl4srec_oracle.py augment_mirror; held bit-equal
to the kernel by tests/test_gpu_cl_kernels.py): crop starts, mask subsets, reorder permutations, Item_Random's method and the
independence of the streams.  No GPU and no HIP library: the mirror draws with the package's numpy Philox.

Deterministic: seed 2023, step 1, 20 000 sequences of distinct items per case, L = 50.  Every chi-square is held against the
1 - 1e-6 quantile of its distribution, every per-cell z-score against |z| < 5 (two-sided 5.7e-7 per cell).

Measured with these inputs (statistic / threshold):
  crop starts     n = 50: chi2 52.0 on 40 dof / 97.7;   n = 20: 23.5 on 16 dof / 58.3;   n = 7: 6.6 on 6 dof / 38.3
  mask            per-position max |z| 2.4 / 2.7 / 1.8 (n = 50 / 20 / 7) / 5;   adjacent pairs max |z| 2.4 / 2.2 / 2.1 / 5
  reorder         n = sub = 4: 24 permutations, chi2 24.6 on 23 dof / 70.5
                  n = 10, sub = 2: swap rate 0.4970 (z -0.83) / 5;   first moved position chi2 4.8 on 8 dof / 42.7
  Item_Random     steps 1..600: counts 187 / 208 / 205, chi2 1.29 on 2 dof / 27.6
  streams         slot b against b + 1: chi2 0.52;   step 1 against step 2: chi2 0.00;   1 dof / 23.9
"""
import itertools
import math

import numpy as np
import pytest

from oracle import cl4srec_oracle as CO

SEED, STEP, B, L = 2023, 1, 20000, 50
TAU, GAMMA, BETA, MASK_ID = 0.2, 0.7, 0.2, 1000
LENGTHS = (50, 20, 7)
Z_MAX = 5.0


def chi2_bound(dof):
    """the 1 - 1e-6 quantile of chi-square with `dof` degrees of freedom"""
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(1 - 1e-6, dof))
    except ImportError:                                    # Wilson-Hilferty; z = the normal's 1 - 1e-6 quantile
        z, a = 4.753424308822899, 2.0 / (9.0 * dof)
        return dof * (1.0 - a + z * math.sqrt(a)) ** 3


def chi2_uniform(counts):
    counts = np.asarray(counts, np.float64)
    e = counts.sum() / counts.size
    return float(((counts - e) ** 2 / e).sum())


def batch(n, rows=B):
    """rows sequences of the n distinct items 1..n, left-aligned in L columns"""
    seq = np.zeros((rows, L), np.int64)
    seq[:, :n] = np.arange(1, n + 1)
    return seq, np.full(rows, n, np.int64)


def crop_starts(n, step=STEP):
    seq, sl = batch(n)
    out, ol, mode = CO.augment_mirror(seq, sl, 0, TAU, GAMMA, BETA, MASK_ID, SEED, step)
    sub = CO.crop_len(n, TAU)
    assert mode == 0 and (ol == sub).all()
    start = out[:, 0] - 1
    assert (out[:, :sub] == start[:, None] + 1 + np.arange(sub)).all() and (out[:, sub:] == 0).all()
    return start, sub


@pytest.mark.parametrize("n", LENGTHS)
def test_crop_starts_are_uniform_over_every_legal_start(n):
    start, sub = crop_starts(n)
    cnt = np.bincount(start, minlength=n - sub + 1)
    assert cnt.size == n - sub + 1 and cnt.min() > 0            # every start in [0, n - sub] occurs, none behind it
    x = chi2_uniform(cnt)
    print(f"crop starts n={n}: chi2 {x:.1f} on {cnt.size - 1} dof, bound {chi2_bound(cnt.size - 1):.1f}")
    assert x < chi2_bound(cnt.size - 1)


@pytest.mark.parametrize("n", LENGTHS)
def test_mask_is_a_uniform_subset(n):
    seq, sl = batch(n)
    out, ol, mode = CO.augment_mirror(seq, sl, 1, TAU, GAMMA, BETA, MASK_ID, SEED, STEP)
    k = CO.mask_count(n, GAMMA)
    m = out[:, :n] == MASK_ID
    assert mode == 1 and (ol == n).all() and (m.sum(1) == k).all()           # exactly int(gamma n) per sequence
    assert (out[:, :n][~m] == seq[:, :n][~m]).all() and (out[:, n:] == 0).all()
    p = k / n
    z = (m.sum(0) - B * p) / math.sqrt(B * p * (1 - p))                       # inclusion count of a position ~ Binomial(B, k / n)
    # right marginals and a wrong joint distribution: both of two neighbours are masked with probability k (k - 1) / (n (n - 1))
    p2 = k * (k - 1) / (n * (n - 1))
    z2 = ((m[:, :-1] & m[:, 1:]).sum(0) - B * p2) / math.sqrt(B * p2 * (1 - p2))
    print(f"mask n={n}: per-position max |z| {np.abs(z).max():.2f}, adjacent pairs max |z| {np.abs(z2).max():.2f}")
    assert np.abs(z).max() < Z_MAX and np.abs(z2).max() < Z_MAX


def test_full_reorder_draws_all_24_permutations_uniformly():
    n = 4
    seq, sl = batch(n)
    out, ol, mode = CO.augment_mirror(seq, sl, 2, TAU, GAMMA, 1.0, MASK_ID, SEED, STEP)
    assert mode == 2 and (ol == n).all() and (out[:, n:] == 0).all()
    code = {p: i for i, p in enumerate(itertools.permutations(range(1, n + 1)))}
    cnt = np.bincount([code[tuple(r)] for r in out[:, :n].tolist()], minlength=24)          # KeyError: not a permutation
    x = chi2_uniform(cnt)
    print(f"reorder n=sub=4: {int((cnt > 0).sum())} permutations, chi2 {x:.1f} on 23 dof, bound {chi2_bound(23):.1f}")
    assert cnt.min() > 0 and x < chi2_bound(23)


def test_reorder_of_a_pair_swaps_half_the_time_at_a_uniform_place():
    n = 10
    seq, sl = batch(n)
    out, ol, mode = CO.augment_mirror(seq, sl, 2, TAU, GAMMA, BETA, MASK_ID, SEED, STEP)
    assert CO.reorder_len(n, BETA) == 2 and mode == 2 and (ol == n).all()
    assert (np.sort(out[:, :n], 1) == seq[:, :n]).all() and (out[:, n:] == 0).all()
    diff = out[:, :n] != seq[:, :n]
    swapped = diff.any(1)
    first = diff[swapped].argmax(1)
    assert (diff[swapped].sum(1) == 2).all() and (out[swapped, first] == first + 2).all()    # two neighbours exchanged
    z = (swapped.sum() - B / 2) / math.sqrt(B / 4)
    cnt = np.bincount(first, minlength=n - 1)
    x = chi2_uniform(cnt)
    print(f"reorder n=10 sub=2: swap rate {swapped.mean():.4f} (z {z:.2f}), first moved position chi2 {x:.1f} on 8 dof, "
          f"bound {chi2_bound(8):.1f}")
    assert cnt.size == n - 1 and cnt.min() > 0 and abs(z) < Z_MAX and x < chi2_bound(8)


def test_item_random_draws_one_method_per_call_uniformly():
    seq, sl = batch(20, rows=64)
    modes = []
    for step in range(1, 601):
        out, ol, mode = CO.augment_mirror(seq, sl, 3, TAU, GAMMA, BETA, MASK_ID, SEED, step)
        modes.append(mode)
        if step <= 30:                                     # one method for the whole batch: the call with that method named
            ref, rl, _ = CO.augment_mirror(seq, sl, mode, TAU, GAMMA, BETA, MASK_ID, SEED, step)
            assert (out == ref).all() and (ol == rl).all()
            kind = 0 if (ol != 20).all() else 1 if ((out == MASK_ID).sum(1) == CO.mask_count(20, GAMMA)).all() else 2
            assert kind == mode
    cnt = np.bincount(modes, minlength=3)
    x = chi2_uniform(cnt)
    print(f"Item_Random over steps 1..600: counts {cnt.tolist()}, chi2 {x:.2f} on 2 dof, bound {chi2_bound(2):.1f}")
    assert cnt.size == 3 and x < chi2_bound(2)


def chi2_2x2(a, b):
    """chi-square (1 dof) of the 2 x 2 table of two boolean samples"""
    t = np.array([[(a & b).sum(), (a & ~b).sum()], [(~a & b).sum(), (~a & ~b).sum()]], np.float64)
    e = t.sum(1, keepdims=True) * t.sum(0, keepdims=True) / t.sum()
    return float(((t - e) ** 2 / e).sum())


def test_streams_of_neighbouring_slots_and_steps_are_uncorrelated():
    s1, sub = crop_starts(50)
    s2, _ = crop_starts(50, STEP + 1)
    lo1, lo2 = s1 < np.median(s1), s2 < np.median(s2)
    x_slot, x_step = chi2_2x2(lo1[:-1], lo1[1:]), chi2_2x2(lo1, lo2)
    print(f"crop starts, slot b against b + 1: chi2 {x_slot:.2f}; step 1 against step 2: chi2 {x_step:.2f}; 1 dof, bound {chi2_bound(1):.1f}")
    assert not (s1 == s2).all() and not (s1[:-1] == s1[1:]).all()
    assert x_slot < chi2_bound(1) and x_step < chi2_bound(1)

