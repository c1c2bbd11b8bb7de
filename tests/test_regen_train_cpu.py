"""CPU tests of the regenerator's pre-training (dr4sr_amd/regen_train.py, the Gumbel mirror of dr4sr_amd/regen_dropout.py): the
schedules against torch's own scheduler and the reference's loop, the noise mirror's index and distribution, the initial state's
distributions, and the argument errors.  Nothing here needs a GPU."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

N_ITEM = 300


# ---------------------------------------------------------------------------------------------------- schedules
def test_learning_rate_is_cosine_annealing_stepped_per_batch():
    """CosineAnnealingLR(T_max = 40) stepped 399 times: the closed form and torch's recursion differ by rounding only (1.1e-16 was
    measured; 1e-12 is asserted); the rate is 0 at s = 40 and 120 and back at 1e-3 at s = 80"""
    from dr4sr_amd.regen_train import lr_at
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=1e-3, betas=(0.9, 0.98), eps=1e-9)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=40)
    want = [opt.param_groups[0]["lr"]]
    for _ in range(399):
        opt.step()
        sched.step()
        want.append(opt.param_groups[0]["lr"])
    got = [lr_at(s, 1e-3, 40) for s in range(400)]
    worst = max(abs(a - b) for a, b in zip(got, want))
    print(f"closed form vs torch's recursion over 400 steps: max |difference| {worst:.2e}")
    assert worst <= 1e-12
    assert got[40] == 0.0 and got[120] == 0.0 and got[0] == 1e-3 and abs(got[80] - 1e-3) <= 1e-18
    assert got[20] == pytest.approx(5e-4, abs=1e-15)


def test_tau_follows_the_reference_loop_to_the_floor():
    from dr4sr_amd.regen_train import tau_at
    tau, want = 1.0, []
    for _ in range(600):
        want.append(tau)
        tau = max(tau * 0.995, 0.1)                  # 2.Pretrain_regenerator.py: after every forward
    assert [tau_at(s) for s in (0, 1, 2, 100, 459, 460, 599)] == [want[s] for s in (0, 1, 2, 100, 459, 460, 599)]
    assert want[459] > 0.1 and want[460] == 0.1 and want[599] == 0.1, "0.995^460 is the first value under the floor"


# ---------------------------------------------------------------------------------------------------- the Gumbel mirror
def test_gumbel_uniform_lies_strictly_inside_the_unit_interval():
    """every 24-bit value, the two ends included: in fp32 the largest one's + 0.5 rounds up to 2^24, u would be 1 and the sample inf"""
    from dr4sr_amd import regen_dropout as rd
    words = np.concatenate([np.array([0, 0xFF, 0x100, 0xFFFFFEFF, 0xFFFFFF00, 0xFFFFFFFF], dtype=np.uint64),
                            np.random.default_rng(0).integers(0, 1 << 32, 100000, dtype=np.uint64)])
    u = rd.gumbel_u(words)
    assert u.dtype == np.float32 and float(u.min()) > 0.0 and float(u.max()) < 1.0
    assert u[0] == np.float32(2.0 ** -25) and u[-1 - 100000] == np.nextafter(np.float32(1), np.float32(0))
    g = rd.gumbel_noise(3, 4, np.arange(4096), 8)
    assert g.dtype == np.float32 and g.shape == (4096, 8) and np.isfinite(g).all()


def test_gumbel_element_depends_on_its_own_index_only():
    from dr4sr_amd import regen_dropout as rd
    pairs = np.array([0, 1, 2, 77, 5000, (1 << 33) + 5], dtype=np.uint64)
    full = rd.gumbel_noise(2024, 3, pairs, 5)
    for i, p in enumerate(pairs):
        assert np.array_equal(rd.gumbel_noise(2024, 3, [p], 5)[0], full[i])
    assert np.array_equal(rd.gumbel_noise(2024, 3, pairs[::-1], 5), full[::-1])
    assert np.array_equal(rd.gumbel_noise(2024, 3, pairs, 3), full[:, :3]), "K does not move an element: the pair stride is 8"
    assert np.array_equal(rd.gumbel_noise(2024, 3, pairs, 8)[:, :5], full)
    for other in (rd.gumbel_noise(2025, 3, pairs, 5), rd.gumbel_noise(2024, 4, pairs, 5)):
        assert not np.array_equal(other, full)
    # against the convention spelled out: element e = pair * 8 + k -> counter (e >> 2 low, e >> 2 high, SITE_GUMBEL, step), word e & 3
    assert rd.SITE_GUMBEL == rd.SITE_BASE + 98 and rd.SITE_GUMBEL not in {v[0] for v in rd.all_sites().values()}
    for p, k in ((77, 0), (77, 3), (77, 4), (5000, 2)):
        e = p * 8 + k
        w = rd.philox4x32_10(np.uint64((e >> 2) & 0xFFFFFFFF), np.uint64((e >> 2) >> 32), np.uint64(rd.SITE_GUMBEL), np.uint64(3), 2024)
        assert int(w[e & 3]) == int(rd.gumbel_words(2024, 3, [p], 5)[0, k])


def test_gumbel_large_pair_indices_reach_the_high_counter_word():
    """the element index passes 2^32 at pair 2^29 and the call index e >> 2 at pair 2^31: from there the counter's high word carries
    the index.  A pair and the pairs that share its low bits must draw other words at each of these sizes"""
    from dr4sr_amd import regen_dropout as rd
    for big in (1 << 29, (1 << 29) + 7, 1 << 31, (1 << 31) + 7, (1 << 33) + 5, (1 << 40) - 1):
        words = rd.gumbel_words(9, 1, [big], 5)[0]
        for cut in (29, 31, 32):
            low = big & ((1 << cut) - 1)
            if low != big:
                assert not np.array_equal(words, rd.gumbel_words(9, 1, [low], 5)[0]), (big, cut)
        for k in (0, 4):
            e = big * 8 + k
            w = rd.philox4x32_10(np.uint64((e >> 2) & 0xFFFFFFFF), np.uint64((e >> 2) >> 32), np.uint64(rd.SITE_GUMBEL), np.uint64(1), 9)
            assert int(w[e & 3]) == int(words[k])
            assert ((e >> 2) >> 32 != 0) == (big >= 1 << 31)


def test_gumbel_moments():
    """10^5 samples: mean within 3 standard errors of Euler's constant, variance within 3 standard errors of pi^2 / 6 (the variance
    estimator's standard error from the fourth central moment of Gumbel(0, 1): kurtosis 5.4)"""
    from dr4sr_amd import regen_dropout as rd
    n = 100000
    g = rd.gumbel_noise(2024, 0, np.arange(n // 5), 5).astype(np.float64).reshape(-1)
    var = math.pi ** 2 / 6
    se_mean = math.sqrt(var / n)
    se_var = var * math.sqrt((5.4 - 1.0) / n)
    print(f"mean {g.mean():.5f} (0.57722, se {se_mean:.5f}), variance {g.var():.5f} ({var:.5f}, se {se_var:.5f})")
    assert abs(g.mean() - 0.5772156649) <= 3 * se_mean
    assert abs(g.var() - var) <= 3 * se_var


# ---------------------------------------------------------------------------------------------------- the initial state
def test_init_state_dict_restates_the_reference_distributions():
    from dr4sr_amd.regen import RegenModel, score_param_names, score_param_shapes
    from dr4sr_amd.regen_train import init_state_dict
    E = torch.randn(N_ITEM, 64, generator=torch.Generator().manual_seed(1))
    sd = init_state_dict(E, K=5, seed=7)
    assert set(sd) == set(score_param_names()) | {"item_embedding_decoder.weight"}
    for name, shape in zip(score_param_names(), score_param_shapes(N_ITEM + 2, 5)):
        assert tuple(sd[name].shape) == shape and sd[name].dtype == torch.float32, name
    assert sd["item_embedding_decoder.weight"] is sd["item_embedding.weight"]
    assert torch.equal(sd["item_embedding.weight"][:N_ITEM], E)
    bound = math.sqrt(6.0 / 256)
    normal, uniform = [], []
    for name in score_param_names():
        t, leaf = sd[name], name.rsplit(".", 1)[-1]
        if name == "item_embedding.weight":
            normal.append(t[N_ITEM:].reshape(-1))
        elif "norm" in name.split(".")[-2]:
            assert torch.equal(t, torch.ones_like(t) if leaf == "weight" else torch.zeros_like(t)), name
        elif leaf == "in_proj_weight":
            assert float(t.abs().max()) <= bound and float(t.abs().max()) > 0.99 * bound, name
            uniform.append(t.reshape(-1))
        elif leaf in ("bias", "in_proj_bias"):
            assert not t.any(), name
        else:                                        # nn.Linear weights (out_proj's included) and position_embedding
            assert abs(float(t.std()) - 0.02) < 0.02 * 4 / math.sqrt(2 * t.numel()) + 1e-4, name
            assert float(t.abs().max()) < 0.02 * 6, name
            normal.append(t.reshape(-1))
    nrm, uni = torch.cat(normal).double(), torch.cat(uniform).double()
    assert len(uniform) == 8                          # 2 + 2 encoder layers, 2 x 2 in the decoder layers
    assert abs(float(nrm.mean())) < 4 * 0.02 / math.sqrt(nrm.numel()) and abs(float(nrm.std()) - 0.02) < 4 * 0.02 / math.sqrt(2 * nrm.numel())
    assert abs(float(uni.mean())) < 4 * bound / math.sqrt(3 * uni.numel())
    assert abs(float(uni.var()) - bound ** 2 / 3) < 4 * (bound ** 2) * math.sqrt(4.0 / 45) / math.sqrt(uni.numel())
    other = init_state_dict(E, K=5, seed=8)
    assert not torch.equal(other["position_embedding.weight"], sd["position_embedding.weight"])
    assert torch.equal(init_state_dict(E, K=5, seed=7)["condition_linear.2.weight"], sd["condition_linear.2.weight"])
    m = RegenModel.from_state_dict(sd, "cpu")
    assert m.has_condition_encoder and m.K == 5 and m.n_item == N_ITEM
    assert RegenModel.from_state_dict(init_state_dict(E, K=3, seed=7), "cpu").K == 3


# ---------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors():
    from dr4sr_amd import _lib, regen_dropout as rd
    from dr4sr_amd.regen import RegenModel, random_state_dict
    from dr4sr_amd.regen_train import RegenTrainer, init_state_dict
    pairs = [[[5, 6, 7], [5, 7]], [[8, 9], [9]]]
    with pytest.raises(ValueError, match="condition_encoder"):
        RegenTrainer(RegenModel.from_state_dict(random_state_dict(N_ITEM, K=5, seed=1), "cpu"), pairs)
    m = RegenModel.from_state_dict(random_state_dict(N_ITEM, K=5, seed=1, condition_encoder=True), "cpu")
    with pytest.raises(ValueError, match="pair 1: a target id is not in its source"):
        RegenTrainer(m, [[[5, 6, 7], [5, 7]], [[8, 9], [10]]])
    with pytest.raises(ValueError, match="K <= 8"):
        RegenTrainer(RegenModel.from_state_dict(random_state_dict(N_ITEM, K=9, seed=1, condition_encoder=True), "cpu"), pairs)
    with pytest.raises(ValueError):
        rd.gumbel_noise(1, 0, [0], 9)
    with pytest.raises(ValueError):
        init_state_dict(torch.zeros(N_ITEM, 64), K=9)
    with pytest.raises(ValueError):
        init_state_dict(torch.zeros(N_ITEM, 32), K=5)
    with pytest.raises(ValueError):
        RegenTrainer(m, pairs, dropout=1.0)
    # the C entry points refuse before anything is launched (host memory stands in for the buffers: it is never touched)
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    fwd = lambda n, K, T, tau, n_tok, pair0: lib.dr4sr_regen_head_fwd(p, None, n, K, T, tau, n_tok, 1, 0, pair0, p, p, p, None, None)
    bwd = lambda n, K, T, tau, n_batch, n_tok, slot: lib.dr4sr_regen_head_bwd(p, p, p, p, n, K, T, tau, 1.0, n_batch, n_tok, p, p, p, slot, None)
    for bad in ((1, 9, 4, 1.0, 4, 0), (1, 0, 4, 1.0, 4, 0), (0, 5, 4, 1.0, 4, 0), (1, 5, 0, 1.0, 4, 0), (1, 5, 51, 1.0, 4, 0), (1, 5, 4, 0.0, 4, 0),
                (1, 5, 4, 1.0, 0, 0), (1, 5, 4, 1.0, 4, -1), (1, 5, 4, 1.0, 4, 1 << 40)):
        assert fwd(*bad) == -1, bad
    for bad in ((1, 9, 4, 1.0, 1, 4, 0), (2, 5, 4, 1.0, 1, 4, 0), (1, 5, 4, 1.0, 1, 0, 0), (1, 5, 4, 1.0, 1, 4, -1), (1, 5, 4, -1.0, 1, 4, 0)):
        assert bwd(*bad) == -1, bad
    assert lib.dr4sr_regen_head_fwd(None, None, 1, 5, 4, 1.0, 4, 1, 0, 0, p, p, p, None, None) == -1
    assert lib.dr4sr_regen_head_bwd(p, p, p, None, 1, 5, 4, 1.0, 1.0, 1, 4, p, p, None, 0, None) == -1, "a loss log needs the NLLs"
