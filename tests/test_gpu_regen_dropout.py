"""Train-mode dropout of the regenerator's HIP scoring and gradients on the MI355X (the DropPhilox instantiations of
csrc/regen_score.hip and csrc/regen_score_bwd.hip through the four *_train entry points): the masks against their host mirror, the
forward and all 98 gradient tensors against the float64 torch restatement under the same masks, and the bit-level promises (batching,
repeats, graph replay, p = 0).

Tolerance unit, as tests/test_gpu_regen_score.py and tests/test_gpu_regen_grad.py: err32 = max |fp32 torch - float64 torch| of the same
quantity on the same rows under the same masks, computed here; bound |HIP - float64| <= 16 x err32.  A factor of 0 or 2 is exact in
every format, so dropout adds no rounding of its own: the unit and the bound are the eval tests'."""
import numpy as np
import pytest
import torch

from test_gpu_regen_score import toys_shaped_pairs
from test_regen_score_cpu import check_close

pytestmark = pytest.mark.gpu

N_ITEM = 300
_cache = {}


def drop(step=3, seed=77, p=0.5):
    from dr4sr_amd.regen import RegenDropout
    return RegenDropout(p, seed, step)


def model(K=5, seed=3, device="cuda", std=0.3):
    from dr4sr_amd.regen import RegenModel, random_state_dict
    key = (K, seed, device, std)
    if key not in _cache:
        _cache[key] = RegenModel.from_state_dict(random_state_dict(N_ITEM, K=K, seed=seed, std=std, condition_encoder=True), device)
    return _cache[key]


def grad_model(K, device="cuda"):
    """std 0.1 (random_state_dict's own default): with the 0.3 of the forward tests the fp32 noise of condition_linear's ReLU inputs (its
    maximum over ~6e5 inputs sets the 16 x band) rejects more than half of the candidate pairs in the torch runs alone, in eval mode too;
    at 0.1 it rejects about one in seven"""
    return model(K, 5, device, 0.1)


def synthetic_pairs(n, seed):
    """toys-shaped pairs (live target tokens straddle several 64-slot tiles; pair 0 has a source of the full width 50, pair 3 a target that
    fills T = 19) plus a source of length 3 with a target of length 3 (SOS, one item, EOS)"""
    pairs = toys_shaped_pairs(n, N_ITEM, seed)
    g = np.random.default_rng(seed + 1000)
    for i in range(10, min(n, 70), 10):              # more sources of the full width, and of length 3: the gradient tests select pairs
        s = g.integers(1, N_ITEM, 48).tolist()
        pairs[i] = [s, [s[p] for p in sorted(g.choice(48, 4, replace=False).tolist())]]
        pairs[i + 5] = [[17 + i], [17 + i]]
    pairs[5] = [[17], [17]]
    assert len(pairs[0][0]) == 48 and len(pairs[3][1]) == 18
    return pairs


def long_pairs(n, seed):
    """the same with one target of 49 items: 51 tokens, T = 50, the longest the position table allows (S = 15 slots per tile window)"""
    pairs = toys_shaped_pairs(n, N_ITEM, seed)
    g = np.random.default_rng(seed + 1000)
    for i in (0, 8, 16):
        s = g.integers(1, N_ITEM, 48).tolist()
        pairs[i] = [s, s + s[:1]]
        pairs[i + 5] = [[23 + i], [23 + i]]
    return pairs


def weights(n_w, n, K, seed):
    return torch.softmax(2 * torch.randn(n_w, n, K, generator=torch.Generator().manual_seed(seed)), -1)


# ---------------------------------------------------------------------------------------------------- the masks
def test_host_mirror_equals_the_device_hook_bit_for_bit():
    """dr4sr_dropout_mask materialises a (seed, step, site) stream from element 0: every site class, two drop probabilities"""
    from dr4sr_amd import _lib, regen_dropout as rd
    lib = _lib.load()
    n = 1 << 16
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    sites = rd.all_sites()
    for name in ("src_emb", "tgt_emb", "enc1.probs", "cond0.ffn_hidden", "dec1.cross_probs", "dec0.ffn_out", "dec1.self_probs"):
        for d in (drop(), drop(9, 1 << 40, 0.3)):
            _lib.check(lib.dr4sr_dropout_mask(_lib.ptr(out), n, d.p, d.seed, d.step, sites[name][0], _lib.cur_stream()), "dr4sr_dropout_mask")
            want = rd.keep_elements(d, sites[name][0], np.arange(n, dtype=np.uint64)) != 0
            assert np.array_equal(out.cpu().numpy() != 0, want), (name, d)


def test_element_indices_beyond_32_bits():
    """pair0 = 600 000: the probability sites' element index has passed 2^32 (at pair 524 288), the hook cannot reach there, so the HIP
    forward is compared with the torch backend at the same pair indices; other indices give other numbers"""
    m = model()
    pairs = synthetic_pairs(48, 21)
    w = weights(2, len(pairs), 5, 1)
    d = drop()
    kw = dict(dropout=d, pair0=600_000)
    hip = m.score(pairs, w, True, None, "hip", **kw)
    r32 = m.score(pairs, w, True, None, "torch", **kw)
    r64 = m.score(pairs, w, True, None, "torch", torch.float64, **kw)
    e = float((r32.nll.double() - r64.nll).abs().max())
    ec = float((r32.cond_logits.double() - r64.cond_logits).abs().max())
    check_close(hip.nll, r64.nll, 16 * e, "HIP vs float64 at pair0 = 600 000", None, e)
    check_close(hip.cond_logits, r64.cond_logits, 16 * ec, "HIP condition logits at pair0 = 600 000", None, ec)
    low = m.score(pairs, w, True, None, "hip", dropout=d, pair0=600_000 - 524_288)      # the same lower 32 bits of the probability indices
    assert float((low.nll - hip.nll).abs().max()) > 1e-3


# ---------------------------------------------------------------------------------------------------- forward
def forward_case(m, pairs, cond, causal, width, what, **kw):
    hip = m.score(pairs, cond, causal, width, "hip", **kw)
    r32 = m.score(pairs, cond, causal, width, "torch", **kw)
    r64 = m.score(pairs, cond, causal, width, "torch", torch.float64, **kw)
    assert torch.isfinite(r64.nll).all() and torch.equal(hip.nll == 0, r64.nll == 0)
    e = float((r32.nll.double() - r64.nll).abs().max())
    ec = float((r32.cond_logits.double() - r64.cond_logits).abs().max())
    d = check_close(hip.nll, r64.nll, 16 * e, f"train-mode NLL, HIP vs float64, {what}", None, e)
    dc = check_close(hip.cond_logits, r64.cond_logits, 16 * ec, f"train-mode condition logits, {what}", None, ec)
    print(f"{what}: |HIP - float64| / err32: NLL {d / e:.2f}, condition logits {dc / ec:.2f}")
    return hip, r64


@pytest.mark.parametrize("K,n_w,causal", [(5, 2, True), (5, 1, False), (3, 2, False), (3, 1, True)])
def test_train_mode_forward_matches_float64(K, n_w, causal):
    m = model(K)
    pairs = synthetic_pairs(300, 7)
    hip, r64 = forward_case(m, pairs, weights(n_w, len(pairs), K, 2), causal, None, f"300 pairs, K={K}, n_w={n_w}, causal={causal}", dropout=drop())
    ev = m.score(pairs[:40], "encoder", causal, None, "hip")
    tr = m.score(pairs[:40], "encoder", causal, None, "hip", dropout=drop())
    assert float((ev.nll - tr.nll).abs().max()) > 1e-2 and float((ev.cond_logits - tr.cond_logits).abs().max()) > 1e-3
    if K == 5 and n_w == 2:
        forward_case(m, pairs, "encoder", causal, None, "300 pairs, the encoder's own weights", dropout=drop(4))
        forward_case(m, long_pairs(24, 9), "encoder", causal, None, "24 pairs with a target of 51 tokens (T = 50)", dropout=drop(5))


def test_train_mode_forward_on_the_fixture_pairs():
    from dr4sr_amd.regen import RegenModel
    from test_regen_dropout_cpu import load_train_fixture
    z, sd, pairs, _, width, d = load_train_fixture()
    m = RegenModel.from_state_dict(sd, "cuda")
    forward_case(m, pairs, "encoder", True, width, "the fixture's 256 pairs, causal", dropout=d)
    forward_case(m, pairs, "all", False, width, "the fixture's 256 pairs, all conditions, bidirectional", dropout=d)


# ---------------------------------------------------------------------------------------------------- gradients
def relu_inputs(m, src, tgt, tgt_len, w, dt, td, causal):
    """the inputs of both ReLUs (condition_linear[0]: [n, Ls, 64 K]; condition_layer[0]: [n, 64]) of the eager restatement at dtype dt"""
    import torch.nn.functional as F
    from dr4sr_amd import regen_torch
    p = m._params_as(dt, src.device)
    names = {id(p["condition_linear.0.weight"]): "mem", id(p["condition_encoder.condition_layer.0.weight"]): "cond"}
    cap, orig = {}, F.linear

    def lin(x, wt, b=None):
        y = orig(x, wt, b)
        if id(wt) in names:
            cap[names[id(wt)]] = y.detach()
        return y

    F.linear = lin
    try:
        regen_torch.score_forward(m, src, tgt, tgt_len, w.to(dt), True, causal, dt, None, td)
    finally:
        F.linear = orig
    return cap["mem"], cap["cond"]


def select_pairs(m, cand, n_keep, d, seed, causal):
    """tests/test_gpu_regen_grad.py's selection, restated for train mode: decided from the float64 and fp32 torch runs ALONE (under the
    masks of the candidates' own indices), a candidate is kept when every input of either ReLU at its live positions is farther from zero
    than 16 x the fp32 noise of that activation (max |fp32 - float64| over all live inputs).  The first n_keep kept INDICES are the case;
    len(cand) = 2 n_keep, so at most half may be dropped, the share the existing test allows.  The masks follow the pair index (a
    source's position 0 sees only SOS and its own masks, so an index can be near a ReLU step whatever pair sits there): the kept pairs are
    used at their candidate indices."""
    from dr4sr_amd.regen_torch import TorchDrop
    n, dev = len(cand), m.device
    w = weights(1, n, m.K, seed).to(dev)
    src, src_len, tgt, tgt_len, Ls, T = m._pack_pairs(cand, None)
    src, src_len, tgt, tgt_len = (t.to(dev) for t in (src, src_len, tgt, tgt_len))
    pre = {dt: relu_inputs(m, src, tgt, tgt_len, w, dt, TorchDrop.of(d, 0, n, dt, dev), causal) for dt in (torch.float32, torch.float64)}
    live = (torch.arange(Ls, device=dev)[None, :] < src_len[:, None])[:, :, None].expand_as(pre[torch.float64][0])
    noise_m = float((pre[torch.float32][0].double() - pre[torch.float64][0])[live].abs().max())
    noise_c = float((pre[torch.float32][1].double() - pre[torch.float64][1]).abs().max())
    near = ((pre[torch.float64][0].abs() <= 16 * noise_m) & live).flatten(1).any(1) | (pre[torch.float64][1].abs() <= 16 * noise_c).any(1)
    keep = [i for i in range(n) if not bool(near[i])]
    print(f"fp32 noise of the ReLU inputs {noise_m:.2e} / {noise_c:.2e}; {int(near.sum())} of {n} candidates have an input within 16 x of zero")
    assert len(cand) == 2 * n_keep and len(keep) >= n_keep, "the selection may drop at most half of the candidates"
    return keep[:n_keep]


def grad_case(m, cand, n_keep, cond, causal, d, what, **kw):
    """loss_and_grad of the selected pairs on the three sides (HIP, fp32 torch, float64 torch).  The kept indices fall into runs of
    consecutive candidates; each run is one call with pair0 = its first index, at the candidates' width, so every pair keeps the masks the
    selection saw.  A call normalises by its own token count, so the runs are weighed back by it and summed in float64, on the three sides
    alike: the compared quantity is the gradient of one scalar, sum over runs of (the run's summed NLL + its tokens x its entropy term)."""
    keep = select_pairs(m, cand, n_keep, d, 5, causal)
    lens = {len(cand[i][0]) for i in keep}
    assert 48 in lens and 1 in lens, "a full-width source and a length-3 source must survive the selection"
    runs, a = [], 0
    while a < len(keep):
        b = a
        while b + 1 < len(keep) and keep[b + 1] == keep[b] + 1:
            b += 1
        runs.append((keep[a], keep[b] + 1))
        a = b + 1
    width = m._pack_pairs(cand, None)[4:]
    total = {}
    for side, (backend, dt) in {"hip": ("hip", torch.float32), "r32": ("torch", torch.float32), "r64": ("torch", torch.float64)}.items():
        acc = dict(loss=0.0, grads=None, dw=[])
        for lo, hi in runs:
            kw_run = {k: (v[lo:hi] if k == "noise" else v) for k, v in kw.items()}
            r = m.loss_and_grad(cand[lo:hi], cond if isinstance(cond, str) else cond[:, lo:hi], causal, width, backend, dt, dropout=d, pair0=lo,
                                **kw_run)
            n_tok = float(sum(len(t) + 1 for _, t in cand[lo:hi]))
            if acc["grads"] is None:
                acc["grads"] = {k: torch.zeros_like(v, dtype=torch.float64) for k, v in r.grads.items()}
            acc["loss"] += float(r.loss) * n_tok
            for k, v in r.grads.items():
                acc["grads"][k] += v.double() * n_tok
            acc["dw"].append(r.dw.double() * n_tok)
        total[side] = acc
    bad, worst, worst_k = [], 0.0, None
    items = [(k, total["hip"]["grads"][k], total["r32"]["grads"][k], total["r64"]["grads"][k]) for k in total["r64"]["grads"]]
    items.append(("dw", torch.cat(total["hip"]["dw"], 1), torch.cat(total["r32"]["dw"], 1), torch.cat(total["r64"]["dw"], 1)))
    assert len(items) == 99
    for k, h, r32, r64 in items:
        e = float((r32 - r64).abs().max())
        dd = float((h.to(r64.device) - r64).abs().max())
        ratio = dd / e if e > 0 else (0.0 if dd == 0 else float("inf"))
        if ratio > worst:
            worst, worst_k = ratio, k
        if dd > 16 * e:
            bad.append(f"{k}: |HIP - float64| {dd:.3e}, err32 {e:.3e}, ratio {ratio:.1f}")
    print(f"{what}: {len(runs)} runs, worst |HIP - float64| / err32_t over 98 tensors and dw: {worst:.2f} ({worst_k})")
    assert not bad, f"{what}:\n" + "\n".join(bad)
    # the scalar: one |fp32 - float64| sample of a sum of thousands of terms can cancel to far below an fp32 ulp of the value, which no
    # fp32 NLL can beat; the unit is the larger of the two, as tests/test_gpu_regen_grad.py takes it for the fixture's loss
    e = max(abs(total["r32"]["loss"] - total["r64"]["loss"]), 6e-8 * abs(total["r64"]["loss"]))
    print(f"{what}: summed loss {total['r64']['loss']:.6f}, |HIP - float64| {abs(total['hip']['loss'] - total['r64']['loss']):.3e}, unit {e:.3e}")
    assert abs(total["hip"]["loss"] - total["r64"]["loss"]) <= 16 * e
    return keep


@pytest.mark.parametrize("K,causal", [(5, True), (3, False)])
def test_train_mode_gradients_match_float64_per_tensor(K, causal):
    m = grad_model(K)
    pool = synthetic_pairs(400, 11)
    w = weights(2, len(pool), K, 3)
    grad_case(m, pool, 200, w, causal, drop(6), f"200 pairs, [2, n, {K}] weights, causal={causal}")
    g = torch.Generator().manual_seed(1)
    noise = -torch.log(-torch.log(torch.rand(len(pool), K, generator=g).clamp_min(1e-9)))
    grad_case(m, pool, 200, "encoder", causal, drop(7), f"200 pairs, encoder + noise, entropy 1, K={K}, causal={causal}",
              noise=noise, tau=0.7, entropy_weight=1.0)


def test_train_mode_gradients_with_the_longest_target():
    m = grad_model(5)
    cand = long_pairs(48, 13)
    keep = grad_case(m, cand, 24, "encoder", True, drop(8), "24 pairs with a target of 51 tokens (T = 50), encoder", entropy_weight=1.0)
    assert any(len(cand[i][1]) == 49 for i in keep), "a target of the longest length must survive the selection"


def test_hip_matches_the_reference_train_mode_gradients_of_the_fixture():
    """HIP against loss.backward() of the reference's Generator in model.train() under the same masks (tests/golden/regen_train_toys.npz):
    all 98 tensors within 16 x the stored err32_t = max |reference fp32 - reference float64|, the two loss terms against the recorded ones"""
    from dr4sr_amd.regen import RegenModel, score_param_names
    from test_regen_dropout_cpu import load_train_fixture
    z, sd, pairs, err32, width, d = load_train_fixture()
    m = RegenModel.from_state_dict(sd, "cuda")
    hip = m.loss_and_grad(pairs, "encoder", True, width, "hip", noise=torch.from_numpy(z["noise"]), tau=1.0, entropy_weight=1.0, dropout=d)
    bad, worst = [], 0.0
    for k in score_param_names():
        dd = float((hip.grads[k].cpu().double() - torch.from_numpy(z[f"g:{k}"]).double()).abs().max())
        worst = max(worst, dd / err32[k]) if err32[k] > 0 else worst
        if dd > 16 * err32[k]:
            bad.append(f"{k}: |HIP - reference| {dd:.3e} > 16 x err32 {err32[k]:.3e}")
    print(f"HIP vs the reference's train-mode gradients: worst ratio to err32_t over 98 tensors: {worst:.2f}")
    assert not bad, "\n".join(bad)
    e_loss = abs(float(z["loss"]) - float(z["loss64"]))
    assert abs(float(hip.loss) - float(z["loss64"])) <= 16 * max(e_loss, 6e-8 * float(z["loss64"]))
    assert abs(float(hip.entropy) - float(z["reg_loss64"])) <= 16 * 6e-8 * 2


# ---------------------------------------------------------------------------------------------------- bits
def device_inputs(m, pairs, n_w, seed):
    src, src_len, tgt, tgt_len, Ls, T = m._pack_pairs(pairs, None)
    dev = [t.cuda().contiguous() for t in (src, src_len, tgt, tgt_len)]
    g = torch.Generator().manual_seed(seed)
    w = torch.softmax(torch.randn(n_w, len(pairs), m.K, generator=g), -1).cuda().contiguous()
    dnll = torch.rand(n_w, len(pairs), T, generator=g).cuda().contiguous()
    return dev, w, dnll


def test_a_pair_scores_and_differentiates_the_same_alone_and_in_the_batch():
    m = model(5, seed=6)
    pairs = synthetic_pairs(300, 15)
    d = drop(9)
    big = m.score(pairs, "all", True, None, "hip", dropout=d)
    again = m.score(pairs, "all", True, None, "hip", dropout=d)
    assert torch.equal(big.nll, again.nll) and torch.equal(big.cond_logits, again.cond_logits)
    for i in (0, 3, 5, 150, 299):
        one = m.score([pairs[i]], "all", True, big.width, "hip", dropout=d, pair0=i)
        assert torch.equal(one.nll[:, 0], big.nll[:, i]) and torch.equal(one.cond_logits[0], big.cond_logits[i]), i
    cut = m.score(pairs[100:200], "all", True, big.width, "hip", dropout=d, pair0=100)
    assert torch.equal(cut.nll, big.nll[:, 100:200]) and torch.equal(cut.cond_logits, big.cond_logits[100:200])
    other = m.score(pairs[:40], "all", True, big.width, "hip", dropout=drop(10))
    assert float((other.nll - big.nll[:, :40]).abs().max()) > 1e-2, "another step must give other NLLs"
    # the backward: dw and the NLLs are per pair, the same bits alone (pair0 = i) and in the batch; the same call twice, the same bits
    dev, w, dnll = device_inputs(m, pairs, 2, 3)
    g_a, dw_a, nll_a = m.score_bwd_device(*dev, w, dnll, dropout=d)
    g_a, dw_a, nll_a = g_a.clone(), dw_a.clone(), nll_a.clone()
    g_b, dw_b, nll_b = m.score_bwd_device(*dev, w, dnll, dropout=d)
    assert torch.equal(g_a, g_b) and torch.equal(dw_a, dw_b) and torch.equal(nll_a, nll_b)
    assert torch.equal(nll_a, m.score_device(*dev, w, True, dropout=d)), "the backward's NLLs are the train-mode forward's"
    for i in (0, 5, 299):
        one = [t[i:i + 1].contiguous() for t in dev]
        _, dw_1, nll_1 = m.score_bwd_device(*one, w[:, i:i + 1].contiguous(), dnll[:, i:i + 1].contiguous(), dropout=d, pair0=i)
        assert torch.equal(dw_1[:, 0], dw_a[:, i]) and torch.equal(nll_1[:, 0], nll_a[:, i]), i


def test_p_zero_and_no_dropout_are_the_eval_bits():
    m = model(5, seed=6)
    pairs = synthetic_pairs(200, 17)
    ev = m.score(pairs, "encoder", False, None, "hip")
    for d in (None, drop(p=0.0)):
        got = m.score(pairs, "encoder", False, None, "hip", dropout=d, pair0=11)
        assert torch.equal(got.nll, ev.nll) and torch.equal(got.cond_logits, ev.cond_logits)
    dev, w, dnll = device_inputs(m, pairs, 2, 4)
    dl = torch.randn(len(pairs), 5, generator=torch.Generator().manual_seed(4)).cuda().contiguous()
    g0, dw0, nll0 = (t.clone() for t in m.score_bwd_device(*dev, w, dnll))
    c0 = m.condition_bwd_device(dev[2], dev[3], dl).clone()
    for d in (None, drop(p=0.0)):
        g1, dw1, nll1 = m.score_bwd_device(*dev, w, dnll, dropout=d, pair0=11)
        assert torch.equal(g1, g0) and torch.equal(dw1, dw0) and torch.equal(nll1, nll0)
        assert torch.equal(m.condition_bwd_device(dev[2], dev[3], dl, dropout=d, pair0=11), c0)
    tr = m.score_bwd_device(*dev, w, dnll, dropout=drop())[0]
    assert float((tr - g0).abs().max()) > 1e-3


def test_graph_replay_of_the_train_mode_backwards_equals_the_eager_bits():
    m = model(5, seed=6)
    pairs = synthetic_pairs(200, 13)
    dev, w, dnll = device_inputs(m, pairs, 3, 4)
    dl = torch.randn(len(pairs), 5, generator=torch.Generator().manual_seed(4)).cuda().contiguous()
    d = drop(11)

    def both():
        g, dw, nll = m.score_bwd_device(*dev, w, dnll, dropout=d, pair0=40)
        m.condition_bwd_device(dev[2], dev[3], dl, g, accumulate=True, dropout=d, pair0=40)
        return g, dw, nll

    eager = [t.clone() for t in both()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = both()
    for _ in range(2):
        for t in out:
            t.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(o, e) for o, e in zip(out, eager))
