"""Gradients of the regenerator's teacher-forced loss on the MI355X (csrc/regen_score_bwd.hip through dr4sr_regen_score_bwd and
dr4sr_regen_score_condition_bwd, RegenModel.loss_and_grad / condition_grad): every one of the 98 gradient tensors, dw and the loss
against float64 autograd, exact repeats, NaN-prefilled buffers, accumulation, graph capture, the forward paths left as they were, and
twenty Adam steps through load_params.

Tolerance unit: per tensor, err32_t = max |fp32 torch autograd - float64 autograd| on the same rows, computed here.  Bound:
|HIP - float64| <= 16 x err32_t, the project's bound for the forward.  A tensor whose gradient is mathematically zero has
err32_t = 0 and must be exactly zero.  Two half-batches accumulated against the full batch: 2 x err32_t (order-dependent, not
bitwise).  Measured worst ratios: DESIGN.md 4j."""
import numpy as np
import pytest
import torch

from test_gpu_regen_score import toys_shaped_pairs

pytestmark = pytest.mark.gpu


def model(n_item=None, seed=3):
    from dr4sr_amd.regen import NUM_ITEM, RegenModel, random_state_dict
    sd = random_state_dict(n_item or NUM_ITEM["toy"], seed=seed, std=0.3, condition_encoder=True)
    return RegenModel.from_state_dict(sd, "cuda"), RegenModel.from_state_dict(sd, "cpu")


def compare(m, hip_flat, g32, g64, factor, what):
    from dr4sr_amd.regen import score_param_names
    hip = m.grads_from_flat(hip_flat)
    assert len(hip) == 98 == len(score_param_names())
    worst, seen = 0.0, 0
    for k in score_param_names():
        want = g64[k] if k in g64 else torch.zeros(m.p[k].shape, dtype=torch.float64)
        got32 = g32[k] if k in g32 else torch.zeros(m.p[k].shape)
        e = float((got32.double() - want).abs().max())
        d = float((hip[k].cpu().double() - want).abs().max())
        assert d <= factor * e, f"{what}: {k}: |HIP - float64| {d:.3e} > {factor} x err32 {e:.3e}"
        if e > 0:
            worst = max(worst, d / e)
        seen += 1
    assert seen == 98
    print(f"{what}: worst |HIP - float64| / err32_t over 98 tensors: {worst:.2f}")
    return worst


def packed(m, pairs):
    _, _, tgt, tgt_len, _, T = m._pack_pairs(pairs, None)
    return tgt.cuda().contiguous(), tgt_len.cuda().contiguous()


def test_condition_backward_matches_float64_per_tensor():
    m, cpu = model()
    pairs = toys_shaped_pairs(2000, m.n_item, 7)
    dl = torch.randn(len(pairs), 5, generator=torch.Generator().manual_seed(1))
    g64 = cpu.condition_grad(pairs, dl.double(), backend="torch", dtype=torch.float64)
    g32 = cpu.condition_grad(pairs, dl, backend="torch", dtype=torch.float32)
    assert float(g64["item_embedding.weight"][0].abs().max()) == 0      # PAD is never looked up by the condition encoder
    tgt, tgt_len = packed(m, pairs)
    flat = m.condition_bwd_device(tgt, tgt_len, dl.cuda().contiguous())
    compare(m, flat, g32, g64, 16, "2 000 toys-shaped pairs, one call")
    via = m.condition_grad(pairs, dl, backend="hip")                    # the public form, chunked with accumulate
    assert len(via) == 30
    compare(m, torch.cat([(via[k] if k in via else torch.zeros_like(v)).reshape(-1) for k, v in m.p.items()]),
            g32, g64, 16, "2 000 toys-shaped pairs, condition_grad (2 chunks)")


def test_a_batch_of_5000_through_the_chunked_accumulate_path():
    m, cpu = model(seed=4)
    pairs = toys_shaped_pairs(5000, m.n_item, 9)
    dl = torch.randn(len(pairs), 5, generator=torch.Generator().manual_seed(2))
    g64 = cpu.condition_grad(pairs, dl.double(), backend="torch", dtype=torch.float64)
    g32 = cpu.condition_grad(pairs, dl, backend="torch", dtype=torch.float32)
    via = m.condition_grad(pairs, dl, backend="hip")
    compare(m, torch.cat([(via[k] if k in via else torch.zeros_like(v)).reshape(-1) for k, v in m.p.items()]),
            g32, g64, 16, "5 000 toys-shaped pairs, 5 chunks")


def test_exact_repeats_nan_prefill_and_half_batches():
    m, cpu = model(seed=5)
    pairs = toys_shaped_pairs(1000, m.n_item, 11)
    dl = torch.randn(len(pairs), 5, generator=torch.Generator().manual_seed(3))
    tgt, tgt_len = packed(m, pairs)
    dl_d = dl.cuda().contiguous()
    a = m.condition_bwd_device(tgt, tgt_len, dl_d).clone()
    b = m.condition_bwd_device(tgt, tgt_len, dl_d)
    assert torch.equal(a, b), "the same call twice must give the same bits"
    nan = torch.full_like(a, float("nan"))
    c = m.condition_bwd_device(tgt, tgt_len, dl_d, nan, accumulate=False)
    assert c.data_ptr() == nan.data_ptr() and not torch.isnan(c).any() and torch.equal(c, a)
    half = m.condition_bwd_device(tgt[:500].contiguous(), tgt_len[:500].contiguous(), dl_d[:500].contiguous())
    half = m.condition_bwd_device(tgt[500:].contiguous(), tgt_len[500:].contiguous(), dl_d[500:].contiguous(), half, accumulate=True)
    g64 = cpu.condition_grad(pairs, dl.double(), backend="torch", dtype=torch.float64)
    g32 = cpu.condition_grad(pairs, dl, backend="torch", dtype=torch.float32)
    ha, hh = m.grads_from_flat(a), m.grads_from_flat(half)
    for k in ha:                                                        # order-dependent, so not bitwise
        e = float((g32[k].double() - g64[k]).abs().max()) if k in g64 else 0.0
        d = float((ha[k] - hh[k]).abs().max())
        assert d <= 2 * e, f"{k}: two half-batches accumulated differ from the full batch by {d:.3e} > 2 x err32 {e:.3e}"
    twice = m.condition_bwd_device(tgt, tgt_len, dl_d, a.clone(), accumulate=True)
    assert torch.equal(twice, a + a)                                    # x + x is exact


def test_graph_capture_replays_the_eager_bits():
    m, _ = model(300, seed=6)
    pairs = toys_shaped_pairs(600, m.n_item, 13)
    tgt, tgt_len = packed(m, pairs)
    dl = torch.randn(len(pairs), 5, generator=torch.Generator().manual_seed(4)).cuda().contiguous()
    eager = m.condition_bwd_device(tgt, tgt_len, dl).clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.condition_bwd_device(tgt, tgt_len, dl)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m.condition_bwd_device(tgt, tgt_len, dl)
    for _ in range(2):
        out.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_score_and_decode_are_unchanged_after_a_backward():
    m, _ = model(seed=7)
    pairs = toys_shaped_pairs(300, m.n_item, 15)
    srcs = [[m.sos] + s + [m.eos] for s, _ in pairs[:40]]
    before = m.score(pairs, "encoder", True, None, "hip")
    dec = m.decode(srcs, 0, 2, "hip")
    flat0, sflat0 = m.flat().clone(), m.score_flat().clone()
    m.condition_grad(pairs, torch.ones(len(pairs), 5), backend="hip")
    after = m.score(pairs, "encoder", True, None, "hip")
    assert torch.equal(before.nll, after.nll) and torch.equal(before.cond_logits, after.cond_logits)
    assert m.decode(srcs, 0, 2, "hip") == dec
    assert torch.equal(m.flat(), flat0) and torch.equal(m.score_flat(), sflat0)


def test_gradient_steps_through_load_params_lower_the_objective():
    """the public use end to end: maximise sum(cond_logits * dlogits) for a fixed dlogits with the reference's Adam settings on
    the condition encoder's HIP gradients, load_params after every step, the HIP forward afterwards sees the new parameters"""
    m, _ = model(300, seed=8)
    pairs = toys_shaped_pairs(256, m.n_item, 17)
    dl = torch.randn(len(pairs), 5, generator=torch.Generator().manual_seed(5))
    objective = lambda: float((m.score(pairs, "encoder", True, None, "hip").cond_logits.double() * dl.double()).sum())
    start = objective()
    names = [k for k in m.p if k.startswith("condition_encoder.")]
    params = [m.p[k].clone().requires_grad_(True) for k in names]
    opt = torch.optim.Adam(params, lr=1e-3, betas=(0.9, 0.98), eps=1e-9)
    addr = m.score_flat().data_ptr()
    for _ in range(20):
        g = m.condition_grad(pairs, dl, backend="hip")
        for p, k in zip(params, names):
            p.grad = g[k].clone()
        opt.step()
        m.load_params({k: p.detach() for p, k in zip(params, names)})
    assert m.score_flat().data_ptr() == addr
    end = objective()
    print(f"sum(cond_logits * dlogits): {start:.4f} -> {end:.4f} after 20 Adam steps")
    assert end < start


# ---------------------------------------------------------------------------------------------------- the whole loss: loss_and_grad
def compare_result(hip, r32, r64, factor, what):
    """every tensor of grads, dw and the loss of a HIP GradResult against float64, in units of the fp32 autograd's own error"""
    assert sorted(hip.grads) == sorted(r64.grads) and len(hip.grads) == 98
    bad, worst, worst_k = [], 0.0, None
    items = [(k, hip.grads[k], r32.grads[k], r64.grads[k]) for k in r64.grads] + [("dw", hip.dw, r32.dw, r64.dw)]
    for k, h, a, b in items:
        e = float((a.double() - b).abs().max())
        d = float((h.double() - b.to(h.device)).abs().max())
        ratio = d / e if e > 0 else (0.0 if d == 0 else float("inf"))
        if ratio > worst:
            worst, worst_k = ratio, k
        if d > factor * e:
            bad.append(f"{k}: |HIP - float64| {d:.3e}, err32 {e:.3e}, ratio {ratio:.1f}")
    print(f"{what}: worst |HIP - float64| / err32_t over 98 tensors and dw: {worst:.2f} ({worst_k})")
    assert not bad, f"{what}:\n" + "\n".join(bad)
    e = abs(float(r32.loss) - float(r64.loss))
    assert abs(float(hip.loss) - float(r64.loss)) <= 16 * e, (float(hip.loss), float(r64.loss), e)
    return worst


def three(m, pairs, cond, causal, **kw):
    hip = m.loss_and_grad(pairs, cond, causal, None, "hip", **kw)
    r32 = m.loss_and_grad(pairs, cond, causal, None, "torch", torch.float32, **kw)
    r64 = m.loss_and_grad(pairs, cond, causal, None, "torch", torch.float64, **kw)
    return hip, r32, r64


@pytest.mark.parametrize("causal", [True, False])
def test_loss_and_grad_matches_float64_per_tensor(causal):
    m, _ = model()
    pairs = toys_shaped_pairs(2000, m.n_item, 7)
    g = torch.Generator().manual_seed(1)
    mixed = torch.softmax(2 * torch.randn(2, len(pairs), 5, generator=g), -1)
    hip, r32, r64 = three(m, pairs, mixed, causal)
    compare_result(hip, r32, r64, 16, f"2 000 pairs, [2, n, 5] weights, causal={causal}")
    assert float(r64.grads["item_embedding.weight"][0].abs().max()) > 0      # PAD row 0: through the logits of padded source rows
    assert all(float(hip.grads[k].abs().max()) == 0 for k in hip.grads if k.startswith("condition_encoder."))
    noise = -torch.log(-torch.log(torch.rand(len(pairs), 5, generator=g).clamp_min(1e-9)))
    hip, r32, r64 = three(m, pairs, "encoder", causal, noise=noise, tau=0.7, entropy_weight=1.0)
    compare_result(hip, r32, r64, 16, f"2 000 pairs, encoder + noise, tau 0.7, entropy 1, causal={causal}")
    assert abs(float(hip.entropy) - float(r64.entropy)) < 1e-5
    e = float((r32.cond_logits.double() - r64.cond_logits).abs().max())
    assert float((hip.cond_logits.double() - r64.cond_logits).abs().max()) <= 16 * e


def test_loss_and_grad_of_5000_pairs_through_the_chunks():
    m, _ = model(seed=4)
    pairs = toys_shaped_pairs(5000, m.n_item, 9)
    mixed = torch.softmax(2 * torch.randn(2, len(pairs), 5, generator=torch.Generator().manual_seed(2)), -1)
    hip, r32, r64 = three(m, pairs, mixed, True)
    compare_result(hip, r32, r64, 16, "5 000 pairs, 20 chunks accumulated")


def score_inputs(m, pairs, n_w, seed):
    src, src_len, tgt, tgt_len, Ls, T = m._pack_pairs(pairs, None)
    dev = [t.cuda().contiguous() for t in (src, src_len, tgt, tgt_len)]
    g = torch.Generator().manual_seed(seed)
    w = torch.softmax(torch.randn(n_w, len(pairs), 5, generator=g), -1).cuda().contiguous()
    dnll = torch.rand(n_w, len(pairs), T, generator=g).cuda().contiguous()
    return dev, w, dnll


def autograd_of_weighted_nll(m, dev, w, dnll):
    """{dtype: {name: gradient}} of sum(nll * dnll) through the eager restatement in fp32 and float64"""
    from dr4sr_amd import regen_torch
    unit = {}
    for dt in (torch.float32, torch.float64):
        leaves = {k: v.to(dt).clone().requires_grad_(True) for k, v in m.p.items()}
        nll, _ = regen_torch.score_forward(m, dev[0], dev[2], dev[3], w.to(dt), False, True, dt, leaves)
        (nll * dnll.to(dt)).sum().backward()
        unit[dt] = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    return unit


def test_score_bwd_exact_repeats_nan_prefill_and_half_batches():
    m, _ = model(seed=5)
    pairs = toys_shaped_pairs(200, m.n_item, 11)
    dev, w, dnll = score_inputs(m, pairs, 2, 3)
    a, dw_a, nll_a = m.score_bwd_device(*dev, w, dnll)
    a, dw_a = a.clone(), dw_a.clone()
    b, dw_b, nll_b = m.score_bwd_device(*dev, w, dnll)
    assert torch.equal(a, b) and torch.equal(dw_a, dw_b), "the same call twice must give the same bits"
    assert torch.equal(nll_a, m.score_device(*dev, w, True)), "the backward's NLLs are the forward's"
    nan = torch.full_like(a, float("nan"))
    c, _, _ = m.score_bwd_device(*dev, w, dnll, True, nan, accumulate=False)
    assert c.data_ptr() == nan.data_ptr() and not torch.isnan(c).any() and torch.equal(c, a)
    cut = lambda lo, hi: ([t[lo:hi].contiguous() for t in dev], w[:, lo:hi].contiguous(), dnll[:, lo:hi].contiguous())
    d0, w0, n0 = cut(0, 100)
    d1, w1, n1 = cut(100, 200)
    half, dw0, _ = m.score_bwd_device(*d0, w0, n0)
    half, dw1, _ = m.score_bwd_device(*d1, w1, n1, True, half, accumulate=True)
    assert torch.equal(torch.cat([dw0, dw1], 1), dw_a), "dw is per pair: the same bits in any batch"
    # the unit for the order-dependent sum: fp32 against float64 autograd of the same scalar sum(nll * dnll)
    unit = autograd_of_weighted_nll(m, dev, w, dnll)
    ha, hh = m.grads_from_flat(a), m.grads_from_flat(half)
    for k in ha:
        e = float((unit[torch.float32][k].double() - unit[torch.float64][k]).abs().max())
        d = float((ha[k] - hh[k]).abs().max())
        assert d <= 2 * e, f"{k}: two half-batches accumulated differ from the full batch by {d:.3e} > 2 x err32 {e:.3e}"


def test_a_random_upstream_gradient_matches_float64_per_tensor():
    """score_bwd_device with a random dnll in [0, 1) per token (not the loss's uniform 1 / n_tok), 200 pairs, 2 weight vectors:
    every tensor within 16 x err32_t of float64 autograd of sum(nll * dnll).

    The gradient of a ReLU network is not defined where a ReLU input is zero, and an input within fp32 rounding of zero takes either
    branch depending on the rounding of the forward that feeds it; a comparison across two branches measures the step of the ReLU,
    not the arithmetic (measured on the MI355X: one input of condition_linear's ReLU at -2.68e-6 in float64 among 792 960 put
    condition_linear.0.bias 205 x err32_t away, every decoder tensor staying below 2).  So the pairs are chosen where the gradient is
    defined to fp32: from 400 candidates, decided from the float64 and fp32 torch runs ALONE, a pair is kept when every input of
    that ReLU at its live source positions is farther from zero than 16 x the fp32 noise of the activation (max |fp32 - float64| over
    all its live inputs; 16 x is the bound the project puts on the HIP forward).  The first 200 kept pairs are the case."""
    m, _ = model(seed=5)
    cand = toys_shaped_pairs(400, m.n_item, 11)
    dev, w, _ = score_inputs(m, cand, 2, 3)
    src_len = dev[1]
    pre = {dt: relu_inputs(m, dev, w, dt) for dt in (torch.float32, torch.float64)}
    Ls = dev[0].shape[1]
    live = (torch.arange(Ls, device="cuda")[None, :] < src_len[:, None])[:, :, None].expand_as(pre[torch.float64])
    noise = float((pre[torch.float32].double() - pre[torch.float64])[live].abs().max())
    near = ((pre[torch.float64].abs() <= 16 * noise) & live).flatten(1).any(1)
    keep = [i for i in range(len(cand)) if not bool(near[i])][:200]
    print(f"fp32 noise of the ReLU inputs {noise:.2e}; {int(near.sum())} of {len(cand)} candidate pairs have an input within 16 x of zero")
    assert len(keep) == 200
    pairs = [cand[i] for i in keep]
    dev, w, dnll = score_inputs(m, pairs, 2, 3)
    a, _, _ = m.score_bwd_device(*dev, w, dnll)
    unit = autograd_of_weighted_nll(m, dev, w, dnll)
    ha = m.grads_from_flat(a)
    bad, worst, seen = [], 0.0, 0
    for k in ha:
        e = float((unit[torch.float32][k].double() - unit[torch.float64][k]).abs().max())
        d = float((ha[k].double() - unit[torch.float64][k]).abs().max())
        seen += 1
        if e > 0:
            worst = max(worst, d / e)
        if d > 16 * e:
            bad.append(f"{k}: |HIP - float64| {d:.3e}, err32 {e:.3e}")
    print(f"random upstream gradient, 200 pairs: worst |HIP - float64| / err32_t: {worst:.2f}")
    assert seen == 98 and not bad, "\n".join(bad)


def relu_inputs(m, dev, w, dt):
    """the inputs of condition_linear's ReLU [n, Ls, 320] in the eager restatement at dtype dt"""
    import torch.nn.functional as F
    from dr4sr_amd import regen_torch
    src, _, tgt, tgt_len = dev
    p = m._params_as(dt, src.device)
    cap, orig = {}, F.linear

    def lin(x, wt, b=None):
        y = orig(x, wt, b)
        if wt is p["condition_linear.0.weight"]:
            cap["y"] = y.detach()
        return y

    F.linear = lin
    try:
        regen_torch.score_forward(m, src, tgt, tgt_len, w.to(dt), False, True, dt)
    finally:
        F.linear = orig
    return cap["y"]


def test_graph_capture_of_both_backwards_replays_the_eager_bits():
    m, _ = model(300, seed=6)
    pairs = toys_shaped_pairs(200, m.n_item, 13)
    dev, w, dnll = score_inputs(m, pairs, 3, 4)
    dl = torch.randn(len(pairs), 5, generator=torch.Generator().manual_seed(4)).cuda().contiguous()

    def both():
        g, dw, nll = m.score_bwd_device(*dev, w, dnll)
        m.condition_bwd_device(dev[2], dev[3], dl, g, accumulate=True)
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


def test_score_and_decode_are_unchanged_after_loss_and_grad():
    m, _ = model(seed=7)
    pairs = toys_shaped_pairs(300, m.n_item, 15)
    srcs = [[m.sos] + s + [m.eos] for s, _ in pairs[:40]]
    before = m.score(pairs, "encoder", True, None, "hip")
    dec = m.decode(srcs, 0, 2, "hip")
    flat0, sflat0 = m.flat().clone(), m.score_flat().clone()
    m.loss_and_grad(pairs, "encoder", True, None, "hip", entropy_weight=1.0)
    after = m.score(pairs, "encoder", True, None, "hip")
    assert torch.equal(before.nll, after.nll) and torch.equal(before.cond_logits, after.cond_logits)
    assert m.decode(srcs, 0, 2, "hip") == dec
    assert torch.equal(m.flat(), flat0) and torch.equal(m.score_flat(), sflat0)


@pytest.mark.parametrize("mode", ["gumbel", "const"])
def test_hip_matches_the_reference_gradients_of_the_fixture(mode):
    """HIP grads, dw and loss against loss.backward() of the reference's own Generator (tests/golden/regen_grad_toys.npz: the scoring
    fixture's checkpoint and first 256 pairs, recorded Gumbel noise / the injected constant sample) and against float64, all 98
    tensors, 16 x the stored err32_t = max |reference fp32 - reference float64|"""
    from dr4sr_amd.regen import RegenModel
    from test_regen_grad_cpu import check_against_fixture, fixture_call, load_grad_fixture
    z, sd, pairs, err32, width = load_grad_fixture()
    m = RegenModel.from_state_dict(sd, "cuda")
    cpu = RegenModel.from_state_dict(sd, "cpu")
    cond, kw = fixture_call(z, mode)
    hip = m.loss_and_grad(pairs, cond, True, width, "hip", **kw)
    assert len(hip.grads) == 98
    check_against_fixture(z, err32, mode, hip, 16, "HIP vs the reference")
    cond64, kw = fixture_call(z, mode, torch.float64)
    r64 = cpu.loss_and_grad(pairs, cond64, True, width, "torch", torch.float64, **kw)
    worst = 0.0
    for k in r64.grads:                                    # table row 0 and the position rows >= max(Ls, T) like any other row
        e = err32[f"{mode}:{k}"]
        d = float((hip.grads[k].cpu().double() - r64.grads[k]).abs().max())
        assert d <= 16 * e, f"{mode}: {k}: |HIP - float64| {d:.3e} > 16 x err32 {e:.3e}"
        worst = max(worst, d / e) if e > 0 else worst
    e = err32.get(f"{mode}:dw")
    if mode == "const":
        assert float((hip.dw.cpu().double() - r64.dw).abs().max()) <= 16 * e
    print(f"HIP vs float64 on the fixture, {mode}: worst ratio {worst:.2f}")
    e_loss = abs(float(z[f"{mode}:loss"]) - float(z[f"{mode}:loss64"]))
    assert abs(float(hip.loss) - float(z[f"{mode}:loss64"])) <= 16 * max(e_loss, 6e-8 * float(z[f"{mode}:loss64"]))   # fp32 ulp of the value
    if mode == "gumbel":
        assert abs(float(hip.entropy) - float(z["gumbel:reg_loss64"])) <= 16 * 6e-8 * 2


def test_twenty_adam_steps_lower_the_scored_loss():
    """the public use end to end on the fixture's checkpoint and 256-pair batch: loss_and_grad + torch.optim.Adam with the reference's
    settings + load_params"""
    from dr4sr_amd.regen import RegenModel
    from test_regen_grad_cpu import load_grad_fixture
    z, sd, pairs, _, width = load_grad_fixture()
    m = RegenModel.from_state_dict(sd, "cuda")
    start = float(m.score(pairs, "encoder", True, width, "hip").loss()[0])
    names = list(m.p)
    params = [m.p[k].clone().requires_grad_(True) for k in names]
    opt = torch.optim.Adam(params, lr=1e-3, betas=(0.9, 0.98), eps=1e-9)
    addr = m.score_flat().data_ptr()
    for _ in range(20):
        r = m.loss_and_grad(pairs, "encoder", True, width, "hip", entropy_weight=1.0)
        for p, k in zip(params, names):
            p.grad = r.grads[k].clone()
        opt.step()
        m.load_params({k: p.detach() for p, k in zip(params, names)})
    assert m.score_flat().data_ptr() == addr
    end = float(m.score(pairs, "encoder", True, width, "hip").loss()[0])
    print(f"teacher-forced loss of the fixture's 256 pairs: {start:.4f} -> {end:.4f} after 20 Adam steps")
    assert end < start
