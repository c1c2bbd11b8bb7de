"""Gradients of the regenerator's teacher-forced loss without a GPU: RegenModel.loss_and_grad(backend="torch") (autograd through the
eager restatement, the float64 side of every gradient check), condition_grad(backend="torch"), state_dict / load_params, and the
argument checks of the HIP backward's entry points (the library loads without a GPU).

The finite-difference checks run in float64 with a central step of 1e-6: the truncation error is O(h^2) ~ 1e-12 relative and the
rounding error ~ 1e-16 / 1e-6 = 1e-10 of the loss (~5), so a correct gradient agrees to ~1e-8 absolute; the bound is 1e-6."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch


def small_model(device="cpu", seed=2, n_item=60):
    from dr4sr_amd.regen import RegenModel, random_state_dict
    return RegenModel.from_state_dict(random_state_dict(n_item, seed=seed, std=0.3, condition_encoder=True), device)


def small_pairs(n, n_item, seed):
    g = np.random.default_rng(seed)
    pairs = []
    for i in range(n):
        l = int(g.integers(2, 12))
        s = g.integers(1, n_item, l).tolist()
        pos = sorted(g.choice(l, int(g.integers(1, min(4, l) + 1)), replace=False).tolist())
        pairs.append([s, [s[p] for p in pos]])
    return pairs


def test_loss_is_the_scored_loss_and_the_result_is_complete():
    from dr4sr_amd.regen import score_param_names
    m = small_model()
    pairs = small_pairs(12, m.n_item, 0)
    w = torch.softmax(torch.randn(2, len(pairs), m.K, generator=torch.Generator().manual_seed(0)), -1)
    r = m.loss_and_grad(pairs, w, backend="torch", dtype=torch.float64)
    want = m.score(pairs, w, True, None, "torch", torch.float64).loss().sum()
    assert abs(float(r.loss) - float(want)) < 1e-12 and r.entropy is None
    assert sorted(r.grads) == sorted(score_param_names()) and len(r.grads) == 98
    assert tuple(r.dw.shape) == (2, len(pairs), m.K) and tuple(r.cond_logits.shape) == (len(pairs), m.K)
    assert all(r.grads[k].shape == m.p[k].shape and torch.isfinite(r.grads[k]).all() for k in r.grads)
    # constant weights: the condition encoder takes no gradient beyond the table rows the decoder and the source share
    assert all(float(r.grads[k].abs().max()) == 0 for k in r.grads if k.startswith("condition_encoder."))
    e = m.loss_and_grad(pairs, "encoder", backend="torch", dtype=torch.float64)
    want = m.score(pairs, "encoder", True, None, "torch", torch.float64).loss()[0]
    assert abs(float(e.loss) - float(want)) < 1e-12
    wz = torch.softmax(e.cond_logits, -1)
    assert abs(float(e.entropy) - float(-(wz * torch.log(wz + 1e-12)).sum(-1).mean())) < 1e-12
    assert any(float(e.grads[k].abs().max()) > 0 for k in e.grads if k.startswith("condition_encoder."))
    # a model without a condition encoder has the 70 tensors
    from dr4sr_amd.regen import RegenModel, random_state_dict
    m70 = RegenModel.from_state_dict(random_state_dict(60, seed=2, std=0.3), "cpu")
    assert len(m70.loss_and_grad(pairs, w, backend="torch").grads) == 70
    with pytest.raises(ValueError):
        m70.loss_and_grad(pairs, "encoder", backend="torch")


@pytest.mark.parametrize("causal", [True, False])
def test_central_finite_differences_in_float64(causal):
    from dr4sr_amd import regen_torch
    m = small_model()
    pairs = small_pairs(6, m.n_item, 1)
    g = torch.Generator().manual_seed(3)
    noise = -torch.log(-torch.log(torch.rand(len(pairs), m.K, generator=g, dtype=torch.float64)))
    kw = dict(causal_source=causal, backend="torch", dtype=torch.float64, noise=noise, tau=0.7, entropy_weight=1.0)
    r = m.loss_and_grad(pairs, "encoder", **kw)
    h = 1e-6
    for name, idx in (("transformer.decoder.layers.1.multihead_attn.in_proj_weight", (70, 5)),
                      ("condition_encoder.encoder.layers.0.linear1.weight", (3, 7)),
                      ("item_embedding.weight", (int(pairs[0][0][0]), 11)),
                      ("transformer.encoder.layers.0.norm1.weight", (9,))):
        base = m.p[name].clone()
        vals = []
        for sgn in (1, -1):
            # float64 perturbation: the model stores fp32, so the step goes into the float64 cast loss_and_grad differentiates
            m._cast.clear()
            p64 = m._params_as(torch.float64, torch.device("cpu"))
            p64[name][idx] += sgn * h
            src, src_len, tgt, tgt_len, _, _ = m._pack_pairs(pairs, None)
            _, c = regen_torch.score_forward(m, src, tgt, tgt_len, None, True, causal, torch.float64, p64)
            w = torch.softmax((c + noise) / 0.7, -1)[None]
            nll, _ = regen_torch.score_forward(m, src, tgt, tgt_len, w, False, causal, torch.float64, p64)
            vals.append(float(nll.sum() / (tgt[:, 1:] != 0).sum() - (w[0] * torch.log(w[0] + 1e-12)).sum(-1).mean()))
        m._cast.clear()
        assert torch.equal(m.p[name], base)
        fd = (vals[0] - vals[1]) / (2 * h)
        assert abs(fd - float(r.grads[name][idx])) < 1e-6, (name, fd, float(r.grads[name][idx]))
    # dw of a constant weight tensor
    w = torch.softmax(torch.randn(2, len(pairs), m.K, generator=g, dtype=torch.float64), -1)
    r = m.loss_and_grad(pairs, w, causal_source=causal, backend="torch", dtype=torch.float64)
    for idx in ((0, 2, 1), (1, 5, 4)):
        vals = []
        for sgn in (1, -1):
            w2 = w.clone()
            w2[idx] += sgn * h
            vals.append(float(m.score(pairs, w2, causal, None, "torch", torch.float64).loss().sum()))
        fd = (vals[0] - vals[1]) / (2 * h)
        assert abs(fd - float(r.dw[idx])) < 1e-6, (idx, fd, float(r.dw[idx]))


def test_condition_grad_is_the_chain_rule_link_of_the_encoder_mode():
    """loss_and_grad("encoder") = the decoder's dw, the few [n, K] operations in autograd, then the condition encoder's backward:
    condition_grad of that dlogits gives the condition_encoder.* gradients of the whole loss"""
    m = small_model()
    pairs = small_pairs(10, m.n_item, 4)
    noise = 0.3 * torch.randn(len(pairs), m.K, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    r = m.loss_and_grad(pairs, "encoder", backend="torch", dtype=torch.float64, noise=noise, tau=0.7, entropy_weight=1.0)
    c = r.cond_logits.clone().requires_grad_(True)
    w = torch.softmax((c + noise) / 0.7, -1)
    ((w * r.dw[0]).sum() - (w * torch.log(w + 1e-12)).sum(-1).mean()).backward()
    g = m.condition_grad(pairs, c.grad, backend="torch", dtype=torch.float64)
    assert len(g) == 2 + 28
    for k, v in g.items():
        if k.startswith("condition_encoder."):
            assert float((v - r.grads[k]).abs().max()) <= 1e-12 * max(1.0, float(r.grads[k].abs().max())), k
    with pytest.raises(ValueError):
        m.condition_grad(pairs, torch.zeros(3, m.K), backend="torch")


def test_a_target_id_outside_its_source_raises():
    m = small_model()
    pairs = small_pairs(5, m.n_item, 6)
    out = next(v for v in range(1, m.n_item) if v not in pairs[2][0])
    pairs[2][1] = [pairs[2][1][0], out]
    w = torch.full((1, 5, m.K), 0.2)
    with pytest.raises(ValueError, match="pair 2"):
        m.loss_and_grad(pairs, w, backend="torch")
    with pytest.raises(ValueError, match="pair 2"):                   # a host check: raised before anything touches a device
        m.loss_and_grad(pairs, w, backend="hip")
    with pytest.raises(ValueError):
        m.loss_and_grad(small_pairs(5, m.n_item, 6), w, backend="triton")


def test_load_params_round_trip_keeps_the_buffers():
    m = small_model()
    pairs = small_pairs(8, m.n_item, 7)
    sd = m.state_dict()
    assert sd["item_embedding_decoder.weight"] is sd["item_embedding.weight"] and len(sd) == 99
    before = m.score(pairs, "encoder", True, None, "torch", torch.float64)
    flat, sflat = m.flat(), m.score_flat()
    addr = (flat.data_ptr(), sflat.data_ptr(), {k: v.data_ptr() for k, v in m.p.items()})
    r = m.loss_and_grad(pairs, "encoder", backend="torch", entropy_weight=1.0)
    stepped = {k: sd[k] - 0.05 * r.grads[k] for k in r.grads}
    m.load_params(stepped)
    assert (m.flat().data_ptr(), m.score_flat().data_ptr(), {k: v.data_ptr() for k, v in m.p.items()}) == addr
    from dr4sr_amd.regen import RegenModel
    fresh = RegenModel.from_state_dict({**stepped, "item_embedding_decoder.weight": stepped["item_embedding.weight"]}, "cpu")
    assert torch.equal(m.flat(), fresh.flat()) and torch.equal(m.score_flat(), fresh.score_flat())
    after = m.score(pairs, "encoder", True, None, "torch", torch.float64)
    want = fresh.score(pairs, "encoder", True, None, "torch", torch.float64)
    assert torch.equal(after.nll, want.nll) and torch.equal(after.cond_logits, want.cond_logits)
    assert float(after.loss()[0]) != float(before.loss()[0])
    m.load_params(sd)                                                  # and back: the same scores, bit for bit
    again = m.score(pairs, "encoder", True, None, "torch", torch.float64)
    assert torch.equal(again.nll, before.nll) and torch.equal(m.state_dict()["condition_linear.2.bias"], sd["condition_linear.2.bias"])
    with pytest.raises(KeyError):
        m.load_params({"no.such.tensor": torch.zeros(1)})
    with pytest.raises(ValueError):
        m.load_params({"condition_linear.2.bias": torch.zeros(3)})


def test_adopt_score_flat_takes_a_checked_buffer_and_load_params_writes_through_it():
    m = small_model()
    n = m.score_flat().numel()
    master = torch.zeros(n + 3)                                        # a trainer's padded master: the model's buffer is a view of it
    master[:n] = m.score_flat()
    m.adopt_score_flat(master[:n])
    plan = m.score_plan()
    assert (m.score_flat().data_ptr(), plan.params, plan.n_params) == (master.data_ptr(), master.data_ptr(), n)
    m.load_params({"condition_linear.2.bias": torch.full_like(m.p["condition_linear.2.bias"], 0.25)})
    assert torch.equal(m.grads_from_flat(master[:n])["condition_linear.2.bias"], m.p["condition_linear.2.bias"])
    assert float(master[n:].abs().max()) == 0.0
    for bad in (torch.zeros(n + 1), torch.zeros(n, dtype=torch.float64), torch.zeros(2 * n)[::2], torch.zeros(1, n), torch.zeros(n, device="meta")):
        with pytest.raises(ValueError, match="score buffer"):
            m.adopt_score_flat(bad)
    assert m.score_flat().data_ptr() == master.data_ptr()


def test_argument_errors_of_the_backward_entry_points():
    from dr4sr_amd import _lib
    lib = _lib.load()
    assert lib.dr4sr_abi_version() == 10 == _lib.ABI_VERSION
    n = lib.dr4sr_regen_score_param_layout(11927, 5, None)
    n_old = lib.dr4sr_regen_param_layout(11927, 5, None)
    off = (C.c_int64 * 98)()
    lib.dr4sr_regen_score_param_layout(11927, 5, off)
    p = _lib.RegenPlan()
    p.abi_version, p.n_rows, p.K, p.max_len, p.D, p.H, p.F, p.n_layer, p.ln_eps = 10, 11927, 5, 25, 64, 2, 256, 2, 1e-12
    p.params, p.n_params = 4096, n                                    # never dereferenced by the host-side checks
    B = C.byref
    al = lambda b: (b + 255) // 256 * 256
    def want(n_pair, T):
        slots = (n_pair * T + 64 - T) // (65 - T) * 64
        return al((n_pair + 1) * 4) + 2 * al(slots * 4) + al(32 * (n - off[70]) * 4) + al(slots * 3976 * 4)
    wsb = lib.dr4sr_regen_score_condition_bwd_workspace_bytes
    assert wsb(B(p), 100, 19) == want(100, 19) and wsb(B(p), 7, 49) == want(7, 49) and wsb(B(p), 0, 1) == want(0, 1)
    for args, rc in (((10, 51), -2), ((-1, 19), -1), ((10, 0), -1), ((1 << 24, 19), -1)):
        assert wsb(B(p), *args) == rc, args
    q = _lib.RegenPlan.from_buffer_copy(p)
    q.n_params = n_old                                                # the decode layout's buffer is refused
    assert wsb(B(q), 10, 19) == -1
    for field, val, rc in (("D", 128, -2), ("H", 4, -2), ("F", 128, -2), ("n_layer", 3, -2), ("K", 6, -2), ("abi_version", 9, -1), ("params", 0, -1)):
        q2 = _lib.RegenPlan.from_buffer_copy(p)
        setattr(q2, field, val)
        assert wsb(B(q2), 10, 19) == rc, field
    a = C.c_void_p(64)
    wsp, big = C.c_void_p(8192), 1 << 40
    bwd = lambda **kw: lib.dr4sr_regen_score_condition_bwd(B(kw.get("plan", p)), kw.get("tgt", a), kw.get("tgt_len", a), kw.get("n", 4),
                                                           kw.get("T", 19), kw.get("dlogits", a), kw.get("ws", wsp), kw.get("bytes", big),
                                                           kw.get("grad", a), kw.get("acc", 1), None)
    for name in ("tgt", "tgt_len", "dlogits", "grad"):
        assert bwd(**{name: None}) == -1, name
    assert bwd(T=51) == -2 and bwd(T=0) == -1 and bwd(n=-1) == -1 and bwd(ws=None) == -3 and bwd(bytes=want(4, 19) - 1) == -3
    assert bwd(plan=q) == -1
    assert bwd(n=0, acc=1) == 0                                       # nothing to add: nothing is launched
    # dr4sr_regen_score_bwd: the forward's workspace first, then the backward's records
    sws = lib.dr4sr_regen_score_bwd_workspace_bytes
    fwd = lambda n_pair, Ls, K=5: al((n_pair + 1) * 4) + n_pair * K * 2 * Ls * 128 * 4
    def want_s(n_pair, Ls, T, n_w):
        tiles = (n_pair * n_w * T + 64 - T) // (65 - T)
        rows = n_pair * n_w * Ls
        return (al(fwd(n_pair, Ls)) + al(n_pair * n_w * T * 4) + 2 * al(tiles * 64 * 4) + 2 * al(n_pair * Ls * 4) + al(rows * 4)
                + al(rows * 256 * 4) + al(rows * 64 * 4) + al(32 * (off[70] - off[2]) * 4) + al(tiles * 64 * 4992 * 4) + al(n_pair * Ls * 6592 * 4))
    assert sws(B(p), 100, 50, 19, 2) == want_s(100, 50, 19, 2) and sws(B(p), 7, 23, 49, 1) == want_s(7, 23, 49, 1)
    for args, rc in (((10, 51, 19, 5), -2), ((10, 50, 51, 5), -2), ((-1, 50, 19, 5), -1), ((10, 0, 19, 5), -1), ((10, 50, 0, 5), -1),
                     ((10, 50, 19, 0), -1)):
        assert sws(B(p), *args) == rc, args
    assert sws(B(q), 10, 50, 19, 5) == -1
    sb = lambda **kw: lib.dr4sr_regen_score_bwd(B(kw.get("plan", p)), kw.get("src", a), kw.get("src_len", a), kw.get("tgt", a), kw.get("tgt_len", a),
                                                kw.get("n", 4), kw.get("Ls", 50), kw.get("T", 19), kw.get("w", a), kw.get("n_w", 2), 1,
                                                kw.get("dnll", a), kw.get("ws", wsp), kw.get("bytes", big), kw.get("grad", a), kw.get("dw", a),
                                                kw.get("nll", None), kw.get("acc", 1), None)
    for name in ("src", "src_len", "tgt", "tgt_len", "w", "dnll", "grad", "dw"):
        assert sb(**{name: None}) == -1, name
    assert sb(Ls=51) == -2 and sb(T=51) == -2 and sb(n_w=0) == -1 and sb(n=-1) == -1 and sb(Ls=0) == -1 and sb(T=0) == -1
    assert sb(ws=None) == -3 and sb(bytes=want_s(4, 50, 19, 2) - 1) == -3 and sb(plan=q) == -1
    assert sb(n=0, acc=1) == 0


# ---------------------------------------------------------------------------------------------------- the reference's own gradients
GOLD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE_MODES = ("gumbel", "const")


def load_grad_fixture():
    """tests/golden/regen_grad_toys.npz (+ its part files), made by tools/make_regen_grad_golden.py from the reference's stage 2
    classes: (arrays, the scoring fixture's state dict, its first 256 pairs, err32 per 'mode:tensor', widths)"""
    from test_regen_score_cpu import load_score_fixture
    z = dict(np.load(os.path.join(GOLD_DIR, "regen_grad_toys.npz")))
    for name in json.loads(str(z["parts"])):
        z.update(np.load(os.path.join(GOLD_DIR, name)))
    _, sd, pairs, _, width = load_score_fixture()
    assert width == (int(z["Ls"]), int(z["T"]))
    return z, sd, pairs[:int(z["n_pairs"])], json.loads(str(z["err32"])), width


def fixture_call(z, mode, dtype=torch.float32):
    """what loss_and_grad takes to replay a fixture mode: (conditions, keyword arguments)"""
    if mode == "gumbel":
        return "encoder", dict(noise=torch.from_numpy(z["noise"]), tau=1.0, entropy_weight=1.0)
    return torch.from_numpy(z["sample"]).to(dtype)[None], {}


def reg_loss_grad(w):
    """the injected weights also feed the reference's reg_loss (condition4loss): its gradient, which the recorded dw contains"""
    return -(torch.log(w + 1e-12) + w / (w + 1e-12)) / w.shape[0]


def check_against_fixture(z, err32, mode, res, factor, what, dw_dtype=torch.float32, slack=0.0):
    """every one of the 98 tensors (and dw in const mode) of a GradResult against the recorded reference gradients: within
    factor x err32_t + slack x max |recorded gradient| of the tensor"""
    from dr4sr_amd.regen import score_param_names
    worst, seen = 0.0, 0
    items = [(k, res.grads[k], z[f"{mode}:g:{k}"]) for k in score_param_names()]
    if mode == "const":
        items.append(("dw", res.dw[0].cpu() + reg_loss_grad(torch.from_numpy(z["sample"]).to(dw_dtype)), z["const:dw"]))
    bad = []
    for k, got, want in items:
        e = err32[f"{mode}:{k}"]
        d = float((got.detach().cpu().double() - torch.from_numpy(want).double()).abs().max())
        seen += 1
        if e > 0:
            worst = max(worst, d / e)
        if d > factor * e + slack * float(np.abs(want).max()):
            bad.append(f"{k}: |diff| {d:.3e} > {factor} x err32 {e:.3e}")
    print(f"{what}, {mode}: worst |diff| / err32_t over {seen} tensors: {worst:.2f}")
    assert seen == 98 + (mode == "const") and not bad, f"{what}, {mode}:\n" + "\n".join(bad)
    return worst


@pytest.mark.parametrize("mode", FIXTURE_MODES)
def test_torch_backend_matches_the_reference_gradients(mode):
    """backend="torch" against loss.backward() of the reference's Generator (loss_fn + 1 * reg_loss, eval mode, recorded Gumbel
    noise, tau 1, causal source mask): fp32 within 4 x err32_t of the reference's fp32 gradients, float64 within 1 x err32_t
    (err32_t = max |reference fp32 - reference float64| per tensor, stored), loss and entropy against the recorded scalars"""
    from dr4sr_amd.regen import RegenModel
    z, sd, pairs, err32, width = load_grad_fixture()
    m = RegenModel.from_state_dict(sd, "cpu")
    assert len(pairs) == 256 and float(z["agree64"]) < 1e-10 and max(json.loads(str(z["ratio32"])).values()) <= 4
    cond, kw = fixture_call(z, mode)
    r32 = m.loss_and_grad(pairs, cond, True, width, "torch", torch.float32, **kw)
    check_against_fixture(z, err32, mode, r32, 4, "fp32 restatement vs the reference")
    cond, kw = fixture_call(z, mode, torch.float64)
    r64 = m.loss_and_grad(pairs, cond, True, width, "torch", torch.float64, **kw)
    # float64 against the recorded fp32 gradients within 1 x err32_t.  err32_t IS max |reference fp32 - reference float64|, and the
    # restatement's float64 equals the reference's float64 only to the 1e-10 relative the tool asserts (measured 1e-15), so by the
    # triangle inequality the bound is 1 x err32_t + 1e-10 x max |gradient|: without that term the comparison is d <= d up to an ulp
    check_against_fixture(z, err32, mode, r64, 1, "float64 restatement vs the reference", torch.float64, slack=1e-10)
    e_loss = abs(float(z[f"{mode}:loss"]) - float(z[f"{mode}:loss64"]))
    assert abs(float(r64.loss) - float(z[f"{mode}:loss64"])) <= 1e-12 and abs(float(r32.loss) - float(z[f"{mode}:loss"])) <= 4 * max(e_loss, 6e-8 * 5)
    if mode == "gumbel":
        assert abs(float(r64.entropy) - float(z["gumbel:reg_loss64"])) <= 1e-12
        assert abs(float(r32.entropy) - float(z["gumbel:reg_loss"])) <= 4 * max(abs(float(z["gumbel:reg_loss"]) - float(z["gumbel:reg_loss64"])), 6e-8 * 2)
        assert any(float(np.abs(z[f"gumbel:g:{k}"]).max()) > 0 for k in r32.grads if k.startswith("condition_encoder."))
    else:
        assert all(float(np.abs(z[f"const:g:{k}"]).max()) == 0 for k in r32.grads if k.startswith("condition_encoder."))
    assert float(np.abs(z[f"{mode}:g:item_embedding.weight"][0]).max()) > 0        # PAD row 0: through the logits of padded rows
