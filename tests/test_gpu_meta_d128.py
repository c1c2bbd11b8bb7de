"""DR4SR+ at embed_dim 128 on the GPU: the D = 128 meta-module selection kernels (dr4sr_meta_select_fwd_d / _bwd_d) against a float64
restatement, the weighted inner step / hyper-gradient / meta SGD against the fixture made by RUNNING the reference at d = 128
(tests/golden/metamodel_sasrec_d128*.npz), and fit() + evaluate() through the dense weighted step (the fused step stays D = 64).

Bound of the kernel tests.  |kernel - float64| <= 16 x e32, e32 = |fp32 torch - float64| of the SAME function on the same inputs (max
norm, per output), the margin of the regenerator tests; e32 is floored at one fp32 rounding of the output's largest magnitude
(2^-24 max|ref|: an fp32 evaluation that happens to land on the float64 values measures 0, and no fp32 result is better than that).  The
ReLU pattern is taken from the kernel (gate_out) in every restatement, so that a pre-activation within rounding of 0 cannot flip between
the three evaluations; that pattern itself is checked against float64 wherever |pre| is above 16 x the fp32 error of pre."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import metamodel_oracle as MO  # noqa: E402

import _meta_d128  # noqa: E402
from test_gpu_meta import build, make_config, rel  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = MO.META_NAMES
L = 50
TAU = 3.0


# ------------------------------------------------------------------------------------------------ selection kernels
def philox_uniform_pair(n, seed, step):
    """the kernel's draw (csrc/meta.hip gumbel_pair): Philox4x32-10, counter (p lo, p hi, 'meta', step), key = seed; u = (r >> 8 + 0.5) / 2^24
    evaluated in fp32 like the kernel; returns u0, u1 as float32 arrays"""
    M = np.uint64(0xFFFFFFFF)
    p = np.arange(n, dtype=np.uint64)
    c = [p & M, p >> np.uint64(32), np.full(n, 0x6D657461, np.uint64), np.full(n, step, np.uint64)]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    f = lambda r: ((r >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    return f(c[0]), f(c[1])


def make_inputs(D, B, forced_row, seed=3):
    g = torch.Generator().manual_seed(seed + 17 * B + D)
    meta = {"0.weight": torch.randn(D, D, generator=g) * (1.6 / D ** 0.5), "0.bias": torch.randn(D, generator=g) * 0.1,
            "2.weight": torch.randn(2, D, generator=g) * 0.3, "2.bias": torch.randn(2, generator=g) * 0.1}
    q = torch.randn(B, L, D, generator=g)
    gum = -torch.empty(B, L, 2).exponential_(generator=g).log()
    tgt = torch.randint(1, 100, (B, L), generator=g)
    tgt[:, 37:] = 0                                         # PAD tail on every row ...
    if B > 1:
        tgt[B // 2, 5:] = 0                                 # ... and one short row
    uid = torch.arange(1, B + 1)
    if forced_row is not None:
        uid[forced_row] = 0
    up = torch.randn(B, L, generator=g)
    return meta, q, gum, tgt, uid, up


def bits_of(gate, n, D):
    return ((gate.cpu().view(n, D // 64, 1) >> torch.arange(64).view(1, 1, 64)) & 1).reshape(n, D)


def restate(meta, q, gum, tgt, uid, up, scale, gate_bits, dtype):
    """weight, d_query, d_phi of sum_p weight_p up_p scale by torch autograd in `dtype`, ReLU pattern given"""
    qo = q.detach().to(dtype).clone().requires_grad_(True)
    mo = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in meta.items()}
    w = MO.mask_weight(MO.selection(qo, mo, gum.to(dtype), TAU, 1.0, relu_gate=gate_bits.view(q.shape).to(dtype)), uid, tgt)
    ((w * up.to(dtype)).sum() * scale).backward()
    zero = lambda t, like: t if t is not None else torch.zeros_like(like)
    dphi = torch.cat([zero(mo[k].grad, mo[k]).reshape(-1) for k in NAMES])
    return w.detach().double(), zero(qo.grad, qo).double(), dphi.double()


class Kernels:
    def __init__(self, D, meta, q, gum, tgt, uid, seed=11, step=7):
        from dr4sr_amd import _lib
        self.L, self.lib, self.D = _lib, _lib.load(), D
        self.B, self.n = q.shape[0], q.shape[0] * q.shape[1]
        self.nphi = int(self.lib.dr4sr_meta_param_count(D))
        assert self.nphi == D * D + D + 2 * D + 2
        self.phi = torch.cat([meta[k].reshape(-1) for k in NAMES]).cuda()
        self.q, self.tgt, self.uid = q.cuda().contiguous(), tgt.cuda(), uid.cuda()
        self.gum = gum.cuda().reshape(-1, 2).contiguous() if gum is not None else None
        self.seed, self.step = seed, step
        nws = int(self.lib.dr4sr_meta_select_workspace_floats_d(self.n, D))
        assert nws > 0 and nws % self.nphi == 0
        self.ws = torch.empty(nws, device="cuda")

    def fwd(self, gate_in=None, want_gate=True, q=None):
        P = self.L.ptr
        w = torch.full((self.n,), -7.0, device="cuda")
        gate = torch.full((self.n * (self.D // 64),), -1, dtype=torch.int64, device="cuda") if want_gate else None
        self.L.check(self.lib.dr4sr_meta_select_fwd_d(P(self.q if q is None else q), P(self.phi), P(self.gum), self.seed, self.step, None, TAU,
                                                    P(self.uid), P(self.tgt), self.B, L, self.D, P(gate_in), P(gate), P(w),
                                                    self.L.cur_stream()), "fwd")
        return w, gate

    def bwd(self, up, scale=None, gate_in=None, want_dq=True):
        P = self.L.ptr
        dq = torch.zeros(self.n, self.D, device="cuda") if want_dq else None
        dphi = torch.zeros(self.nphi, device="cuda")
        sc = torch.tensor([scale], dtype=torch.float32, device="cuda") if scale is not None else None
        self.L.check(self.lib.dr4sr_meta_select_bwd_d(P(self.q), P(self.phi), P(self.gum), self.seed, self.step, None, TAU, P(self.uid),
                                                    P(self.tgt), self.B, L, self.D, P(gate_in), P(up), P(sc), P(dq), P(dphi), P(self.ws),
                                                    self.L.cur_stream()), "bwd")
        return dq, dphi


def select_case(D, B, noise, forced_row):
    """runs one case through kernels, float64 and fp32 torch; asserts the 16 x e32 bound; returns {output: (err, e32)} per scale"""
    meta, q, gum, tgt, uid, up = make_inputs(D, B, forced_row)
    n = B * L
    if noise == "philox":
        K = Kernels(D, meta, q, None, tgt, uid)
        u0, u1 = philox_uniform_pair(n, K.seed, K.step)
        u = torch.from_numpy(np.stack([u0, u1], -1)).view(B, L, 2)
        gum_of = lambda dt: -(-u.to(dt).log()).log()            # the noise of each restatement in its own precision, from the same u
    else:
        K = Kernels(D, meta, q, gum, tgt, uid)
        gum_of = lambda dt: gum.to(dt)
    w, gate = K.fwd()
    bits = bits_of(gate, n, D)
    valid = (tgt != 0).reshape(-1)
    assert int(bits[~valid].sum()) == 0                        # PAD: pattern 0
    pre64 = (q.double() @ meta["0.weight"].double().T + meta["0.bias"].double()).reshape(n, D)
    pre32 = (q @ meta["0.weight"].T + meta["0.bias"]).reshape(n, D)
    clear = (pre64.abs() > 16 * float((pre32.double() - pre64).abs().max())) & valid.view(n, 1)
    assert torch.equal(bits.bool()[clear], (pre64 > 0)[clear]) and float(clear.float().mean()) > 0.5
    upd = up.cuda().reshape(-1).contiguous()
    out = {}
    for scale in (None, 0.37):
        s = 1.0 if scale is None else scale
        r64 = restate(meta, q, gum_of(torch.float64), tgt, uid, up, s, bits, torch.float64)
        r32 = restate(meta, q, gum_of(torch.float32), tgt, uid, up, s, bits, torch.float32)
        dq, dphi = K.bwd(upd, scale)
        dq_n, dphi_n = K.bwd(upd, scale, want_dq=False)        # d_query NULL: d_phi is the same bits
        assert dq_n is None and torch.equal(dphi_n, dphi)
        _, dphi_g = K.bwd(upd, scale, gate_in=gate)            # recorded pattern fed back == recomputed pattern
        assert torch.equal(dphi_g, dphi)
        got = (w.cpu().double().view(B, L), dq.cpu().double().view(B, L, D), dphi.cpu().double())
        for name, a, b64, b32 in zip(("weight", "d_query", "d_phi"), got, r64, r32):
            err = float((a - b64).abs().max())
            e32 = max(float((b32 - b64).abs().max()), 2.0 ** -24 * float(b64.abs().max()))
            out[(name, scale)] = (err, e32)
    for (name, scale), (err, e32) in out.items():
        print(f"D={D} B={B} {noise} forced={forced_row} scale={scale} {name}: |hip-f64| {err:.3e}  e32 {e32:.3e}  ratio {err / max(e32, 1e-300):.2f}")
    if forced_row is not None:
        wv = w.view(B, L).cpu()
        assert bool((wv[forced_row][tgt[forced_row] != 0] == 1.0).all())
    assert float(w[~valid.cuda()].abs().max()) == 0.0
    for key, (err, e32) in out.items():
        assert err <= 16 * e32, (key, err, e32)
    return out


@pytest.mark.parametrize("noise", ["explicit", "philox"])
@pytest.mark.parametrize("B,forced_row", [(1, None), (1, 0), (7, 4), (128, 4)])
def test_select_kernels_match_float64(B, forced_row, noise):
    """B = 128: 6 400 positions, above the grid cap (128 blocks x 4 waves x 8), so the stride loop runs; (1, 0): the only row is a pattern
    row — weight 1, gradients exactly 0"""
    out = select_case(128, B, noise, forced_row)
    if B == 1 and forced_row == 0:
        assert out[("d_phi", None)][0] == 0.0 and out[("d_query", None)][0] == 0.0


@pytest.mark.parametrize("noise", ["explicit", "philox"])
def test_select_kernels_d64_sanity_line(noise):
    """the D = 64 kernels through the same harness and bound (the ratios printed here stand beside the D = 128 ones in NOTEBOOK.md)"""
    select_case(64, 7, noise, 4)


def test_upper_half_units_and_gate_words():
    """W2 = 0 for units 0-63: only units 64-127 (gate word 1) decide the weight.  A gate_in whose SECOND word alone differs from the natural
    pattern moves the weight exactly as the float64 restatement with that pattern; gate_out fed back as gate_in reproduces the forward bitwise"""
    D, B = 128, 7
    meta, q, gum, tgt, uid, up = make_inputs(D, B, 4)
    meta["2.weight"][:, :64] = 0
    n = B * L
    K = Kernels(D, meta, q, gum, tgt, uid)
    w, gate = K.fwd()
    w_again, gate_again = K.fwd(gate_in=gate)
    assert torch.equal(w_again, w) and torch.equal(gate_again, gate)
    g2 = gate.view(n, 2).clone()
    g2[:, 1] ^= 0x5A5A5A5A5A5A5A5                              # flip a fixed set of upper-half units, word 0 untouched
    w_flip, gate_flip = K.fwd(gate_in=g2.view(-1))
    live = (tgt != 0).reshape(-1).cuda()                        # (a PAD position records pattern 0 whatever it was given)
    assert torch.equal(gate_flip.view(n, 2)[live], g2[live]) and int(gate_flip.view(n, 2)[~live].abs().sum()) == 0
    f64 = lambda bits: MO.mask_weight(MO.selection(q.double(), {k: v.double() for k, v in meta.items()}, gum.double(), TAU, 1.0,
                                                   relu_gate=bits.view(B, L, D).double()), uid, tgt)
    f32 = lambda bits: MO.mask_weight(MO.selection(q, meta, gum, TAU, 1.0, relu_gate=bits.view(B, L, D).float()), uid, tgt).double()
    free = ((tgt != 0) & (uid != 0).view(B, 1)).reshape(-1)
    for got, g in ((w, gate), (w_flip, g2.view(-1))):
        bits = bits_of(g, n, D)
        ref = f64(bits)
        e32 = max(float((f32(bits) - ref).abs().max()), 2.0 ** -24)
        assert float((got.cpu().double().view(B, L) - ref).abs().max()) <= 16 * e32
    moved = (w_flip - w).abs().cpu()[free]
    assert float(moved.max()) > 1e-3                            # the second word is read ...
    g1 = gate.view(n, 2).clone()
    g1[:, 0] ^= 0x5A5A5A5A5A5A5A5                              # ... and the first one, whose units have W2 = 0, changes nothing
    w_low, _ = K.fwd(gate_in=g1.view(-1))
    assert torch.equal(w_low, w)


def test_backward_is_bitwise_reproducible():
    D, B = 128, 128
    meta, q, gum, tgt, uid, up = make_inputs(D, B, 4)
    K = Kernels(D, meta, q, gum, tgt, uid)
    upd = up.cuda().reshape(-1).contiguous()
    dq1, dphi1 = K.bwd(upd, 0.37)
    dq2, dphi2 = K.bwd(upd, 0.37)
    assert torch.equal(dq1, dq2) and torch.equal(dphi1, dphi2) and float(dphi1.abs().max()) > 0
    # accumulating semantics of d_phi / d_query: a second call into the same buffers doubles them (x + x is exact)
    P = K.L.ptr
    K.L.check(K.lib.dr4sr_meta_select_bwd_d(P(K.q), P(K.phi), P(K.gum), K.seed, K.step, None, TAU, P(K.uid), P(K.tgt), B, L, D, None, P(upd),
                                          P(torch.tensor([0.37], device="cuda")), P(dq1), P(dphi1), P(K.ws), K.L.cur_stream()), "bwd")
    assert torch.equal(dq1, 2 * dq2) and torch.equal(dphi1, 2 * dphi2)


def test_other_widths_are_shape_errors():
    from dr4sr_amd import _lib
    lib = _lib.load()
    one = torch.zeros(16, device="cuda")
    tgt = torch.ones(4, dtype=torch.int64, device="cuda")
    P = _lib.ptr
    assert lib.dr4sr_meta_param_count(96) == -2 and lib.dr4sr_meta_select_workspace_floats_d(200, 96) == -2
    assert lib.dr4sr_meta_select_fwd_d(P(one), P(one), None, 0, 0, None, 1.0, None, P(tgt), 4, 1, 96, None, None, P(one), None) == -2
    assert lib.dr4sr_meta_select_bwd_d(P(one), P(one), None, 0, 0, None, 1.0, None, P(tgt), 4, 1, 96, None, P(one), None, None, P(one), P(one),
                                     None) == -2
    for D in (96, 128):                                           # the D = 64 entry points keep answering any other width with a shape error
        assert lib.dr4sr_meta_select_fwd(P(one), P(one), None, 0, 0, None, 1.0, None, P(tgt), 4, 1, D, None, None, P(one), None) == -2
        assert lib.dr4sr_meta_select_bwd(P(one), P(one), None, 0, 0, None, 1.0, None, P(tgt), 4, 1, D, None, P(one), None, None, P(one),
                                         P(one), None) == -2
    assert lib.dr4sr_meta_param_count(128) == 16770 and lib.dr4sr_meta_param_count(64) == 4290
    assert lib.dr4sr_meta_select_workspace_floats_d(12800, 64) == lib.dr4sr_meta_select_workspace_floats(12800)
    assert lib.dr4sr_meta_select_workspace_floats_d(12800, 128) == lib.dr4sr_meta_select_workspace_floats(12800) // 4290 * 16770


# ------------------------------------------------------------------------------------------------ against the reference's run at d = 128
def config_d128(n_items, **kw):
    cfg = make_config(n_items, **kw)
    cfg["model"]["embed_dim"] = 128
    cfg["model"]["sub_overrides"]["model"]["embed_dim"] = 128
    return cfg


def load_fixture(model):
    z = _meta_d128.load()
    t = lambda v: torch.from_numpy(v.copy())
    model.sub_model.load_state_dict({k[6:]: t(v) for k, v in z.items() if k.startswith("param.")}, strict=True)
    model.meta_module.load_state_dict({k[11:]: t(v) for k, v in z.items() if k.startswith("meta_param.")}, strict=True)
    dev = model.device
    bt = {k[6:]: t(v).to(dev) for k, v in z.items() if k.startswith("train.")}
    bv = {k[4:]: t(v).to(dev) for k, v in z.items() if k.startswith("val.")}
    model._gumbel = t(z["inner.gumbel"]).to(dev).reshape(-1, 2).contiguous()
    return z, bt, bv


def test_inner_weighted_step_matches_reference(monkeypatch):
    z = _meta_d128.load()
    ds, model = build(config_d128(int(z["meta.num_items"])), monkeypatch)
    z, bt, bv = load_fixture(model)
    assert model.embed_dim == 128 and model._phi.n == 16770 and not model._fused_ok()
    model.train()
    sub, eng = model.sub_model, model.engine
    # API path: loss = model.training_step(batch); loss.backward()
    sub.optimizer.zero_grad()
    model.meta_optimizer.zero_grad()
    loss = model.training_step(batch=bt, align=False)
    loss.backward()
    ref_loss = float(z["inner.loss"])
    print("autograd loss", float(loss.detach()), "reference", ref_loss)
    assert abs(float(loss.detach()) - ref_loss) < 3e-6 * max(1.0, abs(ref_loss))
    for n, p in sub.named_parameters():
        ref = z["inner.grad." + n]
        assert rel(p.grad.cpu().numpy(), ref) < 3e-4 or np.abs(ref).max() < 1e-7, n
    for n, p in model.meta_module.named_parameters():
        assert rel(p.grad.cpu().numpy(), z["inner.meta_grad." + n]) < 3e-4, n
    # dense weighted step: same kernels without autograd, un-normalised sums + tail
    w, lp = model._weighted_fwd_bwd(bt)
    nv = float(eng.grads[eng.n_params])
    np.testing.assert_allclose(w.cpu().numpy().reshape(z["inner.weight"].shape), z["inner.weight"], rtol=1e-4, atol=1e-6)
    assert abs(float(eng.grads[eng.n_params + 1]) / nv - ref_loss) < 3e-6 * max(1.0, abs(ref_loss))
    for n, p in sub.named_parameters():
        ref = z["inner.grad." + n]
        assert rel((p.grad / nv).cpu().numpy(), ref) < 3e-4 or np.abs(ref).max() < 1e-7, n
    for n, p in model.meta_module.named_parameters():
        assert rel((p.grad / nv).cpu().numpy(), z["inner.meta_grad." + n]) < 3e-4, n


@pytest.mark.parametrize("forward_hvp", [False, True])
def test_hypergradient_and_meta_sgd_match_reference(monkeypatch, forward_hvp):
    z = _meta_d128.load()
    cfg = config_d128(int(z["meta.num_items"]))
    cfg["train"]["hypergrad_forward_hvp"] = forward_hvp
    ds, model = build(cfg, monkeypatch)
    z, bt, bv = load_fixture(model)
    model.train()
    theta = model.engine.params.clone()
    hyper = model.hypergrad(bv, bt)
    assert torch.equal(theta, model.engine.params)                 # the probe shifts are undone exactly
    ref = np.concatenate([z["outer.hypergrad." + k].ravel() for k in NAMES])
    err = rel(hyper.cpu().numpy(), ref)
    print("d = 128 hyper-gradient rel. error vs reference double-backward (forward_hvp %s): %.3e" % (forward_hvp, err))
    assert err < 1e-3, err
    for s in (1, 2):
        model.hypergrad_step(bv, bt)
        assert torch.equal(theta, model.engine.params)
        for k, p in model.meta_module.named_parameters():
            np.testing.assert_allclose(p.detach().cpu().numpy(), z[f"outer.step{s}.{k}"], rtol=2e-5, atol=3e-7)


# ------------------------------------------------------------------------------------------------ fit
def fit_config(sub, deterministic):
    cfg = config_d128(150, sub=sub, dropout=0.5, n_rows=300, batch=64, epochs=2, warmup=-1, interval=2)
    cfg["train"]["hip_graph"] = True
    if deterministic:
        cfg["train"]["deterministic"] = True
    return cfg


def one_fit(cfg, evaluate=False):
    from dr4sr_amd.utils import prepare_datasets, prepare_model, seed_everything
    seed_everything(cfg["train"]["seed"])
    ds = prepare_datasets(cfg)
    model = prepare_model(cfg, ds)
    model.fit()
    torch.cuda.synchronize()
    losses = {k: float(v) for k, v in model.logged_metrics.items() if k.startswith("train_")}
    assert losses and all(np.isfinite(v) for v in losses.values()), losses
    assert model.embed_dim == 128 and not model._fused_ok() and model.meta_optimizer.step_count.item() > 0
    metrics = model.evaluate() if evaluate else None
    return [model.engine.params.detach().clone()] + [p.detach().clone() for p in model.meta_module.parameters()], metrics


@pytest.mark.parametrize("sub", ["SASRec", "CL4SRec"])
def test_fit_and_evaluate(tmp_path, monkeypatch, sub):
    """two weighted epochs (no warm-up) with an outer step every 2 steps through the captured dense weighted step, then evaluate()"""
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("DR4SR_CONFIG_DIR", os.path.join(ROOT, "configs"))
    state, out = one_fit(fit_config(sub, False), evaluate=True)
    assert {"ndcg@20", "recall@20"} <= set(out) and all(np.isfinite(v) for v in out.values())
    assert all(bool(torch.isfinite(t).all()) for t in state)


@pytest.mark.parametrize("sub", ["SASRec", "CL4SRec"])
def test_fit_is_bitwise_reproducible_under_train_deterministic(tmp_path, monkeypatch, sub):
    from dr4sr_amd import _lib
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("DR4SR_CONFIG_DIR", os.path.join(ROOT, "configs"))
    try:
        a, _ = one_fit(fit_config(sub, True))
        assert os.environ.get("DR4SR_DETERMINISTIC") == "1"
        b, _ = one_fit(fit_config(sub, True))
    finally:
        _lib.set_env("DR4SR_DETERMINISTIC", None)
    assert len(a) == len(b) == 5 and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("sub", ["SASRec", "CL4SRec"])
def test_captured_weighted_step_is_bitwise_the_eager_one(tmp_path, monkeypatch, sub):
    """train.deterministic: the replayed graph of the weighted step (negatives, weighted fwd/bwd, Adam) leaves the bits of the same launches
    made eagerly from the same state, on the negatives the graph drew"""
    from dr4sr_amd import _lib
    monkeypatch.chdir(tmp_path)
    try:
        ds, model = build(fit_config(sub, True), monkeypatch)
        model.train()
        sub_m, eng = model.sub_model, model.engine
        loader = ds[0].get_loader()
        batch = model._local_batch(loader, model._perm(loader), 0)
        st, run = model._weighted_graph(batch)                      # warm-up + capture; every side effect undone
        keep = [eng.params, eng.adam_m, eng.adam_v] + list(getattr(eng, "states", [eng.state]))
        if model._cl_sub():
            keep.append(sub_m.augmentation_model.augmentation.step_dev)
        snap = [t.clone() for t in keep]
        run()
        torch.cuda.synchronize()
        got = [eng.grads.clone(), model._phi.grads.clone(), eng.params.clone()]
        for dst, src in zip(keep, snap):
            dst.copy_(src)
        model._weighted_fwd_bwd(st)                                 # st["neg_item"]: what the graph drew
        eng.adam_step(sub_m._api_plan())
        torch.cuda.synchronize()
        want = [eng.grads, model._phi.grads, eng.params]
        assert float(got[1].abs().max()) > 0 and not torch.equal(got[2], snap[0])
        for name, x, y in zip(("sub-model gradient", "phi gradient", "parameters after Adam"), got, want):
            assert torch.equal(x, y), name
    finally:
        _lib.set_env("DR4SR_DETERMINISTIC", None)
