"""SASRec's per-token input weight (the reference's model/sasrec.py:61-64) on the HIP path: dr4sr_sasrec_encode_w / _encode_w_bwd in
every launch form of the embedding stage, against tests/_inw_ref.py (the CPU restatement tests/test_input_weight_cpu.py pins to the
reference's recorded numbers) and against tests/golden/sasrec_input_weight.npz itself; then the model surface.

The engine-level batch is the smallest that can still go wrong: B = 7, L = 12, seqlen [12, 1, 5, 12, 3, 7, 9] -> T = 49 packed tokens =
three 16-token tiles plus one token (sequences straddle the tile boundaries, the 32-row tiles end in a partial one), one item id twice
inside a tile (the same-id merge of the dE scatter), one PAD id inside a valid range, weights with two exact zeros and a row of ones.

Bars (tests/test_gpu_parity.py's): max-abs error / max-abs reference < 5e-4 for gradients, 2e-4 for `out`."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _inw_ref as R  # noqa: E402
from oracle import sasrec_oracle as O  # noqa: E402

REL_OUT, REL_GRAD = 2e-4, 5e-4
N, B, L, H, F, NL, EPS = 40, 7, 12, 2, 128, 2, 1e-12
SEQLEN = [12, 1, 5, 12, 3, 7, 9]
ONES_ROW, ZEROS = 4, ((0, 3), (5, 6))

# launch forms of the embedding stage: environment, and what dr4sr_sasrec_at_scale must answer (bit 0: at-scale tiles, bit 2: attention inside
# the 16-row tile kernels, bit 6: deterministic latency form)
FORMS = {
    "latency": ({}, lambda b: not b & 1 and b & 4),                                  # k_embqkv_fwd<16, D>, embedding plane of k_wgrad_blk
    "at_scale": ({"DR4SR_FORCE_SCALE": "1"}, lambda b: b & 1),                       # d = 64: wave tiles; d = 128: 32-row tiles; gout plane
    "at_scale_no_wave_tiles": ({"DR4SR_FORCE_SCALE": "1", "DR4SR_NO_WAVE_TILES": "1"}, lambda b: b & 1),      # 32-row tiles at d = 64 too
    "no_fuse": ({"DR4SR_NO_FUSE": "1"}, lambda b: not b & 1 and not b & 4),          # k_embed_fwd / k_embed_bwd
    "qeb_separate": ({"DR4SR_QEB_SEPARATE": "1"}, lambda b: not b & 1 and b & 4),    # k_qkv_embed_bwd<16, D> as a launch of its own
    "deterministic": ({"DR4SR_DETERMINISTIC": "1"}, lambda b: b & 64),               # k_qkv_embed_bwd<16, D, DET>, ordered table jobs
}


def relerr(a, b):
    a = torch.as_tensor(a).detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    return float((a - b).abs().max() / max(1e-12, float(b.abs().max())))


def random_params(n_items, D, Ln, seed):
    from dr4sr_amd.engine import param_names, param_shapes
    gen = torch.Generator().manual_seed(seed)
    p = {}
    for n, s in zip(param_names(NL), param_shapes(n_items, Ln, D, F, NL)):
        if n.endswith("norm1.weight") or n.endswith("norm2.weight"):
            p[n] = 1.0 + 0.1 * torch.randn(s, generator=gen)
        elif "in_proj_weight" in n:
            p[n] = 0.15 * torch.randn(s, generator=gen)
        else:
            p[n] = 0.05 * torch.randn(s, generator=gen)
    p[R.TABLE][0] = 0
    p[R.TIED] = p[R.TABLE]
    return p


def small_batch():
    rng = np.random.default_rng(71)
    sl = np.array(SEQLEN, dtype=np.int64)
    idx = np.zeros((B, L), dtype=np.int64)
    for b in range(B):
        idx[b, :sl[b]] = rng.integers(1, N, size=sl[b])
    idx[0, 5] = idx[0, 2]                 # one id twice inside the first 16-token tile
    idx[3, 6] = 0                         # PAD inside a valid range (tokens 18..29: the second tile), not at position 0
    g = torch.Generator().manual_seed(72)
    w = 0.25 + 1.5 * torch.rand(B, L, generator=g)
    for b, l in ZEROS:
        assert l < sl[b]
        w[b, l] = 0.0
    w[ONES_ROW] = 1.0
    assert int(sl.sum()) == 49
    return torch.from_numpy(idx), torch.from_numpy(sl), w.contiguous()


@pytest.fixture(scope="module")
def case():
    """per D: parameters, the batch, d_out and the reference's (out, grads, d weight) at p = 0 — computed once, shared, left unchanged"""
    idx, sl, w = small_batch()
    out = {}
    for D in (64, 128):
        params = random_params(N, D, L, seed=13 + D)
        d_out = torch.randn(B, L, D, generator=torch.Generator().manual_seed(5 + D))
        ref = R.encode_grads(params, idx, sl, w.unsqueeze(-1), d_out, H, NL, EPS, "origin")
        out[D] = (params, d_out, ref)
    return idx, sl, w, out


def make_engine(params, D, p_drop=0.0, n_items=N, Ln=L, max_batch=B, seed=2023):
    from dr4sr_amd.engine import SasrecEngine
    eng = SasrecEngine(n_items, Ln, D, H, F, NL, EPS, p_drop, max_batch, "cuda", seed=seed)
    eng.load_named(params)
    return eng


def run(eng, idx, sl, w, d_out, training=False, want_dw=True):
    """-> (plan, out, {name: gradient}, d_input_weight) of encode + encode_bwd (origin pooling) with weight w (None: the old entry points)"""
    from dr4sr_amd import _lib
    plan = eng.make_plan(idx.cuda(), None, sl.cuda())
    wd = None if w is None else w.cuda().contiguous()
    out = eng.encode(plan, training, _lib.POOL_ORIGIN, input_weight=wd)
    eng.grads.zero_()
    dw = torch.zeros(idx.shape, dtype=torch.float32, device="cuda") if (want_dw and w is not None) else None
    eng.encode_bwd(plan, training, _lib.POOL_ORIGIN, d_out.cuda(), input_weight=wd, d_input_weight=dw)
    torch.cuda.synchronize()
    return plan, out, {k: v.clone() for k, v in eng.grad_views.items()}, dw


def check_against(out, grads, dw, ref, sl, tag):
    q_o, g_o, dw_o = ref
    fig = {"out": relerr(out, q_o), "d_input_weight": relerr(dw, dw_o.squeeze(-1))}
    for k, v in grads.items():
        fig[k] = relerr(v, g_o[k])
    worst = max((k for k in fig if k not in ("out", "d_input_weight")), key=lambda k: fig[k])
    print(f"{tag}: out {fig['out']:.2e}, d_input_weight {fig['d_input_weight']:.2e}, worst parameter gradient {fig[worst]:.2e} ({worst})")
    assert fig.pop("out") < REL_OUT
    for k, v in fig.items():
        assert v < REL_GRAD, (tag, k, v)
    dead = torch.arange(dw.shape[1]).view(1, -1) >= sl.view(-1, 1)
    assert bool((dw.cpu()[dead] == 0).all()), "d_input_weight at pos >= seqlen is exactly 0"
    assert float(grads[R.TABLE][0].abs().max()) == 0.0, "the PAD row takes no gradient"


# ------------------------------------------------------------------------------------------------ 1. every form, p = 0
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("form", list(FORMS))
def test_weighted_encode_and_backward_in_every_launch_form(case, monkeypatch, request, form, D):
    from dr4sr_amd import _lib
    idx, sl, w, per_d = case
    params, d_out, ref = per_d[D]
    env, expect = FORMS[form]
    if form == "at_scale":
        request.getfixturevalue("at_scale")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = make_engine(params, D)
    plan, out, grads, dw = run(eng, idx, sl, w, d_out)
    bits = int(_lib.load().dr4sr_sasrec_at_scale(C.byref(plan)))
    assert expect(bits), (form, bits)
    check_against(out, grads, dw, ref, sl, f"{form}/d{D}")
    # the weight reached the kernels: the unweighted call differs where the weight is not 1
    _, out0, _, _ = run(eng, idx, sl, None, d_out)
    assert relerr(out0, ref[0]) > 1e-2
    # without d_input_weight the parameter gradients are the same ones
    _, _, grads2, none = run(eng, idx, sl, w, d_out, want_dw=False)
    assert none is None
    for k, v in grads2.items():
        assert relerr(v, ref[1][k]) < REL_GRAD, k


# ------------------------------------------------------------------------------------------------ 2. train mode: the scale sits before the dropout
def masks_from_engine(eng, sl, D, step):
    """the library's own keep masks (dr4sr_dropout_mask), laid out densely for the oracle"""
    from dr4sr_amd import _lib
    cu = torch.cat([torch.zeros(1, dtype=torch.long), sl.cumsum(0)])
    T = int(cu[-1])
    masks = {O.SITE_EMB: eng.dropout_mask(B * L * D, _lib.SITE_EMB, step).view(B, L, D).cpu()}

    def dense(packed, width):
        m = torch.ones(B, L, width)
        for bi in range(B):
            n = int(sl[bi])
            m[bi, :n] = packed[int(cu[bi]):int(cu[bi]) + n]
        return m
    for l in range(NL):
        a = eng.dropout_mask(B * H * 64 * 64, _lib.SITE_ATTN + 4 * l, step).view(B, H, 64, 64)[:, :, :L, :L]
        masks[O.site(O.SITE_ATTN, l)] = a.cpu().contiguous()
        masks[O.site(O.SITE_PROJ, l)] = dense(eng.dropout_mask(T * D, _lib.SITE_PROJ + 4 * l, step).view(T, D).cpu(), D)
        masks[O.site(O.SITE_ACT, l)] = dense(eng.dropout_mask(T * F, _lib.SITE_ACT + 4 * l, step).view(T, F).cpu(), F)
        masks[O.site(O.SITE_FFN, l)] = dense(eng.dropout_mask(T * D, _lib.SITE_FFN + 4 * l, step).view(T, D).cpu(), D)
    return masks


@pytest.mark.parametrize("D", [64, 128])
def test_train_mode_scale_sits_before_the_dropout(case, D):
    idx, sl, w, per_d = case
    params, d_out, _ = per_d[D]
    p = 0.5
    eng = make_engine(params, D, p_drop=p, seed=4321)
    plan, out, grads, dw = run(eng, idx, sl, w, d_out, training=True)
    step = int(eng.state[3])
    assert step == 1
    masks = masks_from_engine(eng, sl, D, step)
    assert abs(float(masks[O.SITE_EMB].mean()) - (1 - p)) < 0.05
    ref = R.encode_grads(params, idx, sl, w.unsqueeze(-1), d_out, H, NL, EPS, "origin", masks=masks, pdrop=p)
    check_against(out, grads, dw, ref, sl, f"train/d{D}")


# ------------------------------------------------------------------------------------------------ 3. all-ones weight, in == NULL
def raw_encode(eng, plan, ins, training=0):
    from dr4sr_amd import _lib
    out = torch.empty(plan.B, L, eng.D, device="cuda")
    rc = eng.lib.dr4sr_sasrec_encode_w(C.byref(plan), None if ins is None else C.byref(ins), training, _lib.POOL_ORIGIN, _lib.ptr(out), _lib.cur_stream())
    return rc, out


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("det", [False, True])
def test_all_ones_weight_is_the_unweighted_call(case, monkeypatch, D, det):
    from dr4sr_amd import _lib
    idx, sl, w, per_d = case
    params, d_out, _ = per_d[D]
    if det:
        monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    eng = make_engine(params, D)
    ones = torch.ones(B, L)
    plan, out_w, g_w, dw = run(eng, idx, sl, ones, d_out)
    _, out_0, g_0, _ = run(eng, idx, sl, None, d_out)
    assert torch.equal(out_w, out_0), "weight 1: the forward output is bitwise dr4sr_sasrec_encode's"
    if det:
        for k in g_0:
            assert torch.equal(g_w[k], g_0[k]), k
    else:
        for k in g_0:
            assert relerr(g_w[k], g_0[k]) < 1e-5, k
    assert float(dw.abs().max()) > 0
    # in == NULL and in->input_weight == NULL are the old entry points: same bits, forward and (ordered mode) backward
    idx_d, sl_d = idx.cuda(), sl.cuda()                      # (a plan holds raw pointers: its tensors live here)
    plan = eng.make_plan(idx_d, None, sl_d)
    for ins in (None, _lib.SasrecInputs(None, None)):
        rc, out_n = raw_encode(eng, plan, ins)
        assert rc == 0 and torch.equal(out_n, out_0)
        eng.grads.zero_()
        rc = eng.lib.dr4sr_sasrec_encode_w_bwd(C.byref(plan), None if ins is None else C.byref(ins), 0, _lib.POOL_ORIGIN, _lib.ptr(d_out.cuda()),
                                               _lib.cur_stream())
        assert rc == 0
        torch.cuda.synchronize()
        for k, v in eng.grad_views.items():
            assert torch.equal(v, g_0[k]) if det else relerr(v, g_0[k]) < 1e-5, k


# ------------------------------------------------------------------------------------------------ 4. written, not accumulated
@pytest.mark.parametrize("form", ["latency", "at_scale", "no_fuse"])
def test_two_backward_calls_store_the_same_weight_gradient(case, monkeypatch, form):
    from dr4sr_amd import _lib
    idx, sl, w, per_d = case
    params, d_out, ref = per_d[64]
    for k, v in FORMS[form][0].items():
        monkeypatch.setenv(k, v)
    eng = make_engine(params, 64)
    plan = eng.make_plan(idx.cuda(), None, sl.cuda())
    wd, dw = w.cuda(), torch.zeros(B, L, device="cuda")
    eng.encode(plan, True, _lib.POOL_ORIGIN, input_weight=wd)
    eng.encode_bwd(plan, True, _lib.POOL_ORIGIN, d_out.cuda(), input_weight=wd, d_input_weight=dw)
    first = dw.clone()
    eng.encode_bwd(plan, True, _lib.POOL_ORIGIN, d_out.cuda(), input_weight=wd, d_input_weight=dw)
    torch.cuda.synchronize()
    assert float(first.abs().max()) > 0 and torch.equal(first, dw)
    assert relerr(dw, ref[2].squeeze(-1)) < REL_GRAD


# ------------------------------------------------------------------------------------------------ 5. argument errors
def test_weight_gradient_without_weight_is_an_argument_error(case):
    from dr4sr_amd import _lib
    idx, sl, w, per_d = case
    eng = make_engine(per_d[64][0], 64)
    plan = eng.make_plan(idx.cuda(), None, sl.cuda())
    dw = torch.zeros(B, L, device="cuda")
    ins = _lib.SasrecInputs(None, _lib.ptr(dw))
    rc, _ = raw_encode(eng, plan, ins)
    assert rc == -1                       # DR4SR_E_ARG
    d_out = torch.zeros(B, L, 64, device="cuda")
    assert eng.lib.dr4sr_sasrec_encode_w_bwd(C.byref(plan), C.byref(ins), 0, _lib.POOL_ORIGIN, _lib.ptr(d_out), _lib.cur_stream()) == -1
    with pytest.raises(_lib.Dr4srError, match="DR4SR_E_ARG"):
        eng.encode_bwd(plan, False, _lib.POOL_ORIGIN, d_out, d_input_weight=dw)
    with pytest.raises(_lib.Dr4srError, match="input_weight must be"):
        eng.encode(plan, False, _lib.POOL_ORIGIN, input_weight=torch.ones(B, L, 1, device="cuda"))
    assert float(dw.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 6. + 7. the reference's recorded numbers; the model
def make_config(n_items):
    return {
        "data": {"dataset": "synthetic-toys", "domain_name_list": ["toy"], "max_seq_len": 50, "dataset_class": "synthetic",
                 "train_file": "", "n_items": n_items, "n_rows": 64, "n_eval_rows": 16, "seed": 5},
        "model": {"model": "SASRec", "embed_dim": 64, "loss_fn": "bce", "hidden_size": 128, "layer_num": 2, "head_num": 2,
                  "dropout_rate": 0.0, "activation": "gelu", "layer_norm_eps": 1e-12},
        "train": {"batch_size": 8, "early_stop_mode": "max", "early_stop_patience": 20, "epochs": 1, "device": "cuda",
                  "optimizer": "adam", "learning_rate": 0.001, "weight_decay": 0, "num_neg": 1, "seed": 2023, "hip_graph": True},
        "eval": {"batch_size": 16, "cutoff": [20, 10], "val_metrics": ["ndcg", "recall"], "test_metrics": ["ndcg", "recall"],
                 "topk": 100, "save_path": "./saved/"},
    }


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = R.load_golden(golden_dir)
    assert (int(g["meta.embed_dim"]), int(g["meta.head_num"]), int(g["meta.hidden_size"]), int(g["meta.layer_num"])) == (64, H, F, NL)
    return g


@pytest.fixture(scope="module")
def model(golden):
    from dr4sr_amd.utils import prepare_datasets, prepare_model, seed_everything
    cfg = make_config(int(golden["meta.num_items"]))
    seed_everything(cfg["train"]["seed"])
    ds = prepare_datasets(cfg)
    m = prepare_model(cfg, ds)
    m._init_model(ds[0])
    m.load_state_dict({k: v for k, v in R.golden_params(golden).items()})
    return m


def test_engine_reproduces_the_reference_query(golden):
    from dr4sr_amd import _lib
    p, b = R.golden_params(golden), R.golden_batch(golden)
    Bg, Lg = b["in_item_id"].shape
    eng = make_engine(p, 64, n_items=int(golden["meta.num_items"]), Ln=Lg, max_batch=Bg)
    plan = eng.make_plan(b["in_item_id"].cuda(), None, b["seqlen"].cuda())
    w = torch.from_numpy(golden["weight"]).reshape(Bg, Lg).contiguous().cuda()
    out = eng.encode(plan, False, _lib.POOL_ORIGIN, input_weight=w)
    e = relerr(out, golden["out.query"])
    print("golden query", e)
    assert e < REL_OUT


def step(model, batch, w):
    model.train()
    model.optimizer.zero_grad()
    if model.item_embedding.weight.grad is not None:
        model.item_embedding.weight.grad.zero_()
    b = dict(batch)
    if w is not None:
        b["input_weight"] = w
    loss = model.training_step(b, reduce=True)
    loss.backward()
    torch.cuda.synchronize()
    return loss


def test_model_training_step_reproduces_the_reference(golden, model):
    batch = {k: v.cuda() for k, v in R.golden_batch(golden).items()}
    w = torch.from_numpy(golden["weight"]).cuda().requires_grad_(True)
    loss = step(model, batch, w)
    fig = {"loss": abs(float(loss.detach()) - float(golden["out.loss"])) / abs(float(golden["out.loss"]))}
    for n, p in model.named_parameters():
        fig[n] = relerr(p.grad, golden["grad." + n])
    fig["weight.grad"] = relerr(w.grad, golden["grad_weight"])
    worst = max((k for k in fig if k not in ("loss", "weight.grad")), key=lambda k: fig[k])
    print(f"golden step: loss {fig['loss']:.2e}, weight.grad {fig['weight.grad']:.2e}, worst parameter gradient {fig[worst]:.2e} ({worst})")
    assert fig.pop("loss") < 1e-5
    assert w.grad.shape == w.shape
    for k, v in fig.items():
        assert v < REL_GRAD, (k, v)
    Lg = w.shape[1]
    dead = (torch.arange(Lg).view(1, -1) >= batch["seqlen"].cpu().view(-1, 1))
    assert bool((w.grad.cpu()[..., 0][dead] == 0).all())


def test_model_weight_shapes_eval_none_and_refusals(golden, model):
    p, bc = R.golden_params(golden), R.golden_batch(golden)
    batch = {k: v.cuda() for k, v in bc.items()}
    Bg, Lg = bc["in_item_id"].shape
    # a [1, L, 1] weight: autograd's expand-backward makes its gradient the batch sum
    w1 = (0.5 + torch.rand(1, Lg, 1, generator=torch.Generator().manual_seed(3)))
    loss_o, _, g_o, gw_o = R.step_grads(p, bc, w1, H, NL, EPS)
    wd = w1.cuda().requires_grad_(True)
    loss = step(model, batch, wd)
    assert abs(float(loss) - float(loss_o)) < 1e-5 * abs(float(loss_o))
    assert wd.grad.shape == (1, Lg, 1) and relerr(wd.grad, gw_o) < REL_GRAD
    assert relerr(model.item_embedding.weight.grad, g_o[R.TABLE]) < REL_GRAD
    # eval forward: 'last' pooling with the weight
    wB = torch.from_numpy(golden["weight"])
    model.eval()
    with torch.no_grad():
        q = model.forward({**batch, "input_weight": wB.cuda()})
        q_none = model.forward({**batch, "input_weight": None})
        q_absent = model.forward(batch)
    q_o = R.encode(p, bc["in_item_id"], bc["seqlen"], wB, H, NL, EPS, "last")
    assert q.shape == (Bg, 64) and relerr(q, q_o) < REL_OUT
    assert torch.equal(q_none, q_absent) and relerr(q_absent, q_o) > 1e-3, "input_weight = None is an absent key"
    # refusals
    with pytest.raises(NotImplementedError, match=r"\[B, L, 1\]"):
        model.forward({**batch, "input_weight": torch.ones(Bg, Lg, 64, device="cuda")})
    with pytest.raises(NotImplementedError, match="seq_emb"):
        model.forward({**batch, "seq_emb": torch.zeros(Bg, Lg, 64, device="cuda")})
    model.train()
