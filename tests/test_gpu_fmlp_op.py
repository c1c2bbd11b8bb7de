"""torch.ops.dr4sr_hip.fmlp_layer / layer_norm (csrc/fmlp_op.hip) and dr4sr_amd.module.layers.FMLPOps / FMLPEncoderOps on the GPU.

Yardsticks: tests/_fmlp_layer_ref.py in float64 (the reference's rfft / irfft form; pinned to the oracle by tests/test_fmlp_op_cpu.py), the
FMLP engine on the same parameters, and the reference's recorded numbers (tests/golden/fmlp_d64.npz).  Bars: max-abs error / max-abs
reference < 2e-4 for outputs, < 3e-4 for gradients (tests/test_gpu_fmlp_scale.py's).

Inputs: 0.05 randn weights, 1 + 0.05 randn LayerNorm weights, x = randn with one all-zero row.  Every case prints its worst figure
(pytest -s); NOTEBOOK.md records them."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import dr4sr_amd.ops  # noqa: E402,F401  (registers torch.ops.dr4sr_hip.*)
import _fmlp_layer_ref as LR  # noqa: E402
import _fmlp_ref as FR  # noqa: E402
from oracle import fmlp_oracle as FO  # noqa: E402

REL_OUT, REL_GRAD = 2e-4, 3e-4
EPS = 1e-12
SLOTS = 256                     # gradient slots of a backward launch (csrc/fmlp_op.hip MAX_SLOTS)


def relerr(a, b):
    a = torch.as_tensor(a).detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    return float((a - b).abs().max() / max(1e-12, float(b.abs().max())))


def layer_tensors(leaf, i):
    return [leaf[LR.prefix(i) + n] for n in LR.LAYER_TENSORS]


def run_op(x, p, d_out, n_layer=1, p_drop=0.0, seed=7, step=1, backward_twice=False):
    """the op chain on the GPU through autograd -> (y, dx, {name: gradient}) [, the same from a second backward of the same forward]"""
    xd = x.cuda().requires_grad_(True)
    leaf = {k: v.cuda().requires_grad_(True) for k, v in p.items()}
    y = xd
    for i in range(n_layer):
        y, _ = torch.ops.dr4sr_hip.fmlp_layer(y, *layer_tensors(leaf, i), EPS, p_drop, seed, step, i)
    names = list(leaf)

    def backward():
        gs = torch.autograd.grad(y, [xd] + [leaf[k] for k in names], d_out.cuda(), retain_graph=True)
        return gs[0], dict(zip(names, gs[1:]))
    dx, g = backward()
    if backward_twice:
        return y.detach(), dx, g, backward()
    return y.detach(), dx, g


def check(tag, got, ref):
    (y, dx, g), (y_o, dx_o, g_o) = got, ref
    for t in (y, dx, *g.values()):
        assert bool(torch.isfinite(t).all()), tag
    fig = {"y": relerr(y, y_o), "dx": relerr(dx, dx_o)}
    assert set(g) == set(g_o)
    for k in g_o:
        fig[k] = relerr(g[k], g_o[k])
    worst = max((k for k in fig if k != "y"), key=lambda k: fig[k])
    print(f"{tag}: y {fig['y']:.2e}, worst gradient {fig[worst]:.2e} ({worst})")
    assert fig.pop("y") < REL_OUT, tag
    bad = "; ".join(f"{k} {v:.2e}" for k, v in fig.items() if not v < REL_GRAD)
    assert not bad, f"{tag}: at or above {REL_GRAD:g}: {bad}"


@functools.lru_cache(maxsize=None)
def case(B, L, NL):
    """parameters, x, d_out and the float64 result — built once per shape, shared, left unchanged"""
    p = LR.layer_params(NL, L, seed=500 + 3 * L + NL)
    x = LR.make_x(B, L, seed=600 + B + L)
    d_out = torch.randn(B, L, 64, generator=torch.Generator().manual_seed(700 + B + L))
    return p, x, d_out, LR.layer_grads(x, p, d_out, NL)


# ------------------------------------------------------------------------------------------------ 1. every even L
@pytest.mark.parametrize("L", list(range(2, 65, 2)))
def test_every_even_length_matches_float64(L):
    """L = 2 has only DC and Nyquist, 50 is the reference's length, 64 the upper edge, 10 and 22 are no multiples of 16"""
    p, x, d_out, ref = case(3, L, 1)
    got = run_op(x, p, d_out)
    check(f"L={L}", got, ref)
    g = got[2][LR.prefix(0) + "filterlayer.complex_weight"]
    assert float(g[0, 0, :, 1].abs().max()) == 0.0 and float(g[0, L // 2, :, 1].abs().max()) == 0.0, "imaginary DC / Nyquist take no gradient"


# ------------------------------------------------------------------------------------------------ 2. batch shapes
@pytest.mark.parametrize("B", [1, 5, SLOTS + 44])
def test_batch_shapes_with_two_layers_match_float64(B):
    """B = 300: more sequences than gradient slots, a workgroup owns two"""
    p, x, d_out, ref = case(B, 50, 2)
    check(f"B={B}", run_op(x, p, d_out, 2), ref)


# ------------------------------------------------------------------------------------------------ 3. train mode
def library_mask(n, p, seed, step, site):
    from dr4sr_amd import _lib
    out = torch.empty(n, device="cuda")
    _lib.check(_lib.load().dr4sr_dropout_mask(_lib.ptr(out), n, p, seed, step, site, _lib.cur_stream()), "dr4sr_dropout_mask")
    return out.cpu()


def library_masks(B, L, n_layer, p, seed, step, emb=False):
    """the keep masks of dr4sr_dropout_mask in the element order include/dr4sr_hip.h documents: e = (b L + pos) D + c"""
    m = {}
    if emb:
        m[FO.SITE_EMB] = library_mask(B * L * 64, p, seed, step, 0).view(B, L, 64)
    for l in range(n_layer):
        m[FO.site(FO.SITE_FILT, l)] = library_mask(B * L * 64, p, seed, step, 1 + 2 * l).view(B, L, 64)
        m[FO.site(FO.SITE_FFN, l)] = library_mask(B * L * 64, p, seed, step, 2 + 2 * l).view(B, L, 64)
    return m


def test_train_mode_runs_under_the_documented_masks():
    B, L, NL, pd, seed, step = 5, 50, 2, 0.5, 4321, 3
    p, x, d_out, ref_eval = case(B, L, NL)
    masks = library_masks(B, L, NL, pd, seed, step)
    assert abs(float(masks[FO.site(FO.SITE_FFN, 1)].mean()) - (1 - pd)) < 0.05
    ref = LR.layer_grads(x, p, d_out, NL, EPS, masks, pd)
    got = run_op(x, p, d_out, NL, pd, seed, step)
    check("train", got, ref)
    again = run_op(x, p, d_out, NL, pd, seed, step)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1]), "the same (seed, step, layer): the same bits"
    other = run_op(x, p, d_out, NL, pd, seed, step + 1)
    assert relerr(other[0], got[0]) > 1e-2, "another step: other masks"
    assert relerr(ref_eval[0], got[0]) > 1e-2


# ------------------------------------------------------------------------------------------------ 4. repeatability, written not accumulated
@pytest.mark.parametrize("B", [5, SLOTS + 44])
def test_two_backward_calls_return_the_same_bits_and_outputs_are_written(B):
    from dr4sr_amd import _lib
    L = 50
    p, x, d_out, ref = case(B, L, 2)
    p1 = {k: v for k, v in p.items() if k.startswith(LR.prefix(0))}
    y, dx, gr, (dx2, gr2) = run_op(x, p1, d_out, 1, backward_twice=True)
    assert torch.equal(dx, dx2) and float(dx.abs().max()) > 0
    for k in gr:
        assert torch.equal(gr[k], gr2[k]) and float(gr[k].abs().max()) > 0, k
    # through the C ABI into garbage-filled outputs: the same bits
    lib = _lib.load()
    xd, dyd = x.cuda(), d_out.cuda()
    w = [p1[LR.prefix(0) + n].cuda() for n in LR.LAYER_TENSORS]
    n_saved = int(lib.dr4sr_fmlp_layer_saved_floats(B, L, 64, 256))
    nb0, nb1 = (int(lib.dr4sr_fmlp_layer_workspace_bytes(B, L, 64, 256, k)) for k in (0, 1))
    saved = torch.full((n_saved,), float("nan"), device="cuda")
    ws = torch.full((nb1 // 4,), float("nan"), device="cuda")
    y2 = torch.full_like(xd, float("nan"))
    ws_struct = _lib.FmlpLayerWeights(*[_lib.ptr(t) for t in w])
    _lib.check(lib.dr4sr_fmlp_layer_fwd(_lib.ptr(xd), ws_struct, B, L, 64, 256, EPS, 0.0, 7, 1, 0, _lib.ptr(y2), _lib.ptr(saved), _lib.ptr(ws), nb0,
                                        _lib.cur_stream()), "fwd")
    assert torch.equal(y2, y)
    dx3 = torch.full_like(xd, 1e30)
    dws = [torch.full_like(t, -1e30) for t in w]
    _lib.check(lib.dr4sr_fmlp_layer_bwd(_lib.ptr(xd), ws_struct, B, L, 64, 256, EPS, 0.0, 7, 1, 0, _lib.ptr(saved), _lib.ptr(dyd), _lib.ptr(dx3),
                                        _lib.FmlpLayerGrads(*[_lib.ptr(t) for t in dws]), _lib.ptr(ws), nb1, _lib.cur_stream()), "bwd")
    assert torch.equal(dx3, dx)
    for n, t in zip(LR.LAYER_TENSORS, dws):
        assert torch.equal(t, gr[LR.prefix(0) + n]), n
    # a workspace one byte short is refused before any launch
    assert lib.dr4sr_fmlp_layer_bwd(_lib.ptr(xd), ws_struct, B, L, 64, 256, EPS, 0.0, 7, 1, 0, _lib.ptr(saved), _lib.ptr(dyd), _lib.ptr(dx3),
                                    _lib.FmlpLayerGrads(*[_lib.ptr(t) for t in dws]), _lib.ptr(ws), nb1 - 1, _lib.cur_stream()) == -3
    assert lib.dr4sr_fmlp_layer_fwd(_lib.ptr(xd), ws_struct, B, L, 64, 256, EPS, 0.0, 7, 1, 0, _lib.ptr(y2), None, None, 0, _lib.cur_stream()) == -3


# ------------------------------------------------------------------------------------------------ 5. B = 0
def test_empty_batch_launches_nothing_and_zero_fills_the_weight_gradients():
    L = 50
    w = [v.cuda() for v in LR.layer_params(1, L, seed=1).values()]
    x = torch.empty(0, L, 64, device="cuda")
    o = torch.ops.dr4sr_hip
    y, saved = o.fmlp_layer(x, *w, EPS, 0.5, 7, 1, 0)
    assert y.shape == (0, L, 64)
    gs = o.fmlp_layer_backward(x, *w, EPS, 0.5, 7, 1, 0, saved, torch.empty(0, L, 64, device="cuda"))
    assert gs[0].shape == (0, L, 64) and len(gs) == 10
    for g, t in zip(gs[1:], w):
        assert g.shape == t.shape and float(g.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 6. layer_norm
@pytest.mark.parametrize("shape", [(7, 64), (300 * 50, 64)])
def test_layer_norm_op_matches_float64_and_repeats_its_bits(shape):
    g = torch.Generator().manual_seed(shape[0])
    x = torch.randn(shape, generator=g)
    x[3] = 0                                                # an all-zero row: y = bias there
    w, b = 1 + 0.05 * torch.randn(64, generator=g), 0.05 * torch.randn(64, generator=g)
    d_out = torch.randn(shape, generator=g)
    y_o, dx_o, dw_o, db_o = LR.layer_norm_grads(x, w, b, d_out)
    xd, wd, bd = (t.cuda().requires_grad_(True) for t in (x, w, b))
    y = torch.ops.dr4sr_hip.layer_norm(xd, wd, bd, EPS)
    outs = [torch.autograd.grad(y, [xd, wd, bd], d_out.cuda(), retain_graph=True) for _ in range(2)]
    for a, c in zip(*outs):
        assert torch.equal(a, c)
    dx, dw, db = outs[0]
    rest = torch.arange(shape[0]) != 3                      # the zero row's dx is 1e6 times the others': look at the others on their own too
    fig = {"y": relerr(y, y_o), "dx": relerr(dx, dx_o), "dx (other rows)": relerr(dx.cpu()[rest], dx_o[rest]), "dw": relerr(dw, dw_o),
           "db": relerr(db, db_o)}
    print(f"layer_norm {shape}: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert torch.equal(y.detach()[3].cpu(), b), "the all-zero row normalises to the bias"
    assert fig.pop("y") < REL_OUT
    for k, v in fig.items():
        assert v < REL_GRAD, (k, v)


# ------------------------------------------------------------------------------------------------ 7. against the engine
def op_chain(leaf, idx, NL, p_drop, seed, step):
    o = torch.ops.dr4sr_hip
    x = o.embed_gather_posadd(leaf[FR.TABLE], leaf["position_embeddings.weight"], idx)
    x = o.layer_norm(x, leaf["LayerNorm.weight"], leaf["LayerNorm.bias"], EPS)
    if p_drop > 0:
        x = o.dropout(x, p_drop, seed, step, 0)
    for i in range(NL):
        x, _ = o.fmlp_layer(x, *layer_tensors(leaf, i), EPS, p_drop, seed, step, i)
    return x[:, -1]


def test_op_chain_against_the_engine():
    from dr4sr_amd.fmlp_engine import FmlpEngine
    B, L, NL, N, pd, seed = 29, 50, 2, 150, 0.5, 31
    params, idx, _, _ = FR.make_case(B, L, NL, N, seed=77)
    d_out = torch.randn(B, 64, generator=torch.Generator().manual_seed(78))
    eng = FmlpEngine(N, L, 64, 256, NL, EPS, pd, B, "cuda", seed=seed)
    eng.load_named(params)
    idx_d, d_out_d = idx.cuda(), d_out.cuda()
    plan = eng.make_plan(idx_d, None)                       # rows = None

    def engine_backward(training):
        eng.grads.zero_()
        eng.encode_bwd(plan, training, d_out_d)
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in eng.grad_views.items()}

    def compare(tag, training, step):
        leaf = {k: v.cuda().requires_grad_(True) for k, v in params.items()}
        out = op_chain(leaf, idx_d, NL, pd if training else 0.0, seed, step)
        names = list(leaf)
        gs = dict(zip(names, torch.autograd.grad(out, [leaf[k] for k in names], d_out_d)))
        g_e = engine_backward(training)
        fig = {k: relerr(gs[k], g_e[k]) for k in g_e}
        worst = max(fig, key=lambda k: fig[k])
        print(f"engine/{tag}: out {relerr(out, out_e):.2e}, worst parameter gradient {fig[worst]:.2e} ({worst})")
        assert set(fig) == set(names)
        assert relerr(out, out_e) < REL_OUT
        for k, v in fig.items():
            assert v < REL_GRAD, (tag, k, v)
        assert float(gs[FR.TABLE][0].abs().max()) == 0.0, "the PAD row takes no gradient"
        return out

    out_e = eng.encode(plan, False)
    out_eval = compare("eval", False, 0)
    # train mode: the engine advances its RNG step word FIRST and draws this call's masks with the new value, keyed (seed, step, site,
    # (b L + pos) D + c) on a plan without rows — the op chain is handed that value
    before = int(eng.state[3])
    out_e = eng.encode(plan, True)
    step = int(eng.state[3])
    assert step == before + 1
    out_train = compare("train", True, step)
    assert relerr(out_train, out_eval) > 1e-2


# ------------------------------------------------------------------------------------------------ 8. the reference's recorded numbers
def test_module_reproduces_the_reference_training_step(golden_dir):
    import test_gpu_fmlp as TF
    from dr4sr_amd.module.layers import FMLPOps
    g, params, b = TF.load(golden_dir)
    N, NL = int(g["meta.num_items"]), int(g["meta.layer_num"])
    B, L = b["in_item_id"].shape
    table = torch.nn.Embedding(N, 64, padding_idx=0)
    m = FMLPOps(table, NL, max_seq_len=L, dropout=0.5, layer_norm_eps=EPS, seed=2023)
    m.load_state_dict(params, strict=True)                  # an FMLP checkpoint as it is
    m = m.cuda().eval()
    batch = {k: v.cuda() for k, v in b.items()}
    q = m(batch)
    assert q.shape == (B, 64) and m.step == 0
    lp, st = torch.ops.dr4sr_hip.score_bce(q, m.item_embedding.weight, batch["item_id"], batch["neg_item"].view(-1).contiguous())
    loss = lp.sum() / st[0]
    loss.backward()
    e_q, e_l = relerr(q, g["out.query"]), abs(float(loss.detach()) - float(g["out.loss"]))
    grads = {n: t.grad for n, t in m.named_parameters()}
    assert set(grads) == set(params)
    fig = {k: relerr(v, g["grad." + k]) for k, v in grads.items()}
    worst = max(fig, key=lambda k: fig[k])
    print(f"golden: query {e_q:.2e}, loss difference {e_l:.2e}, worst gradient {fig[worst]:.2e} ({worst})")
    assert int(st[0]) == B and e_q < TF.REL and e_l < 1e-5
    for k, v in fig.items():
        assert v < TF.REL, (k, v)
    # train mode: the step advances, the masks are the documented ones (site 0 for the embedding dropout)
    m.train()
    with torch.no_grad():
        a = m(batch)
        c = m(batch)
        m.step = 0
        a2 = m(batch)
        full = m(batch, need_pooling=False)
    assert m.step == 2 and torch.equal(a, a2) and relerr(c, a) > 1e-2 and full.shape == (B, L, 64)
    masks = library_masks(B, L, NL, 0.5, m.seed, 0, emb=True)
    p64 = {k: v.double() for k, v in params.items()}
    ref = FO.fmlp_encode(p64, b["in_item_id"], NL, EPS, masks, 0.5, use_fft=True)
    e = relerr(a, ref)
    print(f"golden parameters, train mode: query {e:.2e}")
    assert e < REL_OUT
    no_emb = {k: v for k, v in masks.items() if k != FO.SITE_EMB}
    assert relerr(a, FO.fmlp_encode(p64, b["in_item_id"], NL, EPS, no_emb, 0.5, use_fft=True)) > 1e-2, "the embedding mask is applied"


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_unsupported_shapes_are_refused_before_any_launch():
    from dr4sr_amd._lib import Dr4srError
    o = torch.ops.dr4sr_hip

    def call(L, D=64, cw_shape=None):
        shapes = [(1, L // 2 + 1, D, 2), (D,), (D,), (4 * D, D), (4 * D,), (D, 4 * D), (D,), (D,), (D,)]
        if cw_shape:
            shapes[0] = cw_shape
        w = [torch.zeros(s, device="cuda") for s in shapes]
        x = torch.zeros(2, L, D, device="cuda")
        return x, w
    for kw in ({"L": 49}, {"L": 66}, {"L": 50, "D": 128}, {"L": 50, "cw_shape": (1, 25, 64, 2)}, {"L": 50, "cw_shape": (26, 64, 2)}):
        x, w = call(**kw)
        with pytest.raises(Dr4srError):
            o.fmlp_layer(x, *w, EPS, 0.0, 7, 1, 0)
        with pytest.raises(Dr4srError):
            o.fmlp_layer_backward(x, *w, EPS, 0.0, 7, 1, 0, torch.zeros(8, device="cuda"), torch.zeros_like(x))
    x, w = call(50)
    for bad in ({"p": 1.0}, {"p": -0.1}, {"eps": -1.0}, {"layer": 1025}):
        with pytest.raises(Dr4srError):
            o.fmlp_layer(x, *w, bad.get("eps", EPS), bad.get("p", 0.0), 7, 1, bad.get("layer", 0))
    with pytest.raises(Dr4srError):
        o.layer_norm(torch.zeros(4, 66, device="cuda"), torch.zeros(66, device="cuda"), torch.zeros(66, device="cuda"), EPS)


# ------------------------------------------------------------------------------------------------ 10. graph capture
def test_captured_graph_replays_to_the_eager_bits():
    B, L, NL = 5, 50, 2
    p, x, d_out, _ = case(B, L, NL)
    p = {k: v.cuda() for k, v in p.items()}
    g = torch.Generator().manual_seed(55)
    x, d_out = x.cuda(), d_out.cuda()
    lw, lb = (1 + 0.05 * torch.randn(64, generator=g)).cuda(), (0.05 * torch.randn(64, generator=g)).cuda()
    o = torch.ops.dr4sr_hip

    def fwd_bwd():
        """forward and backward as one chain of op calls (the backward ops by hand: no autograd engine thread inside the capture)"""
        ys, saved = [o.layer_norm(x, lw, lb, EPS)], []
        for i in range(NL):
            y, s = o.fmlp_layer(ys[-1], *layer_tensors(p, i), EPS, 0.5, 9, 2, i)
            ys.append(y)
            saved.append(s)
        dy, grads = d_out, []
        for i in reversed(range(NL)):
            gs = o.fmlp_layer_backward(ys[i], *layer_tensors(p, i), EPS, 0.5, 9, 2, i, saved[i], dy)
            dy = gs[0]
            grads += gs[1:]
        return [ys[-1]] + list(o.layer_norm_backward(x, lw, EPS, dy)) + grads

    eager = [t.clone() for t in fwd_bwd()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fwd_bwd()                                           # warm-up on the capture stream (allocator, LDS opt-in)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = fwd_bwd()
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert len(captured) == 4 + 9 * NL
    for a, b in zip(captured, eager):
        assert torch.equal(a, b) and float(b.abs().max()) > 0
