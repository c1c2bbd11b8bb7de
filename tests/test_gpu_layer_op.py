"""torch.ops.dr4sr_hip.sasrec_layer / seq_pool / dropout (csrc/layer_op.hip) and dr4sr_amd.module.layers.SASRecQueryEncoderOps on the GPU.

Yardsticks: tests/_layer_ref.py (oracle.sasrec_oracle.sasrec_layer restated with a general mask; bit-equal to the oracle when causal,
tests/test_layer_op_cpu.py), the engine's packed encoder on the same parameters, and the reference's recorded numbers
(tests/golden/sasrec_input_weight.npz).  Bars (tests/test_gpu_parity.py's): max-abs error / max-abs reference < 2e-4 for outputs, < 5e-4 for
gradients.

The every-edge batch is B = 5, L = 12, H = 2 with the rows: no padding | only key 0 valid | post-padded at 5 | a padded key at position 6
inside a valid range | every key padded (no query of that row admits a key: a zero attention context, finite everywhere)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import dr4sr_amd.ops  # noqa: E402,F401  (registers torch.ops.dr4sr_hip.*)
import _inw_ref as R  # noqa: E402
import _layer_ref as LR  # noqa: E402
from oracle import sasrec_oracle as O  # noqa: E402

REL_OUT, REL_GRAD = 2e-4, 5e-4
H, EPS = 2, 1e-12


def relerr(a, b):
    a = torch.as_tensor(a).detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    return float((a - b).abs().max() / max(1e-12, float(b.abs().max())))


def edge_key_pad():
    kp = torch.zeros(5, 12, dtype=torch.bool)
    kp[1, 1:] = True
    kp[2, 5:] = True
    kp[3, 6] = True
    kp[4, :] = True
    return kp


def run_op(x, key_pad, p, causal, d_out, n_layer=1, p_drop=0.0, seed=7, step=1, backward_twice=False):
    """the op chain on the GPU through autograd -> (y, dx, {name: gradient}) [, the same from a second backward of the same forward]"""
    xd = x.cuda().requires_grad_(True)
    leaf = {k: v.cuda().requires_grad_(True) for k, v in p.items()}
    kp = None if key_pad is None else key_pad.cuda()
    y = xd
    for i in range(n_layer):
        w = [leaf[f"layers.{i}.{n}"] for n in LR.LAYER_TENSORS]
        y, _ = torch.ops.dr4sr_hip.sasrec_layer(y, kp, causal, *w, H, EPS, p_drop, seed, step, i)
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
    for k in g_o:
        fig[k] = relerr(g[k], g_o[k])
    worst = max((k for k in fig if k != "y"), key=lambda k: fig[k])
    print(f"{tag}: y {fig['y']:.2e}, worst gradient {fig[worst]:.2e} ({worst})")
    assert fig.pop("y") < REL_OUT, tag
    for k, v in fig.items():
        assert v < REL_GRAD, (tag, k, v)


# ------------------------------------------------------------------------------------------------ 1. every edge, p = 0
@pytest.mark.parametrize("D,F,causal,masked", [(64, 128, True, True), (64, 128, False, True), (128, 128, True, True), (128, 128, False, True),
                                               (64, 128, False, False), (64, 128, True, False), (64, 256, True, True)])
def test_every_edge_batch_matches_the_helper(D, F, causal, masked):
    B, L = 5, 12
    g = torch.Generator().manual_seed(100 + D + F)
    p = LR.layer_params(D, F, 1, seed=11 + D)
    x = torch.randn(B, L, D, generator=g)
    d_out = torch.randn(B, L, D, generator=g)
    kp = edge_key_pad() if masked else None
    ref = LR.layer_grads(x, kp, p, H, EPS, causal, d_out)
    got = run_op(x, kp, p, causal, d_out)
    check(f"edge/d{D}/f{F}/causal{int(causal)}/mask{int(masked)}", got, ref)
    if masked:                                              # the row without an admissible key: LayerNorm of the remaining terms, not NaN
        assert bool(torch.isfinite(got[0][4]).all()) and float(got[0][4].abs().max()) > 0


@pytest.mark.parametrize("L", [50, 64])
@pytest.mark.parametrize("D", [64, 128])
def test_long_rows_a_non_multiple_of_16_and_the_upper_edge(D, L):
    B, F = 2, 128
    g = torch.Generator().manual_seed(L + D)
    p = LR.layer_params(D, F, 1, seed=5 + D)
    x = torch.randn(B, L, D, generator=g)
    d_out = torch.randn(B, L, D, generator=g)
    kp = torch.zeros(B, L, dtype=torch.bool)
    kp[1, 37:] = True
    for causal in (True, False):
        check(f"long/d{D}/L{L}/causal{int(causal)}", run_op(x, kp, p, causal, d_out), LR.layer_grads(x, kp, p, H, EPS, causal, d_out))


# ------------------------------------------------------------------------------------------------ 2. train mode
def library_masks(B, L, D, F, n_layer, p, seed, step):
    """the keep masks of dr4sr_dropout_mask in the element order include/dr4sr_hip.h documents for the op"""
    from dr4sr_amd import _lib
    lib = _lib.load()

    def mask(n, site):
        out = torch.empty(n, device="cuda")
        _lib.check(lib.dr4sr_dropout_mask(_lib.ptr(out), n, p, seed, step, site, _lib.cur_stream()), "dr4sr_dropout_mask")
        return out.cpu()
    m = {}
    for l in range(n_layer):
        m[O.site(O.SITE_ATTN, l)] = mask(B * H * L * L, _lib.SITE_ATTN + 4 * l).view(B, H, L, L)
        m[O.site(O.SITE_PROJ, l)] = mask(B * L * D, _lib.SITE_PROJ + 4 * l).view(B, L, D)
        m[O.site(O.SITE_ACT, l)] = mask(B * L * F, _lib.SITE_ACT + 4 * l).view(B, L, F)
        m[O.site(O.SITE_FFN, l)] = mask(B * L * D, _lib.SITE_FFN + 4 * l).view(B, L, D)
    return m


@pytest.mark.parametrize("D", [64, 128])
def test_train_mode_runs_under_the_documented_masks(D):
    B, L, F, NL, pd, seed, step = 5, 12, 128, 2, 0.5, 4321, 3
    g = torch.Generator().manual_seed(D)
    p = LR.layer_params(D, F, NL, seed=21 + D)
    x = torch.randn(B, L, D, generator=g)
    d_out = torch.randn(B, L, D, generator=g)
    kp = edge_key_pad()
    masks = library_masks(B, L, D, F, NL, pd, seed, step)
    assert abs(float(masks[O.site(O.SITE_ATTN, 1)].mean()) - (1 - pd)) < 0.05
    ref = LR.layer_grads(x, kp, p, H, EPS, True, d_out, NL, masks, pd)
    got = run_op(x, kp, p, True, d_out, NL, pd, seed, step)
    check(f"train/d{D}", got, ref)
    again = run_op(x, kp, p, True, d_out, NL, pd, seed, step)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1]), "the same (seed, step, layer): the same bits"
    other = run_op(x, kp, p, True, d_out, NL, pd, seed, step + 1)
    assert relerr(other[0], got[0]) > 1e-2, "another step: other masks"
    eval_ = run_op(x, kp, p, True, d_out, NL, 0.0, seed, step)
    assert relerr(eval_[0], got[0]) > 1e-2


# ------------------------------------------------------------------------------------------------ 3. repeatability
@pytest.mark.parametrize("B", [5, 300])
def test_two_backward_calls_return_the_same_bits(B):
    """B = 300 is more sequences than workgroups of the backward launch: a workgroup adds its second sequence onto its partial slot"""
    L, D, F = 12, 64, 128
    g = torch.Generator().manual_seed(B)
    p = LR.layer_params(D, F, 1, seed=31)
    x = torch.randn(B, L, D, generator=g)
    d_out = torch.randn(B, L, D, generator=g)
    kp = (torch.rand(B, L, generator=g) < 0.3)
    kp[:, 0] = False
    y, dx, gr, (dx2, gr2) = run_op(x, kp, p, False, d_out, backward_twice=True)
    assert torch.equal(dx, dx2) and float(dx.abs().max()) > 0
    for k in gr:
        assert torch.equal(gr[k], gr2[k]), k
    check(f"repeat/B{B}", (y, dx, gr), LR.layer_grads(x, kp, p, H, EPS, False, d_out))


def test_empty_batch_launches_nothing_and_zero_fills_the_weight_gradients():
    D, F, L = 64, 128, 12
    w = [v.cuda() for v in LR.layer_params(D, F, 1, seed=1).values()]
    x = torch.empty(0, L, D, device="cuda")
    o = torch.ops.dr4sr_hip
    y, saved = o.sasrec_layer(x, None, True, *w, H, EPS, 0.5, 7, 1, 0)
    assert y.shape == (0, L, D)
    gs = o.sasrec_layer_backward(x, None, True, *w, H, EPS, 0.5, 7, 1, 0, saved, torch.empty(0, L, D, device="cuda"))
    assert gs[0].shape == (0, L, D) and len(gs) == 13
    for g, t in zip(gs[1:], w):
        assert g.shape == t.shape and float(g.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 4. seq_pool
@pytest.mark.parametrize("pooling", ["origin", "last", "mean"])
def test_seq_pool_and_its_backward(pooling):
    from dr4sr_amd import _lib
    code = {"origin": _lib.POOL_ORIGIN, "last": _lib.POOL_LAST, "mean": _lib.POOL_MEAN}[pooling]
    B, L, D = 4, 12, 64
    sl = torch.tensor([12, 1, 5, 0])
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, L, D, generator=g)
    xo = x.clone().requires_grad_(True)
    ref = LR.pool(xo, sl, pooling)
    d_out = torch.randn(ref.shape, generator=g)
    ref.backward(d_out)
    xd = x.cuda().requires_grad_(True)
    out = torch.ops.dr4sr_hip.seq_pool(xd, sl.cuda(), code)
    out.backward(d_out.cuda())
    assert out.shape == ref.shape and float(out.detach()[3].abs().max()) == 0.0, "seqlen 0 pools to zeros"
    if pooling == "mean":
        assert relerr(out, ref) < 1e-6 and relerr(xd.grad, xo.grad) < 1e-6
    else:
        assert torch.equal(out.cpu(), ref.detach()) and torch.equal(xd.grad.cpu(), xo.grad)
    assert float(xd.grad[3].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 5. against the engine
@pytest.mark.parametrize("D", [64, 128])
def test_op_chain_against_the_engine(D):
    import test_gpu_input_weight as TI
    from dr4sr_amd import _lib
    idx, sl, _ = TI.small_batch()
    params = TI.random_params(TI.N, D, TI.L, seed=13 + D)
    d_out = torch.randn(TI.B, TI.L, D, generator=torch.Generator().manual_seed(5 + D))
    eng = TI.make_engine(params, D)
    _, out_e, g_e, _ = TI.run(eng, idx, sl, None, d_out)
    leaf = {k: v.cuda().requires_grad_(True) for k, v in params.items() if k != R.TIED}
    o = torch.ops.dr4sr_hip
    x = o.embed_gather_posadd(leaf[R.TABLE], leaf["query_encoder.position_emb.weight"], idx.cuda())
    for i in range(TI.NL):
        w = [leaf[O.layer_prefix(i) + n] for n in LR.LAYER_TENSORS]
        x, _ = o.sasrec_layer(x, (idx == 0).cuda(), True, *w, H, EPS, 0.0, 7, 0, i)
    out = o.seq_pool(x, sl.cuda(), _lib.POOL_ORIGIN)
    names = list(leaf)
    gs = dict(zip(names, torch.autograd.grad(out, [leaf[k] for k in names], d_out.cuda())))
    fig = {k: relerr(gs[k], g_e[k]) for k in g_e}
    worst = max(fig, key=lambda k: fig[k])
    print(f"engine/d{D}: out {relerr(out, out_e):.2e}, worst parameter gradient {fig[worst]:.2e} ({worst})")
    assert set(fig) == set(names)
    assert relerr(out, out_e) < REL_OUT
    for k, v in fig.items():
        assert v < REL_GRAD, (k, v)
    assert float(gs[R.TABLE][0].abs().max()) == 0.0, "the PAD row takes no gradient"


# ------------------------------------------------------------------------------------------------ 6. the reference's recorded numbers
def build_module(p, n_items, L, D, F, n_layer, dropout=0.0, bidirectional=False):
    from dr4sr_amd.module.layers import SASRecQueryEncoderOps
    table = torch.nn.Embedding(n_items, D, padding_idx=0)
    m = SASRecQueryEncoderOps("item_id", D, L, H, F, dropout, "gelu", EPS, n_layer, table, bidirectional=bidirectional)
    pre = "query_encoder."
    sd = {k[len(pre):]: v for k, v in p.items() if k.startswith(pre)}          # an engine-backed SASRec checkpoint, prefix stripped
    sd["item_encoder.weight"] = p[R.TABLE]
    m.load_state_dict(sd)
    return m.cuda()


def test_module_reproduces_the_reference_training_step(golden_dir):
    gd = R.load_golden(golden_dir)
    p, b = R.golden_params(gd), R.golden_batch(gd)
    Bg, Lg = b["in_item_id"].shape
    m = build_module(p, int(gd["meta.num_items"]), Lg, 64, 128, 2)
    m.train()
    w = torch.from_numpy(gd["weight"]).cuda().requires_grad_(True)
    batch = {k: v.cuda() for k, v in b.items()}
    q = m({**batch, "input_weight": w})
    assert m.step == 1
    lp, st = torch.ops.dr4sr_hip.score_bce(q, m.item_encoder.weight, batch["item_id"], batch["neg_item"].squeeze(-1).contiguous())
    loss = lp.sum() / st[0]
    loss.backward()
    fig = {"query": relerr(q, gd["out.query"]), "loss": abs(float(loss.detach()) - float(gd["out.loss"])) / abs(float(gd["out.loss"]))}
    assert fig["query"] < REL_OUT and fig["loss"] < 1e-5, fig
    grads = {"item_embedding.weight": m.item_encoder.weight.grad}
    for n, t in m.named_parameters():
        if n != "item_encoder.weight":
            grads["query_encoder." + n] = t.grad
    ref = {k[len("grad."):]: v for k, v in gd.items() if k.startswith("grad.")}
    assert set(grads) == set(ref)
    for k in ref:
        fig[k] = relerr(grads[k], ref[k])
    fig["grad_weight"] = relerr(w.grad, gd["grad_weight"])
    worst = max((k for k in fig if k not in ("query", "loss")), key=lambda k: fig[k])
    print(f"golden: query {fig['query']:.2e}, loss {fig['loss']:.2e}, worst gradient {fig[worst]:.2e} ({worst})")
    for k, v in fig.items():
        if k not in ("query", "loss"):
            assert v < REL_GRAD, (k, v)


# ------------------------------------------------------------------------------------------------ 7. seq_emb and bidirectional
def test_module_seq_emb_and_bidirectional():
    import test_gpu_input_weight as TI
    B, L, D, F, NL, N = 5, 12, 64, 128, 2, 40
    p = TI.random_params(N, D, L, seed=77)
    g = torch.Generator().manual_seed(78)
    seq = torch.randn(B, L, D, generator=g)
    sl = torch.tensor([12, 1, 5, 12, 3])
    d_out = torch.randn(B, L, D, generator=g)
    m = build_module(p, N, L, D, F, NL, bidirectional=True)
    m.train()
    sd = seq.cuda().requires_grad_(True)
    out = m({"seq_emb": sd, "seqlen": sl.cuda(), "in_item_id": torch.zeros(B, L, dtype=torch.long, device="cuda")})
    out.backward(d_out.cuda())
    # the helper composed the same way: sasrec.py:50-54 (no key-padding mask), :60 (no causal mask), origin pooling
    so = seq.clone().requires_grad_(True)
    leaf = {k: v.clone().requires_grad_(True) for k, v in p.items() if k != R.TIED}
    x = so + leaf["query_encoder.position_emb.weight"][:L].unsqueeze(0)
    for i in range(NL):
        x = LR.layer(x, None, leaf, O.layer_prefix(i), H, EPS, causal=False)
    ref = LR.pool(x, sl, "origin")
    ref.backward(d_out)
    assert relerr(out, ref) < REL_OUT
    assert relerr(sd.grad, so.grad) < REL_GRAD
    for n, t in m.named_parameters():
        if n == "item_encoder.weight":
            assert t.grad is None                           # the table is not read on the seq_emb path
            continue
        assert relerr(t.grad, leaf["query_encoder." + n].grad) < REL_GRAD, n
    # the causal form of the same module differs
    m2 = build_module(p, N, L, D, F, NL, bidirectional=False)
    m2.train()
    with torch.no_grad():
        out2 = m2({"seq_emb": seq.cuda(), "seqlen": sl.cuda()})
    assert relerr(out2, ref) > 1e-2
    # eval mode pools 'last' and does not advance the step
    m.eval()
    with torch.no_grad():
        last = m({"seq_emb": seq.cuda(), "seqlen": sl.cuda()})
    assert last.shape == (B, D) and m.step == 1
    assert relerr(last, LR.pool(x.detach(), sl, "last")) < REL_OUT


def test_module_dropout_advances_the_step_and_uses_the_embedding_site():
    import test_gpu_input_weight as TI
    from dr4sr_amd import _lib
    idx, sl, _ = TI.small_batch()
    p = TI.random_params(TI.N, 64, TI.L, seed=3)
    m = build_module(p, TI.N, TI.L, 64, TI.F, TI.NL, dropout=0.5)
    m.train()
    batch = {"in_item_id": idx.cuda(), "seqlen": sl.cuda()}
    with torch.no_grad():
        a = m(batch)
        b = m(batch)
        m.step = 0
        a2 = m(batch)
    assert m.step == 1 and torch.equal(a, a2) and relerr(b, a) > 1e-2
    masks = library_masks(TI.B, TI.L, 64, TI.F, TI.NL, 0.5, m.seed, 0)
    emb = torch.empty(TI.B * TI.L * 64, device="cuda")
    _lib.check(_lib.load().dr4sr_dropout_mask(_lib.ptr(emb), emb.numel(), 0.5, m.seed, 0, _lib.SITE_EMB, _lib.cur_stream()), "mask")
    masks[O.SITE_EMB] = emb.view(TI.B, TI.L, 64).cpu()
    ref = R.encode(p, idx, sl, None, H, TI.NL, EPS, "origin", masks, 0.5)
    assert relerr(a, ref) < REL_OUT


# ------------------------------------------------------------------------------------------------ 8. graph capture
def test_captured_graph_replays_to_the_eager_bits():
    B, L, D, F, NL = 5, 12, 64, 128, 2
    g = torch.Generator().manual_seed(55)
    p = {k: v.cuda() for k, v in LR.layer_params(D, F, NL, seed=56).items()}
    x = torch.randn(B, L, D, generator=g).cuda()
    d_out = torch.randn(B, L, D, generator=g).cuda()
    kp = edge_key_pad().cuda()
    sl = torch.tensor([12, 1, 5, 12, 3]).cuda()
    o = torch.ops.dr4sr_hip

    def fwd_bwd():
        """forward and backward as one chain of op calls (the backward ops by hand: no autograd engine thread inside the capture)"""
        ys, saved = [x], []
        for i in range(NL):
            w = [p[f"layers.{i}.{n}"] for n in LR.LAYER_TENSORS]
            y, s = o.sasrec_layer(ys[-1], kp, True, *w, H, EPS, 0.5, 9, 2, i)
            ys.append(y)
            saved.append(s)
        out = o.seq_pool(ys[-1], sl, 1)
        dy = o.seq_pool_backward(d_out, sl, 1, L)
        grads = []
        for i in reversed(range(NL)):
            w = [p[f"layers.{i}.{n}"] for n in LR.LAYER_TENSORS]
            gs = o.sasrec_layer_backward(ys[i], kp, True, *w, H, EPS, 0.5, 9, 2, i, saved[i], dy)
            dy = gs[0]
            grads += gs[1:]
        return [out, dy] + grads

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
    assert len(captured) == 2 + 12 * NL
    for a, b in zip(captured, eager):
        assert torch.equal(a, b) and float(b.abs().max()) > 0
