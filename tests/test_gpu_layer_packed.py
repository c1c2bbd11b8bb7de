"""torch.ops.dr4sr_hip.sasrec_layer_packed (csrc/layer_packed.hip) and SASRecQueryEncoderOps(use_seqlen=True) on the GPU.

Yardstick: tests/_layer_ref.py in float64 with key_pad = pos >= n_b and a d_out zeroed at the pads (tests/_packed_ref.ref64).  y is
compared at the valid positions, dx and the 12 weight gradients everywhere.  Bars (tests/test_gpu_layer_op.py's): max-abs error /
max-abs reference < 2e-4 for outputs, < 5e-4 for gradients."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import dr4sr_amd.ops  # noqa: E402,F401  (registers torch.ops.dr4sr_hip.*)
import _inw_ref as R  # noqa: E402
import _layer_ref as LR  # noqa: E402
import _packed_ref as PR  # noqa: E402
from dr4sr_amd import _lib  # noqa: E402

REL_OUT, REL_GRAD = 2e-4, 5e-4
H, EPS = 2, 1e-12
EDGE_L, EDGE_LEN = 12, [12, 0, 1, 5, 12, 3, 2]
BOUND_L, BOUND_LEN = 50, [50, 14, 1, 50, 15, 64, -3, 13, 50]


def relerr(a, b):
    a = torch.as_tensor(a).detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    return float((a - b).abs().max() / max(1e-12, float(b.abs().max())))


def chunk():
    return int(_lib.probe("dr4sr_sasrec_layer_packed_chunk")())


def many_tiles_len():
    """B = 600, L = 40: every length 40 but 3 for b in [C - 6, C + 6) — more tiles than slots, short sequences on both sides of a chunk edge"""
    c = chunk()
    return [3 if c - 6 <= b < c + 6 else 40 for b in range(600)]


def inputs(B, L, D, F, n_layer, seed):
    g = torch.Generator().manual_seed(seed)
    return LR.layer_params(D, F, n_layer, seed=seed + 1), torch.randn(B, L, D, generator=g), torch.randn(B, L, D, generator=g)


def run_op(x, seqlen, p, causal, d_out, n_layer=1, p_drop=0.0, seed=7, step=1):
    """the op chain on the GPU through autograd -> (y, dx, {name: gradient})"""
    xd = x.cuda().requires_grad_(True)
    leaf = {k: v.cuda().requires_grad_(True) for k, v in p.items()}
    sl = torch.as_tensor(seqlen, dtype=torch.int64).cuda()
    y = xd
    for i in range(n_layer):
        w = [leaf[f"layers.{i}.{n}"] for n in LR.LAYER_TENSORS]
        y, _ = torch.ops.dr4sr_hip.sasrec_layer_packed(y, sl, causal, *w, H, EPS, p_drop, seed, step, i)
    names = list(leaf)
    gs = torch.autograd.grad(y, [xd] + [leaf[k] for k in names], d_out.cuda())
    return y.detach().cpu(), gs[0].cpu(), {k: g.cpu() for k, g in zip(names, gs[1:])}


def check(tag, got, ref, seqlen):
    (y, dx, g), (y_o, dx_o, g_o) = got, ref
    for t in (y, dx, *g.values()):
        assert bool(torch.isfinite(t).all()), tag
    pads = ~PR.valid_mask(seqlen, y.shape[1])
    assert float(y[pads].abs().sum()) == 0.0 and float(dx[pads].abs().sum()) == 0.0, (tag, "y and dx are exactly 0 at the pads")
    fig = {"y": relerr(PR.zero_pads(y, seqlen), PR.zero_pads(y_o, seqlen)), "dx": relerr(dx, dx_o)}
    for k in g_o:
        fig[k] = relerr(g[k], g_o[k])
    worst = max((k for k in fig if k != "y"), key=lambda k: fig[k])
    print(f"{tag}: y {fig['y']:.2e}, worst gradient {fig[worst]:.2e} ({worst})")
    assert fig.pop("y") < REL_OUT, tag
    for k, v in fig.items():
        assert v < REL_GRAD, (tag, k, v)


def same_bits(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(a[2][k], b[2][k]) for k in a[2])


# ------------------------------------------------------------------------------------------------ 1. every edge in one tile
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("D,F", [(64, 128), (64, 256), (128, 128)])
def test_every_edge_in_one_tile(D, F, causal):
    p, x, d_out = inputs(len(EDGE_LEN), EDGE_L, D, F, 1, 100 + D + F)
    ref = PR.ref64(x, EDGE_LEN, p, H, EPS, causal, d_out)
    check(f"edge/d{D}/f{F}/causal{int(causal)}", run_op(x, EDGE_LEN, p, causal, d_out), ref, EDGE_LEN)


# ------------------------------------------------------------------------------------------------ 2. tile boundaries and clamping
@pytest.mark.parametrize("D", [64, 128])
def test_tile_boundaries_and_clamped_lengths(D):
    for L, sl in ((BOUND_L, BOUND_LEN), (64, [64, 63, 1])):
        p, x, d_out = inputs(len(sl), L, D, 128, 1, L + D)
        for causal in (True, False):
            check(f"bound/d{D}/L{L}/causal{int(causal)}", run_op(x, sl, p, causal, d_out), PR.ref64(x, sl, p, H, EPS, causal, d_out), sl)


# ------------------------------------------------------------------------------------------------ 3. more tiles than slots, a chunk edge
def test_more_tiles_than_slots_and_a_chunk_boundary():
    sl = many_tiles_len()
    assert PR.plan(sl, 40, chunk())[2] > 256
    p, x, d_out = inputs(600, 40, 64, 128, 1, 33)
    check("many", run_op(x, sl, p, True, d_out), PR.ref64(x, sl, p, H, EPS, True, d_out), sl)


# ------------------------------------------------------------------------------------------------ 4. train mode
@pytest.mark.parametrize("D", [64, 128])
def test_train_mode_draws_the_dense_ops_masks(D):
    import test_gpu_layer_op as TL
    B, L, F, NL, pd, seed, step = len(EDGE_LEN), EDGE_L, 128, 2, 0.5, 4321, 3
    p, x, d_out = inputs(B, L, D, F, NL, 21 + D)
    masks = TL.library_masks(B, L, D, F, NL, pd, seed, step)
    ref = PR.ref64(x, EDGE_LEN, p, H, EPS, True, d_out, NL, masks, pd)
    got = run_op(x, EDGE_LEN, p, True, d_out, NL, pd, seed, step)
    check(f"train/d{D}", got, ref, EDGE_LEN)
    assert same_bits(run_op(x, EDGE_LEN, p, True, d_out, NL, pd, seed, step), got), "the same (seed, step, layer): the same bits"
    other = run_op(x, EDGE_LEN, p, True, d_out, NL, pd, seed, step + 1)
    assert relerr(other[0], got[0]) > 1e-2, "another step: other masks"
    eval_ = run_op(x, EDGE_LEN, p, True, d_out, NL, 0.0, seed, step)
    assert relerr(eval_[0], got[0]) > 1e-2
    assert same_bits(run_op(x, EDGE_LEN, p, True, d_out, NL, 0.0, seed + 1, step + 5), eval_), "p = 0 is eval: no mask is drawn"
    # a sequence draws the same masks alone in its tile (at row 0) as behind its neighbours: the elements are (b, pos)'s, not the row's
    b = 3
    alone = run_op(x, [n if i == b else 0 for i, n in enumerate(EDGE_LEN)], p, True, d_out, NL, pd, seed, step)
    assert relerr(alone[0][b], got[0][b]) < 1e-5 and relerr(alone[1][b], got[1][b]) < 1e-5 and float(alone[0][b].abs().max()) > 0
    if D == 64:
        dense_in_batch = torch.ops.dr4sr_hip.sasrec_layer(x.cuda(), (~PR.valid_mask(EDGE_LEN, L)).cuda(), True,
                                                          *[p[f"layers.0.{n}"].cuda() for n in LR.LAYER_TENSORS], H, EPS, pd, seed, step, 0)[0]
        packed = torch.ops.dr4sr_hip.sasrec_layer_packed(x.cuda(), torch.tensor(EDGE_LEN).cuda(), True,
                                                         *[p[f"layers.0.{n}"].cuda() for n in LR.LAYER_TENSORS], H, EPS, pd, seed, step, 0)[0]
        assert relerr(PR.zero_pads(packed.cpu(), EDGE_LEN), PR.zero_pads(dense_in_batch.cpu(), EDGE_LEN)) < 1e-5, "the dense op's decisions"


# ------------------------------------------------------------------------------------------------ 5. nothing behind the lengths is read
@pytest.mark.parametrize("D,pd", [(64, 0.0), (128, 0.5)])
def test_nothing_behind_the_lengths_is_read(D, pd):
    for L, sl in ((EDGE_L, EDGE_LEN), (BOUND_L, BOUND_LEN)):
        p, x, d_out = inputs(len(sl), L, D, 128, 1, 5 + D)
        clean = run_op(PR.zero_pads(x, sl), sl, p, True, PR.zero_pads(d_out, sl), 1, pd)
        dirty = run_op(PR.fill_pads(x, sl, float("nan")), sl, p, True, PR.fill_pads(d_out, sl, float("nan")), 1, pd)
        for t in (dirty[0], dirty[1], *dirty[2].values()):
            assert bool(torch.isfinite(t).all())
        assert same_bits(clean, dirty) and float(clean[1].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 6. written, not accumulated
def abi_call(x, seqlen, p, causal, d_out, pd, D, F):
    """forward and two backwards through the C ABI, every output and scratch buffer pre-filled with NaN -> (y, [(dx, 12 gradients)] * 2)"""
    lib = _lib.load()
    B, L, _ = x.shape
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")            # noqa: E731
    n = lib.dr4sr_sasrec_layer_packed_saved_floats(B, L, D, H, F)
    nf, nb = (lib.dr4sr_sasrec_layer_packed_workspace_bytes(B, L, D, H, F, k) for k in (0, 1))
    assert n > 0 and 0 < nf <= nb
    xd, dyd, sl = x.cuda(), d_out.cuda(), torch.as_tensor(seqlen, dtype=torch.int64).cuda()
    wt = [p[f"layers.0.{k}"].cuda() for k in LR.LAYER_TENSORS]
    w = _lib.LayerWeights(*[_lib.ptr(t) for t in wt])
    y, saved, ws = nan(B, L, D), nan(n), nan(nf // 4)
    st = _lib.cur_stream()
    _lib.check(lib.dr4sr_sasrec_layer_packed_fwd(_lib.ptr(xd), _lib.ptr(sl), int(causal), w, B, L, D, H, F, EPS, pd, 7, 1, 0, _lib.ptr(y),
                                                 _lib.ptr(saved), _lib.ptr(ws), nf, st), "fwd")
    outs = []
    for _ in range(2):
        dx, dws, ws = nan(B, L, D), [nan(*t.shape) for t in wt], nan(nb // 4)
        g = _lib.LayerGrads(*[_lib.ptr(t) for t in dws])
        _lib.check(lib.dr4sr_sasrec_layer_packed_bwd(_lib.ptr(xd), _lib.ptr(sl), int(causal), w, B, L, D, H, F, EPS, pd, 7, 1, 0,
                                                     _lib.ptr(saved), _lib.ptr(dyd), _lib.ptr(dx), g, _lib.ptr(ws), nb, st), "bwd")
        outs.append([dx] + dws)
    torch.cuda.synchronize()
    return y, outs


@pytest.mark.parametrize("case", ["edge", "many"])
def test_outputs_are_written_not_accumulated_and_reproducible(case):
    L, sl = (EDGE_L, EDGE_LEN) if case == "edge" else (40, many_tiles_len())
    p, x, d_out = inputs(len(sl), L, 64, 128, 1, 61)
    y, (a, b) = abi_call(x, sl, p, True, d_out, 0.5, 64, 128)
    assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
    for ta, tb in zip(a, b):
        assert bool(torch.isfinite(ta).all()) and torch.equal(ta, tb) and float(ta.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 7. empty inputs
def test_empty_inputs_give_zeros():
    D, F, L = 64, 128, 12
    w = [v.cuda() for v in LR.layer_params(D, F, 1, seed=1).values()]
    o = torch.ops.dr4sr_hip
    for B in (0, 5):
        x = torch.randn(B, L, D, device="cuda")
        sl = torch.zeros(B, dtype=torch.int64, device="cuda")
        y, saved = o.sasrec_layer_packed(x, sl, True, *w, H, EPS, 0.5, 7, 1, 0)
        assert y.shape == (B, L, D) and float(y.abs().sum()) == 0.0
        gs = o.sasrec_layer_packed_backward(x, sl, True, *w, H, EPS, 0.5, 7, 1, 0, saved, torch.randn(B, L, D, device="cuda"))
        assert gs[0].shape == (B, L, D) and float(gs[0].abs().sum()) == 0.0 and len(gs) == 13
        for g, t in zip(gs[1:], w):
            assert g.shape == t.shape and float(g.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 8. the plan
def device_plan(seqlen, L):
    lib = _lib.load()
    B = len(seqlen)
    sl = torch.as_tensor(seqlen, dtype=torch.int64).cuda()
    tile_of, row_of = (torch.full((max(B, 1),), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    n_tiles = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    nb = lib.dr4sr_sasrec_layer_packed_workspace_bytes(B, L, 64, 2, 128, 0)
    ws = torch.full((nb // 4,), -7, dtype=torch.int32, device="cuda")
    plan = _lib.probe("dr4sr_sasrec_layer_packed_plan")
    _lib.check(plan(_lib.ptr(sl), B, L, _lib.ptr(tile_of), _lib.ptr(row_of), _lib.ptr(n_tiles), _lib.ptr(ws), nb, _lib.cur_stream()), "plan")
    return tile_of[:B].tolist(), row_of[:B].tolist(), int(n_tiles)


def test_device_plan_equals_the_python_statement():
    g = torch.Generator().manual_seed(8)
    B, L = 1000, 50
    short = torch.randint(1, 12, (B,), generator=g).tolist()                                   # toys-like
    mixed = (torch.randint(0, L + 8, (B,), generator=g) * (torch.rand(B, generator=g) > 0.3)).tolist()
    cases = [(EDGE_L, EDGE_LEN), (BOUND_L, BOUND_LEN), (64, [64, 63, 1]), (40, many_tiles_len()), (L, short), (L, [L] * B), (L, mixed),
             (L, [])]
    c = chunk()
    assert c >= 64
    for L_, sl in cases:
        want = PR.plan(sl, L_, c)
        assert device_plan(sl, L_) == want, (L_, sl[:16])
        PR.check_plan(sl, L_, c, *want)


# ------------------------------------------------------------------------------------------------ 9. the module
def build_module(p, n_items, L, D, F, n_layer, dropout, use_seqlen, **kw):
    from dr4sr_amd.module.layers import SASRecQueryEncoderOps
    table = torch.nn.Embedding(n_items, D, padding_idx=0)
    m = SASRecQueryEncoderOps("item_id", D, L, H, F, dropout, "gelu", EPS, n_layer, table, use_seqlen=use_seqlen, **kw)
    pre = "query_encoder."
    sd = {k[len(pre):]: v for k, v in p.items() if k.startswith(pre)}
    sd["item_encoder.weight"] = p[R.TABLE]
    m.load_state_dict(sd)
    return m.cuda()


@pytest.mark.parametrize("pooling", ["origin", "last", "mean"])
def test_module_with_use_seqlen_agrees_with_the_dense_module(pooling):
    import test_gpu_input_weight as TI
    N, L, D, F, NL = 40, EDGE_L, 64, 128, 2
    sl = torch.tensor(EDGE_LEN)
    g = torch.Generator().manual_seed(91)
    idx = torch.randint(1, N, (len(EDGE_LEN), L), generator=g) * PR.valid_mask(EDGE_LEN, L)   # post-padded ids
    p = TI.random_params(N, D, L, seed=92)
    batch = {"in_item_id": idx.cuda(), "seqlen": sl.cuda()}
    res = {}
    for flag in (False, True):
        m = build_module(p, N, L, D, F, NL, 0.5, flag, training_pooling_type=pooling, eval_pooling_type=pooling)
        m.train()
        m.step = 4
        out = m(batch)
        d_out = torch.randn(out.shape, generator=torch.Generator().manual_seed(93)).cuda()
        out.backward(d_out)
        m.eval()
        with torch.no_grad():
            ev = m(batch)
        res[flag] = (out.detach(), {n: t.grad for n, t in m.named_parameters()}, ev)
        assert m.step == 5
    assert relerr(res[True][0], res[False][0]) < REL_OUT and relerr(res[True][2], res[False][2]) < REL_OUT
    assert set(res[True][1]) == set(res[False][1])
    for n, gr in res[False][1].items():
        assert relerr(res[True][1][n], gr) < REL_GRAD, n


def test_module_with_use_seqlen_reproduces_the_reference_training_step(golden_dir):
    """tests/test_gpu_layer_op.py's run of the dense module against the reference's recorded step, with use_seqlen=True, at the same bars.

    The fixture's batch has an id 0 INSIDE a valid range (row 6, position 4, seqlen 12), which the reference masks as a key
    (mask4padding = id == 0) and sasrec_layer_packed cannot: forced through the packed op the module missed the bars by far (measured:
    query 3.2e-2, loss 1.4e-4, grad_weight 1.2e-1).  The module therefore checks its requirement per batch and runs such a batch on the
    dense op — test_module_takes_the_packed_op_only_where_the_ids_are_post_padded pins which batch takes which."""
    gd = R.load_golden(golden_dir)
    p, b = R.golden_params(gd), R.golden_batch(gd)
    Bg, Lg = b["in_item_id"].shape
    off = (b["in_item_id"] != 0) != PR.valid_mask(b["seqlen"].tolist(), Lg)
    print(f"golden/use_seqlen: positions where (id != 0) differs from (pos < seqlen): {off.nonzero().tolist()}")
    m = build_module(p, int(gd["meta.num_items"]), Lg, 64, 128, 2, 0.0, True)
    m.train()
    w = torch.from_numpy(gd["weight"]).cuda().requires_grad_(True)
    batch = {k: v.cuda() for k, v in b.items()}
    q = m({**batch, "input_weight": w})
    lp, st = torch.ops.dr4sr_hip.score_bce(q, m.item_encoder.weight, batch["item_id"], batch["neg_item"].squeeze(-1).contiguous())
    loss = lp.sum() / st[0]
    loss.backward()
    fig = {"query": relerr(q, gd["out.query"]), "loss": abs(float(loss.detach()) - float(gd["out.loss"])) / abs(float(gd["out.loss"]))}
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
    print(f"golden/use_seqlen: query {fig['query']:.2e}, loss {fig['loss']:.2e}, worst gradient {fig[worst]:.2e} ({worst})")
    assert fig["query"] < REL_OUT and fig["loss"] < 1e-5, fig
    for k, v in fig.items():
        if k not in ("query", "loss"):
            assert v < REL_GRAD, (k, v)


def test_module_takes_the_packed_op_only_where_the_ids_are_post_padded(monkeypatch):
    import test_gpu_input_weight as TI
    N, L, D, F, NL = 40, EDGE_L, 64, 128, 2
    p = TI.random_params(N, D, L, seed=92)
    good = torch.randint(1, N, (len(EDGE_LEN), L), generator=torch.Generator().manual_seed(94)) * PR.valid_mask(EDGE_LEN, L)
    hole = good.clone()
    hole[4, 6] = 0                                          # an id 0 in front of the length: a masked key that seqlen cannot express
    tail = good.clone()
    tail[3, 9] = 7                                          # an id behind the length: a key that seqlen would drop
    sl = torch.tensor(EDGE_LEN).cuda()
    pads = ~PR.valid_mask(EDGE_LEN, L)
    m0, m1 = (build_module(p, N, L, D, F, NL, 0.0, flag).eval() for flag in (False, True))
    with torch.no_grad():
        for tag, idx, takes_packed in (("post-padded", good, True), ("hole", hole, False), ("tail", tail, False)):
            batch = {"in_item_id": idx.cuda(), "seqlen": sl}
            y0, y1 = m0(batch, need_pooling=False).cpu(), m1(batch, need_pooling=False).cpu()
            assert float(y0[pads].abs().max()) > 0, tag      # the dense op computes the pads too
            if takes_packed:
                assert float(y1[pads].abs().sum()) == 0.0 and relerr(PR.zero_pads(y1, EDGE_LEN), PR.zero_pads(y0, EDGE_LEN)) < REL_OUT, tag
            else:
                assert torch.equal(y1, y0), tag              # the dense op's bits
        # without the check the requirement is the caller's: the packed op runs, and on the batch with the hole it differs
        monkeypatch.setenv("DR4SR_NO_ID_CHECK", "1")
        y1 = m1({"in_item_id": hole.cuda(), "seqlen": sl}, need_pooling=False).cpu()
        assert float(y1[pads].abs().sum()) == 0.0


def test_module_seq_emb_path_keeps_the_dense_op():
    import test_gpu_input_weight as TI
    B, L, D, F, NL, N = 5, 12, 64, 128, 2, 40
    p = TI.random_params(N, D, L, seed=77)
    seq = torch.randn(B, L, D, generator=torch.Generator().manual_seed(78)).cuda()
    batch = {"seq_emb": seq, "seqlen": torch.tensor([12, 1, 5, 12, 3]).cuda()}
    outs = []
    for flag in (False, True):
        m = build_module(p, N, L, D, F, NL, 0.0, flag)
        m.train()
        with torch.no_grad():
            outs.append(m(batch, need_pooling=False))
    assert torch.equal(outs[0], outs[1]) and float(outs[0][1, 5:].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 10. refusals
def test_refusals_come_before_any_launch():
    D, F, L, B = 64, 128, 12, 4
    o = torch.ops.dr4sr_hip
    w = [v.cuda() for v in LR.layer_params(D, F, 1, seed=1).values()]
    x = torch.randn(B, L, D, device="cuda")
    sl = torch.full((B,), 5, dtype=torch.int64, device="cuda")
    tail = (H, EPS, 0.0, 7, 1, 0)
    y, saved = o.sasrec_layer_packed(x, sl, True, *w, *tail)
    dy = torch.randn(B, L, D, device="cuda")
    wide = torch.randn(B, L, 2 * D, device="cuda")[:, :, :D]
    bad_fwd = {
        "x dtype": (x.double(), sl, w), "x on the host": (x.cpu(), sl, w), "x not contiguous": (wide, sl, w),
        "x not 3-d": (x[0], sl, w),
        "seqlen dtype": (x, sl.int(), w), "seqlen shape": (x, sl[:3], w), "seqlen 2-d": (x, sl.view(B, 1), w),
        "seqlen on the host": (x, sl.cpu(), w), "seqlen not contiguous": (x, torch.stack([sl, sl], 1)[:, 0], w),
        "weight dtype": (x, sl, [w[0].double()] + w[1:]), "weight not contiguous": (x, sl, [w[0].t().contiguous().t()] + w[1:]),
        "weight shape": (x, sl, w[:4] + [w[4][:100]] + w[5:]),
    }
    for tag, (x_, sl_, w_) in bad_fwd.items():
        with pytest.raises(_lib.Dr4srError):
            o.sasrec_layer_packed(x_, sl_, True, *w_, *tail)
            pytest.fail(tag)
    for tag, (s_, dy_) in {"dy not contiguous": (saved, wide), "dy dtype": (saved, dy.double()), "dy shape": (saved, dy[:, :5].contiguous()),
                           "saved too small": (saved[:100], dy), "dy on the host": (saved, dy.cpu())}.items():
        with pytest.raises(_lib.Dr4srError):
            o.sasrec_layer_packed_backward(x, sl, True, *w, *tail, s_, dy_)
            pytest.fail(tag)
    # unsupported (D, F, H, L): the library's refusal, by its name
    for tag, (Lb, Db, Fb, Hb) in {"L = 65": (65, 64, 128, 2), "D = 96": (12, 96, 128, 2), "head_dim 16": (12, 64, 128, 4),
                                  "D = 128 with F = 256": (12, 128, 256, 2), "F = 192": (12, 64, 192, 2)}.items():
        wb = [torch.zeros(s, device="cuda") for s in [(3 * Db, Db), (3 * Db,), (Db, Db), (Db,), (Fb, Db), (Fb,), (Db, Fb), (Db,), (Db,),
                                                      (Db,), (Db,), (Db,)]]
        with pytest.raises(_lib.Dr4srError, match="DR4SR_E_SHAPE"):
            o.sasrec_layer_packed(torch.zeros(B, Lb, Db, device="cuda"), sl, True, *wb, Hb, EPS, 0.0, 7, 1, 0)
            pytest.fail(tag)
    y2, _ = o.sasrec_layer_packed(x, sl, True, *w, *tail)                 # and the op still runs
    assert torch.equal(y, y2)


# ------------------------------------------------------------------------------------------------ 11. graph replay
def test_captured_graph_replays_to_the_eager_bits_and_plans_again_on_the_device():
    L, D, F, NL = EDGE_L, 64, 128, 2
    B = len(EDGE_LEN)
    second = [3, 12, 0, 7, 1, 12, 12]
    p, x, d_out = inputs(B, L, D, F, NL, 55)
    p = {k: v.cuda() for k, v in p.items()}
    x, d_out = x.cuda(), d_out.cuda()
    sl = torch.tensor(EDGE_LEN).cuda()
    o = torch.ops.dr4sr_hip

    def fwd_bwd():
        """forward and backward as one chain of op calls (the backward ops by hand: no autograd engine thread inside the capture)"""
        ys, saved = [x], []
        for i in range(NL):
            w = [p[f"layers.{i}.{n}"] for n in LR.LAYER_TENSORS]
            y, s = o.sasrec_layer_packed(ys[-1], sl, True, *w, H, EPS, 0.5, 9, 2, i)
            ys.append(y)
            saved.append(s)
        out = o.seq_pool(ys[-1], sl, 1)
        dy = o.seq_pool_backward(d_out, sl, 1, L)
        grads = []
        for i in reversed(range(NL)):
            w = [p[f"layers.{i}.{n}"] for n in LR.LAYER_TENSORS]
            gs = o.sasrec_layer_packed_backward(ys[i], sl, True, *w, H, EPS, 0.5, 9, 2, i, saved[i], dy)
            dy = gs[0]
            grads += gs[1:]
        return [out, dy] + grads

    eager = [t.clone() for t in fwd_bwd()]
    sl.copy_(torch.tensor(second))
    eager2 = [t.clone() for t in fwd_bwd()]
    sl.copy_(torch.tensor(EDGE_LEN))
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
    assert len(captured) == 2 + 12 * NL
    for want, lens in ((eager, EDGE_LEN), (eager2, second), (eager, EDGE_LEN)):
        sl.copy_(torch.tensor(lens))
        for t in captured:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(captured, want):
            assert torch.equal(a, b) and float(b.abs().max()) > 0
    assert not torch.equal(eager[0], eager2[0])
