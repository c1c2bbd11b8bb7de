"""torch.ops.dr4sr_hip.gru_layer (csrc/gru_op.hip) and dr4sr_amd.module.layers.GRULayerOps / GRU4RecQueryEncoderOps on the GPU.

Yardsticks: tests/_gru_layer_ref.py in float64 (pinned to torch.nn.GRU and the oracle by tests/test_gru_op_cpu.py), the GRU4Rec engine
on the same parameters, and the reference's recorded numbers (tests/golden/gru4rec_d64.npz).  Bars: tests/test_gpu_layer_op.py's —
max-abs error / max-abs reference < 2e-4 for outputs, < 5e-4 for gradients; against the engine tests/test_gpu_fmlp_op.py's 2e-4 / 3e-4;
against the golden file tests/test_gru_oracle.py's (rtol 2e-4 on queries, 3e-4 of the max-norm on gradients).

Inputs: tests/_gru_layer_ref.py make_case — weights uniform in +-3 / sqrt(H), x from N(0, 1): the gates leave their linear regime (the CPU
test asserts it).  Every case prints its worst figure (pytest -s); DESIGN.md records them."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dr4sr_amd.ops  # noqa: E402,F401  (registers torch.ops.dr4sr_hip.*)
import _gru_layer_ref as GR  # noqa: E402

REL_OUT, REL_GRAD = 2e-4, 5e-4
SPLITS, SPLIT_TILES = 32, 2                # csrc/gru_op.hip MAX_SPLITS, MIN_SPLIT_TILES: token splits of the weight-gradient launch
GROUP = "DR4SR_GRU_OP_GROUP"               # sequences per workgroup of the recurrence launches: 4, 8 or 16 (default: chosen by B)


def relerr(a, b):
    a = torch.as_tensor(a).detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    return float((a - b).abs().max() / max(1e-12, float(b.abs().max())))


@functools.lru_cache(maxsize=None)
def case(B, L, I, H, with_len):
    """inputs and the float64 result — built once per shape, shared, left unchanged"""
    x, w_ih, w_hh, d_out = GR.make_case(B, L, I, H)
    seqlen = GR.lengths(B, L) if with_len else None
    return x, w_ih, w_hh, d_out, seqlen, GR.layer_grads(x, w_ih, w_hh, d_out, seqlen)


def run_op(x, w_ih, w_hh, d_out, seqlen, backward_twice=False):
    """the op on the GPU through autograd -> (y, dx, dw_ih, dw_hh) [, the gradients of a second backward of the same forward]"""
    leaf = [t.cuda().requires_grad_(True) for t in (x, w_ih, w_hh)]
    y, _ = torch.ops.dr4sr_hip.gru_layer(*leaf, None if seqlen is None else seqlen.cuda())
    gs = [torch.autograd.grad(y, leaf, d_out.cuda(), retain_graph=True) for _ in range(2 if backward_twice else 1)]
    out = (y.detach(), *gs[0])
    return (out, gs[1]) if backward_twice else out


def check(tag, got, ref, rel_out=REL_OUT, rel_grad=REL_GRAD):
    names = ("y", "dx", "dw_ih", "dw_hh")
    for t in got:
        assert bool(torch.isfinite(t).all()), tag
    fig = {n: relerr(a, b) for n, a, b in zip(names, got, ref)}
    print(f"{tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert fig.pop("y") < rel_out, tag
    bad = "; ".join(f"{k} {v:.2e}" for k, v in fig.items() if not v < rel_grad)
    assert not bad, f"{tag}: at or above {rel_grad:g}: {bad}"


def zero_behind(t, seqlen):
    """is t [B, L, .] exactly zero at and behind every length?"""
    L = t.shape[1]
    behind = torch.arange(L).unsqueeze(0) >= seqlen.clamp(0, L).unsqueeze(1)
    return float(t.detach().cpu()[behind].abs().max()) == 0.0 if bool(behind.any()) else True


# ------------------------------------------------------------------------------------------------ 1. shapes, with and without lengths
@pytest.mark.parametrize("with_len", [False, True])
@pytest.mark.parametrize("shape", GR.SHAPES)
def test_forward_and_gradients_match_float64(shape, with_len):
    """(17, 12): a second group of the 16-row tile holds one row; (5, 50, 256, 256): both widest; (3, 70): L above the engine's 64"""
    x, w_ih, w_hh, d_out, seqlen, ref = case(*shape, with_len)
    got = run_op(x, w_ih, w_hh, d_out, seqlen)
    check(f"{shape} seqlen={'yes' if with_len else 'None'}", got, ref)
    if with_len:
        assert zero_behind(got[0], seqlen) and zero_behind(got[1], seqlen)


# ------------------------------------------------------------------------------------------------ 2. group sizes
@pytest.mark.parametrize("shape", [(17, 12, 128, 256), (5, 50, 256, 256)])
def test_group_sizes_agree(shape, monkeypatch):
    x, w_ih, w_hh, d_out, seqlen, ref = case(*shape, True)
    res = {}
    for gs in (4, 8, 16):
        monkeypatch.setenv(GROUP, str(gs))
        res[gs] = run_op(x, w_ih, w_hh, d_out, seqlen)
        check(f"{shape} group {gs}", res[gs], ref)
    for gs in (8, 16):
        check(f"{shape} group {gs} against group 4", res[gs], res[4])


# ------------------------------------------------------------------------------------------------ 3. behind the lengths
def test_garbage_behind_the_lengths_reaches_no_output():
    B, L, I, H = 5, 12, 64, 128
    x, w_ih, w_hh, d_out, seqlen, ref = case(B, L, I, H, True)
    clean = run_op(x, w_ih, w_hh, d_out, seqlen)
    behind = (torch.arange(L).unsqueeze(0) >= seqlen.unsqueeze(1)).unsqueeze(2)
    dirty = run_op(x.masked_fill(behind, float("nan")), w_ih, w_hh, d_out.masked_fill(behind, float("nan")), seqlen)
    for a, b in zip(clean, dirty):
        assert torch.equal(a, b)
    assert zero_behind(dirty[0], seqlen) and zero_behind(dirty[1], seqlen)
    # lengths outside [0, L] are clamped
    wide = run_op(x, w_ih, w_hh, d_out, torch.where(seqlen == L, seqlen + 5, torch.where(seqlen == 0, seqlen - 3, seqlen)))
    for a, b in zip(clean, wide):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 4. repeatability, written not accumulated
def token_splits(B, L):
    """csrc/gru_op.hip n_splits_of: the 64-token tiles dealt to at most SPLITS splits of at least SPLIT_TILES tiles, in equal runs"""
    tiles = (B * L + 63) // 64
    s = min(SPLITS, max(1, tiles // SPLIT_TILES))
    per = (tiles + s - 1) // s
    return (tiles + per - 1) // per


@pytest.mark.parametrize("B", [40, 341])
def test_two_backward_calls_return_the_same_bits_and_outputs_are_written(B):
    """B = 40: groups of 4 by default, 8 token tiles in 4 splits; B = 341: 64 token tiles, two for every one of the 32 slots"""
    from dr4sr_amd import _lib
    L, I, H = 12, 64, 128
    x, w_ih, w_hh, d_out, seqlen, ref = case(B, L, I, H, True)
    got, again = run_op(x, w_ih, w_hh, d_out, seqlen, backward_twice=True)
    check(f"B={B}", got, ref)
    for a, b in zip(got[1:], again):
        assert torch.equal(a, b) and float(a.abs().max()) > 0
    # through the C ABI into garbage-filled outputs and workspaces: the same bits
    lib = _lib.load()
    xd, wi, wh, dyd, sl = x.cuda(), w_ih.cuda(), w_hh.cuda(), d_out.cuda(), seqlen.cuda()
    n_saved = int(lib.dr4sr_gru_layer_saved_floats(B, L, I, H))
    nb0, nb1 = (int(lib.dr4sr_gru_layer_workspace_bytes(B, L, I, H, k)) for k in (0, 1))
    n_split = token_splits(B, L)
    assert nb1 == (B * L * 4 * H + n_split * 3 * H * (I + H)) * 4 and n_split == (4 if B == 40 else SPLITS)
    saved = torch.full((n_saved,), float("nan"), device="cuda")
    ws = torch.full((max(nb0, nb1) // 4,), float("nan"), device="cuda")
    y2 = torch.full((B, L, H), float("nan"), device="cuda")
    args = (_lib.ptr(xd), _lib.ptr(wi), _lib.ptr(wh), _lib.ptr(sl), B, L, I, H)
    _lib.check(lib.dr4sr_gru_layer_fwd(*args, _lib.ptr(y2), _lib.ptr(saved), _lib.ptr(ws), nb0, _lib.cur_stream()), "fwd")
    assert torch.equal(y2, got[0])
    ws.fill_(float("nan"))
    dx, dwi, dwh = torch.full_like(xd, 1e30), torch.full_like(wi, -1e30), torch.full_like(wh, 1e30)
    outs = (_lib.ptr(y2), _lib.ptr(saved), _lib.ptr(dyd), _lib.ptr(dx), _lib.ptr(dwi), _lib.ptr(dwh), _lib.ptr(ws))
    _lib.check(lib.dr4sr_gru_layer_bwd(*args, *outs, nb1, _lib.cur_stream()), "bwd")
    assert torch.equal(dx, got[1]) and torch.equal(dwi, got[2]) and torch.equal(dwh, got[3])
    # inference: no saved buffer, the same y
    y3 = torch.full_like(y2, float("nan"))
    _lib.check(lib.dr4sr_gru_layer_fwd(*args, _lib.ptr(y3), None, _lib.ptr(ws), nb0, _lib.cur_stream()), "fwd (inference)")
    assert torch.equal(y3, y2)
    # a workspace one byte short is refused before any launch
    assert lib.dr4sr_gru_layer_bwd(*args, *outs, nb1 - 1, _lib.cur_stream()) == -3
    assert lib.dr4sr_gru_layer_fwd(*args, _lib.ptr(y2), None, None, 0, _lib.cur_stream()) == -3


# ------------------------------------------------------------------------------------------------ 5. B = 0
def test_empty_batch_launches_nothing_and_zero_fills_the_weight_gradients():
    o = torch.ops.dr4sr_hip
    L, I, H = 12, 64, 128
    wi, wh = torch.randn(3 * H, I, device="cuda"), torch.randn(3 * H, H, device="cuda")
    x = torch.empty(0, L, I, device="cuda")
    for sl in (None, torch.empty(0, dtype=torch.int64, device="cuda")):
        y, saved = o.gru_layer(x, wi, wh, sl)
        assert y.shape == (0, L, H)
        dx, dwi, dwh = o.gru_layer_backward(x, wi, wh, sl, y, saved, torch.empty(0, L, H, device="cuda"))
        assert dx.shape == (0, L, I) and dwi.shape == wi.shape and dwh.shape == wh.shape
        assert float(dwi.abs().max()) == 0.0 and float(dwh.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 6. two layers through the module
@pytest.mark.parametrize("with_len", [False, True])
def test_two_layers_through_the_module_with_return_hidden(with_len):
    from dr4sr_amd.module.layers import GRULayerOps
    B, L, I, H = 5, 12, 64, 128
    x, w0, h0, d_out, seqlen, _ = case(B, L, I, H, with_len)
    _, w1, h1, _ = GR.make_case(B, L, H, H, seed=4242)
    m = GRULayerOps(I, H, 2, return_hidden=True)
    m.load_state_dict({"gru.weight_ih_l0": w0, "gru.weight_hh_l0": h0, "gru.weight_ih_l1": w1, "gru.weight_hh_l1": h1}, strict=True)
    m = m.cuda()
    xd = x.cuda().requires_grad_(True)
    out, hidden = m(xd, None if seqlen is None else seqlen.cuda())
    d_hid = torch.randn(2, B, H, generator=torch.Generator().manual_seed(5))
    (out * d_out.cuda()).sum().add((hidden * d_hid.cuda()).sum()).backward()
    # float64
    leaf = [t.double().requires_grad_(True) for t in (x, w0, h0, w1, h1)]
    y0 = GR.gru_layer(leaf[0], leaf[1], leaf[2], seqlen)
    y1 = GR.gru_layer(y0, leaf[3], leaf[4], seqlen)
    n = torch.full((B,), L) if seqlen is None else seqlen
    rows = torch.arange(B)
    last = [torch.where((n > 0).unsqueeze(1), y[rows, (n - 1).clamp(min=0)], torch.zeros(B, H, dtype=torch.float64)) for y in (y0, y1)]
    hid_o = torch.stack(last)
    gs = torch.autograd.grad((y1 * d_out.double()).sum() + (hid_o * d_hid.double()).sum(), leaf)
    fig = {"out": relerr(out, y1), "hidden": relerr(hidden, hid_o), "dx": relerr(xd.grad, gs[0])}
    for k, g in zip(("gru.weight_ih_l0", "gru.weight_hh_l0", "gru.weight_ih_l1", "gru.weight_hh_l1"), gs[1:]):
        fig[k] = relerr(dict(m.named_parameters())[k].grad, g)
    print(f"two layers, seqlen={'yes' if with_len else 'None'}: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert hidden.shape == (2, B, H) and out.shape == (B, L, H)
    assert fig.pop("out") < REL_OUT and fig.pop("hidden") < REL_OUT
    for k, v in fig.items():
        assert v < REL_GRAD, (k, v)


# ------------------------------------------------------------------------------------------------ 7. against the engine
def load_golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "gru4rec_d64.npz"))
    g = {k: z[k] for k in z.files}
    params = {k[6:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param.")}
    b = {k[6:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("batch.")}
    return g, params, b


def op_chain(leaf, idx, seqlen, NL, p_drop, seed, step, pooling):
    from dr4sr_amd import _lib
    o = torch.ops.dr4sr_hip
    E = leaf["item_embedding.weight"]
    x = o.embed_gather_posadd(E, torch.zeros(idx.shape[1], E.shape[1], device=E.device), idx)
    if p_drop > 0:
        x = o.dropout(x, p_drop, seed, step, _lib.SITE_EMB)
    for l in range(NL):
        x, _ = o.gru_layer(x, leaf[f"query_encoder.0.3.gru.weight_ih_l{l}"], leaf[f"query_encoder.0.3.gru.weight_hh_l{l}"], seqlen)
    x = torch.nn.functional.linear(x, leaf["query_encoder.1.weight"], leaf["query_encoder.1.bias"])
    return o.seq_pool(x, seqlen, pooling)


def test_op_chain_against_the_engine(golden_dir):
    """eval mode and train mode.  The train-mode comparison holds because the dropout op's keying at SITE_EMB is the engine's: k_gru_embed_gi<D>
    (csrc/gru.hip) draws element ((b L + pos) D + column) of stream (seed, RNG step, SITE_EMB) with b the batch row on a plan without `rows`
    — k_embed_fwd<D>'s index (csrc/embed.hip) and the memory order of the dense [B, L, D] tensor the op masks.  The engine's recurrences are
    bf16x3 products, the op's fp32."""
    from dr4sr_amd import _lib
    from dr4sr_amd.gru_engine import GruEngine
    g, params, b = load_golden(golden_dir)
    N, H, NL = int(g["meta.num_items"]), int(g["meta.hidden_size"]), int(g["meta.layer_num"])
    B, L = b["in_item_id"].shape
    pd, seed = 0.2, 31
    params = {k: v for k, v in params.items() if k != "query_encoder.0.1.weight"}
    eng = GruEngine(N, L, 64, H, NL, pd, B, "cuda", seed=seed)
    eng.load_named(params)
    idx, sl = b["in_item_id"].cuda(), b["seqlen"].cuda()
    plan = eng.make_plan(idx, None, sl)
    valid = (torch.arange(L).unsqueeze(0) < b["seqlen"].unsqueeze(1)).unsqueeze(2)
    d_out = (torch.randn(B, L, 64, generator=torch.Generator().manual_seed(78)) * valid).cuda()

    def compare(tag, training, step, out_e):
        leaf = {k: v.cuda().requires_grad_(True) for k, v in params.items()}
        out = op_chain(leaf, idx, sl, NL, pd if training else 0.0, seed, step, _lib.POOL_ORIGIN)
        names = list(leaf)
        gs = dict(zip(names, torch.autograd.grad(out, [leaf[k] for k in names], d_out)))
        eng.grads.zero_()
        eng.encode_bwd(plan, training, _lib.POOL_ORIGIN, d_out)
        torch.cuda.synchronize()
        eng.check_coop()
        fig = {k: relerr(gs[k], v) for k, v in eng.grad_views.items()}
        worst = max(fig, key=lambda k: fig[k])
        print(f"engine/{tag}: out {relerr(out, out_e):.2e}, worst parameter gradient {fig[worst]:.2e} ({worst})")
        assert set(fig) == set(names)
        assert relerr(out, out_e) < 2e-4
        for k, v in fig.items():
            assert v < 3e-4, (tag, k, v)
        assert float(gs["item_embedding.weight"][0].abs().max()) == 0.0, "the PAD row takes no gradient"
        return out

    out_eval = compare("eval", False, 0, eng.encode(plan, False, _lib.POOL_ORIGIN))
    before = int(eng.state[3])
    out_e = eng.encode(plan, True, _lib.POOL_ORIGIN)         # the engine advances its RNG step word first and draws with the new value
    step = int(eng.state[3])
    assert step == before + 1
    out_train = compare("train", True, step, out_e)
    assert relerr(out_train, out_eval) > 1e-2


# ------------------------------------------------------------------------------------------------ 8. the reference's recorded numbers
@pytest.mark.parametrize("use_seqlen", [True, False])
def test_module_reproduces_the_reference_training_step(golden_dir, use_seqlen):
    """both settings pass: what the seqlen argument skips is read by nothing downstream"""
    from dr4sr_amd.module.layers import GRU4RecQueryEncoderOps
    g, params, b = load_golden(golden_dir)
    N, H, NL = int(g["meta.num_items"]), int(g["meta.hidden_size"]), int(g["meta.layer_num"])
    B, L = b["in_item_id"].shape
    table = torch.nn.Embedding(N, 64, padding_idx=0)
    m = GRU4RecQueryEncoderOps("item_id", table, H, NL, 0.0, L, use_seqlen=use_seqlen)     # p = 0
    m.load_state_dict({k[len("query_encoder."):]: v for k, v in params.items() if k.startswith("query_encoder.")}, strict=True)
    m = m.cuda().train()
    batch = {k: v.cuda() for k, v in b.items()}
    q = m(batch)                                            # 'origin' in train mode
    assert q.shape == (B, L, 64) and m.step == 1
    np.testing.assert_allclose(q.detach().cpu().numpy(), g["out.query"], rtol=2e-4, atol=2e-6)
    lp, st = torch.ops.dr4sr_hip.score_bce(q, table.weight, batch["item_id"], batch["neg_item"].squeeze(-1).contiguous())
    loss = lp.sum() / st[0]
    loss.backward()
    e_l = abs(float(loss.detach()) - float(g["out.loss"]))
    grads = {"item_embedding.weight": table.weight.grad}
    grads.update({"query_encoder." + n: t.grad for n, t in m.named_parameters() if n != "0.1.weight"})
    assert set(grads) == {k[5:] for k in g if k.startswith("grad.")}
    fig = {k: relerr(v, g["grad." + k]) for k, v in grads.items()}
    worst = max(fig, key=lambda k: fig[k])
    print(f"golden, use_seqlen={use_seqlen}: query {relerr(q, g['out.query']):.2e}, loss difference {e_l:.2e}, worst gradient "
          f"{fig[worst]:.2e} ({worst})")
    assert int(st[0]) == int((b["item_id"] != 0).sum()) and e_l < 1e-5
    for k, v in fig.items():
        assert v < 3e-4, (k, v)
    m.eval()
    with torch.no_grad():
        ql = m({k[5:]: torch.from_numpy(g[k]).cuda() for k in ("eval.in_item_id", "eval.seqlen")})     # 'last' in eval mode
        full = m(batch, need_pooling=False)
    assert m.step == 1 and full.shape == (B, L, 64)
    np.testing.assert_allclose(ql.cpu().numpy(), g["eval.query_last"], rtol=2e-4, atol=2e-6)


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_raise_before_any_launch():
    from dr4sr_amd._lib import Dr4srError
    o = torch.ops.dr4sr_hip

    def tensors(B=2, L=12, I=64, H=128):
        return torch.zeros(B, L, I, device="cuda"), torch.zeros(3 * H, I, device="cuda"), torch.zeros(3 * H, H, device="cuda")
    for kw in ({"I": 32}, {"I": 96}, {"H": 64}, {"H": 192}, {"L": 1025}):
        x, wi, wh = tensors(**kw)
        with pytest.raises(Dr4srError):
            o.gru_layer(x, wi, wh, None)
        with pytest.raises(Dr4srError):
            o.gru_layer_backward(x, wi, wh, None, torch.zeros(x.shape[0], x.shape[1], wh.shape[1], device="cuda"), torch.zeros(8, device="cuda"),
                                 torch.zeros(x.shape[0], x.shape[1], wh.shape[1], device="cuda"))
    x, wi, wh = tensors()
    with pytest.raises(Dr4srError):
        o.gru_layer(x, torch.zeros(64, 3 * 128, device="cuda").t(), wh, None)              # a non-contiguous weight
    with pytest.raises(Dr4srError):
        o.gru_layer(torch.zeros(2, 64, 12, device="cuda").transpose(1, 2), wi, wh, None)   # a non-contiguous input
    with pytest.raises(Dr4srError):
        o.gru_layer(x, wi, wh, torch.ones(2, dtype=torch.int32, device="cuda"))            # int32 seqlen
    with pytest.raises(Dr4srError):
        o.gru_layer(x, wi, wh, torch.ones(3, dtype=torch.int64, device="cuda"))            # seqlen of another batch
    with pytest.raises(Dr4srError):
        o.gru_layer(x, wi, torch.zeros(3 * 128, 256, device="cuda"), None)                 # weight_hh not [3H, H]
    with pytest.raises(Dr4srError):
        o.gru_layer(x.double(), wi, wh, None)


# ------------------------------------------------------------------------------------------------ 10. graph capture
def test_captured_graph_replays_to_the_eager_bits():
    B, L, I, H = 5, 12, 64, 128
    x, w0, h0, d_out, seqlen, _ = case(B, L, I, H, True)
    _, w1, h1, _ = GR.make_case(B, L, H, H, seed=4242)
    x, w0, h0, w1, h1, d_out, sl = (t.cuda() for t in (x, w0, h0, w1, h1, d_out, seqlen))
    o = torch.ops.dr4sr_hip

    def fwd_bwd():
        """two layers forward and backward as one chain of op calls (the backward ops by hand: no autograd engine thread inside the capture)"""
        y0, s0 = o.gru_layer(x, w0, h0, sl)
        y1, s1 = o.gru_layer(y0, w1, h1, sl)
        d0, dw1, dh1 = o.gru_layer_backward(y0, w1, h1, sl, y1, s1, d_out)
        dx, dw0, dh0 = o.gru_layer_backward(x, w0, h0, sl, y0, s0, d0)
        return [y1, dx, dw0, dh0, dw1, dh1]

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
    for a, b in zip(captured, eager):
        assert torch.equal(a, b) and float(b.abs().max()) > 0
