"""GPU parity tests: the HIP path (through the C ABI in libdr4sr_hip.so) vs the CPU oracle and the
golden vectors produced by the reference.  Run with `pytest -m gpu` on an MI355X box.

Tolerances: north_star asks for <= 1e-3 relative in fp32 and bit-exact index gather; the tests hold
the kernels to 2e-4 (max-abs error / max-abs reference) and exact equality for the gather.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import sasrec_oracle as O  # noqa: E402

REL = 2e-4


def relerr(a, b):
    a = a.detach().cpu().double()
    b = torch.as_tensor(b).double()
    return float((a - b).abs().max() / max(1e-12, float(b.abs().max())))


def load_golden(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    g = {k: z[k] for k in z.files}
    params = {k[len("param."):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param.")}
    batch = {k[len("batch."):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("batch.")}
    return g, params, batch


def make_engine(g, params, B, p_drop=0.0, n_items=None, **kw):
    from dr4sr_amd.engine import SasrecEngine
    D = int(g["meta.embed_dim"])
    eng = SasrecEngine(n_items=n_items or int(g["meta.num_items"]), L=50, D=D, H=int(g["meta.head_num"]),
                       F=int(g["meta.hidden_size"]), n_layer=int(g["meta.layer_num"]),
                       ln_eps=float(g["meta.layer_norm_eps"]), p_drop=p_drop, max_batch=B, device="cuda", **kw)
    eng.load_named(params)
    return eng


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dr4sr_amd import _lib
    _lib.load()                       # fail loudly if the HIP library is missing
    return torch.device("cuda")


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("B", [1, 7, 256])
def test_embed_gather_bit_exact(dev, D, B):
    from dr4sr_amd import _lib
    lib = _lib.load()
    torch.manual_seed(B + D)
    N, L = 11925, 50
    E = torch.randn(N, D, device=dev)
    E[0] = 0
    P = torch.randn(L, D, device=dev)
    idx = torch.randint(0, N, (B, L), device=dev)
    idx[:, L // 2:] = 0
    out = torch.empty(B, L, D, device=dev)
    _lib.check(lib.dr4sr_embed_gather_posadd(_lib.ptr(E), _lib.ptr(P), _lib.ptr(idx), _lib.ptr(out), B, L, D, N,
                                             _lib.cur_stream()), "gather")
    ref = E[idx] + P.unsqueeze(0)
    assert torch.equal(out, ref)
    ref_cpu = O.embed_posadd(E.cpu(), P.cpu(), idx.cpu())
    assert torch.equal(out.cpu(), ref_cpu)


def test_embed_gather_empty_and_errors(dev):
    from dr4sr_amd import _lib
    lib = _lib.load()
    E = torch.zeros(4, 64, device=dev)
    assert lib.dr4sr_embed_gather_posadd(_lib.ptr(E), _lib.ptr(E), _lib.ptr(E), _lib.ptr(E), 0, 50, 64, 4, None) == 0
    assert lib.dr4sr_embed_gather_posadd(None, _lib.ptr(E), _lib.ptr(E), _lib.ptr(E), 1, 50, 64, 4, None) == -1
    assert lib.dr4sr_embed_gather_posadd(_lib.ptr(E), _lib.ptr(E), _lib.ptr(E), _lib.ptr(E), 1, 50, 48, 4, None) == -2


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sasrec_d64", "sasrec_d128"])
def test_encode_vs_golden(dev, golden_dir, name):
    from dr4sr_amd import _lib
    g, params, b = load_golden(golden_dir, name)
    B = b["in_item_id"].shape[0]
    eng = make_engine(g, params, B)
    idx, tgt, sl = b["in_item_id"].to(dev), b["item_id"].to(dev), b["seqlen"].to(dev)
    plan = eng.make_plan(idx, tgt, sl)
    q = eng.encode(plan, False, _lib.POOL_ORIGIN)
    assert relerr(q, g["out.query"]) < REL
    # eval rows ('last' pooling) against the reference's eval-mode forward
    eidx, esl = torch.from_numpy(g["eval.in_item_id"]).to(dev), torch.from_numpy(g["eval.seqlen"]).to(dev)
    plan = eng.make_plan(eidx, None, esl)
    ql = eng.encode(plan, False, _lib.POOL_LAST)
    assert relerr(ql, g["eval.query_last"]) < REL


@pytest.mark.parametrize("name", ["sasrec_d64", "sasrec_d128"])
def test_fwd_bwd_and_adam_vs_golden(dev, golden_dir, name):
    g, params, b = load_golden(golden_dir, name)
    B = b["in_item_id"].shape[0]
    eng = make_engine(g, params, B, lr=float(g["meta.lr"]), weight_decay=float(g["meta.weight_decay"]))
    idx, tgt, sl = b["in_item_id"].to(dev), b["item_id"].to(dev), b["seqlen"].to(dev)
    neg = b["neg_item"].squeeze(-1).contiguous().to(dev)
    plan = eng.make_plan(idx, tgt, sl, neg_item=neg, sample_neg=False)
    eng.fwd_bwd(plan)
    loss, n = eng.loss_and_count()
    assert n == int((b["item_id"] != 0).sum())
    assert abs(loss - float(g["out.loss"])) < 1e-5 * abs(float(g["out.loss"])) + 1e-6
    grads = eng.normalized_grads()
    for k, gv in grads.items():
        assert relerr(gv, g["grad." + k]) < REL, k
    # PAD row of the table never receives gradient
    assert float(grads["item_embedding.weight"][0].abs().max()) == 0.0
    # two optimizer steps (second on the same batch) against the reference's torch.optim.Adam
    eng.adam_step(plan)
    for k, v in eng.views.items():
        well = np.abs(g["grad." + k]) > 1e-5
        d = (v.cpu().numpy() - g["adam1." + k])
        assert np.abs(d[well]).max(initial=0) < 5e-6, (k, float(np.abs(d[well]).max(initial=0)))
        # where |g| <~ adam_eps the update lr * m / (sqrt(v) + eps) amplifies a 1e-9 gradient difference (fp32 atomics order) to O(lr):
        # the bound is lr / 5, the observed worst value is reported on failure
        assert np.abs(d).max() < 2e-4, (k, "worst |param - reference| %.3e on near-zero-gradient elements" % float(np.abs(d).max()))
    eng.fwd_bwd(plan)
    loss2, _ = eng.loss_and_count()
    assert abs(loss2 - float(g["out.loss_step2"])) < 2e-5
    eng.adam_step(plan)
    assert int(eng.state[0]) == 2
    for k, v in eng.views.items():
        well = np.abs(g["grad." + k]) > 1e-5
        d = (v.cpu().numpy() - g["adam2." + k])
        assert np.abs(d[well]).max(initial=0) < 1e-5, (k, float(np.abs(d[well]).max(initial=0)))
        assert np.abs(d).max() < 4e-4, (k, "worst |param - reference| %.3e after two steps (near-zero-gradient elements)" % float(np.abs(d).max()))


# ------------------------------------------------------------------------------------------------
def _masks_from_engine(eng, cu, seqlen, B, L, D, H, F, n_layer, step):
    """Materialise the library's own keep-masks and lay them out densely for the oracle."""
    from dr4sr_amd import _lib
    masks = {}
    masks[O.SITE_EMB] = eng.dropout_mask(B * L * D, _lib.SITE_EMB, step).view(B, L, D).cpu()
    T = int(cu[-1])

    def dense(packed, width):
        out = torch.ones(B, L, width)
        for bi in range(B):
            n = int(seqlen[bi])
            out[bi, :n] = packed[int(cu[bi]):int(cu[bi]) + n]
        return out
    for l in range(n_layer):
        a = eng.dropout_mask(B * H * 64 * 64, _lib.SITE_ATTN + 4 * l, step).view(B, H, 64, 64)[:, :, :L, :L]
        masks[O.site(O.SITE_ATTN, l)] = a.cpu().contiguous()
        masks[O.site(O.SITE_PROJ, l)] = dense(eng.dropout_mask(T * D, _lib.SITE_PROJ + 4 * l, step).view(T, D).cpu(), D)
        masks[O.site(O.SITE_ACT, l)] = dense(eng.dropout_mask(T * F, _lib.SITE_ACT + 4 * l, step).view(T, F).cpu(), F)
        masks[O.site(O.SITE_FFN, l)] = dense(eng.dropout_mask(T * D, _lib.SITE_FFN + 4 * l, step).view(T, D).cpu(), D)
    return masks


@pytest.mark.parametrize("name,p", [("sasrec_d64", 0.5), ("sasrec_d128", 0.2)])
def test_fwd_bwd_with_dropout_matches_oracle_with_same_masks(dev, golden_dir, name, p):
    g, params, b = load_golden(golden_dir, name)
    B, L = b["in_item_id"].shape
    H, nl, eps = int(g["meta.head_num"]), int(g["meta.layer_num"]), float(g["meta.layer_norm_eps"])
    D, F = int(g["meta.embed_dim"]), int(g["meta.hidden_size"])
    eng = make_engine(g, params, B, p_drop=p, seed=1234)
    idx, tgt, sl = b["in_item_id"].to(dev), b["item_id"].to(dev), b["seqlen"].to(dev)
    neg = b["neg_item"].squeeze(-1).contiguous().to(dev)
    plan = eng.make_plan(idx, tgt, sl, neg_item=neg, sample_neg=False)
    eng.fwd_bwd(plan)
    step = int(eng.state[3])
    assert step == 1
    cu = torch.cat([torch.zeros(1, dtype=torch.long), b["seqlen"].cumsum(0)])
    masks = _masks_from_engine(eng, cu, b["seqlen"], B, L, D, H, F, nl, step)
    keep = float(masks[O.SITE_EMB].mean())
    assert abs(keep - (1 - p)) < 0.02
    loss_o, q_o, grads_o = O.grads_of(params, b, H, nl, eps, masks=masks, pdrop=p)
    loss, n = eng.loss_and_count()
    assert abs(loss - float(loss_o)) < 2e-5 * max(1.0, abs(float(loss_o)))
    grads = eng.normalized_grads()
    for k, gv in grads.items():
        assert relerr(gv, grads_o[k]) < REL, k
    # a second call draws different masks (RNG step advanced)
    eng.fwd_bwd(plan)
    loss_b, _ = eng.loss_and_count()
    assert int(eng.state[3]) == 2 and abs(loss_b - loss) > 1e-7


# ------------------------------------------------------------------------------------------------
def _toys_batch(B, dense, seed, n_items=None):
    from dr4sr_amd.data.synthetic import make_rows, TOYS_N_ITEMS
    N = n_items or TOYS_N_ITEMS
    rows = make_rows(n_rows=B, n_items=N, seed=seed, dense=dense)
    b = {k: torch.from_numpy(rows[k]) for k in ("in_item_id", "item_id", "seqlen")}
    b["neg_item"] = torch.randint(1, N, (B, 50, 1), generator=torch.Generator().manual_seed(seed))
    return b, N


def _random_params(n_items, D, F, n_layer, L=50, seed=0):
    from dr4sr_amd.engine import param_names, param_shapes
    gen = torch.Generator().manual_seed(seed)
    p = {}
    for n, s in zip(param_names(n_layer), param_shapes(n_items, L, D, F, n_layer)):
        if n.endswith("norm1.weight") or n.endswith("norm2.weight"):
            p[n] = 1.0 + 0.1 * torch.randn(s, generator=gen)
        elif "in_proj_weight" in n:
            p[n] = 0.15 * torch.randn(s, generator=gen)
        else:
            p[n] = 0.05 * torch.randn(s, generator=gen)
    p["item_embedding.weight"][0] = 0
    p["query_encoder.item_encoder.weight"] = p["item_embedding.weight"]
    return p


@pytest.mark.parametrize("dense,D,n_items", [(False, 64, None), (True, 64, None), (False, 128, 20034)])
def test_full_size_batch_vs_oracle(dev, dense, D, n_items):
    """BASELINE configs[1] at its real size: B=256, N=11925, L=50, d=64 (toys-shaped and all-dense), and configs[3]'s shape
    (yelp: N=20034, d=128)."""
    from dr4sr_amd.engine import SasrecEngine
    B = 256
    b, N = _toys_batch(B, dense, seed=5, n_items=n_items)
    params = _random_params(N, D, 128, 2, seed=1)
    eng = SasrecEngine(N, 50, D, 2, 128, 2, 1e-12, 0.0, B, "cuda")
    eng.load_named(params)
    plan = eng.make_plan(b["in_item_id"].to(dev), b["item_id"].to(dev), b["seqlen"].to(dev),
                         neg_item=b["neg_item"].squeeze(-1).contiguous().to(dev), sample_neg=False)
    eng.fwd_bwd(plan)
    loss, n = eng.loss_and_count()
    loss_o, _, grads_o = O.grads_of(params, b, 2, 2, 1e-12)
    assert n == int((b["item_id"] != 0).sum())
    assert abs(loss - float(loss_o)) < 2e-5
    grads = eng.normalized_grads()
    for k, gv in grads.items():
        assert relerr(gv, grads_o[k]) < REL, k
    # size-independent properties: PAD row untouched, untouched table rows exactly zero,
    # and the replay is reproducible up to fp32 atomic ordering
    touched = torch.zeros(N, dtype=torch.bool)
    valid = b["item_id"] != 0
    touched[b["item_id"][valid]] = True
    touched[b["neg_item"].squeeze(-1)[valid]] = True
    touched[b["in_item_id"][b["in_item_id"] != 0]] = True
    gE = grads["item_embedding.weight"].cpu()
    assert float(gE[0].abs().max()) == 0.0
    assert float(gE[~touched].abs().max()) == 0.0
    g1 = {k: v.clone() for k, v in grads.items()}
    eng.fwd_bwd(plan)
    for k, v in eng.normalized_grads().items():
        assert relerr(v, g1[k].cpu()) < 1e-5, k


def test_large_batch_length_split_attention(dev, monkeypatch, at_scale):
    """B = 1024 (T_max > 16384): BM = 32 token tiles and the attention split into a short-sequence (n <= 16) and a long-sequence
    persistent launch over k_prep's length-class lists.  Checked against the oracle and against the unsplit launch.
    (Round 6: the lists are the cross-check form, DR4SR_ATTN_LISTS — the default at scale is csrc/attn_wave.hip, tests/test_gpu_attn_wave.py.)"""
    from dr4sr_amd.engine import SasrecEngine
    monkeypatch.setenv("DR4SR_ATTN_LISTS", "1")
    B = 1024
    b, N = _toys_batch(B, False, seed=9)
    b["seqlen"][5] = 16
    b["seqlen"][6] = 17                                            # both sides of the class boundary
    for r in (5, 6):
        n = int(b["seqlen"][r])
        b["in_item_id"][r] = 0
        b["item_id"][r] = 0
        b["in_item_id"][r, :n] = torch.arange(1, n + 1)
        b["item_id"][r, :n] = torch.arange(2, n + 2)
    params = _random_params(N, 64, 128, 2, seed=2)
    eng = SasrecEngine(N, 50, 64, 2, 128, 2, 1e-12, 0.0, B, "cuda")
    eng.load_named(params)
    plan = eng.make_plan(b["in_item_id"].to(dev), b["item_id"].to(dev), b["seqlen"].to(dev),
                         neg_item=b["neg_item"].squeeze(-1).contiguous().to(dev), sample_neg=False)
    eng.fwd_bwd(plan)
    loss, n = eng.loss_and_count()
    g_split = {k: v.clone() for k, v in eng.normalized_grads().items()}
    loss_o, _, grads_o = O.grads_of(params, b, 2, 2, 1e-12)
    assert n == int((b["item_id"] != 0).sum()) and abs(loss - float(loss_o)) < 2e-5
    for k, gv in g_split.items():
        assert relerr(gv, grads_o[k]) < REL, k
    monkeypatch.setenv("DR4SR_ATTN_NOSPLIT", "1")
    eng.fwd_bwd(plan)
    for k, gv in eng.normalized_grads().items():
        assert relerr(gv, g_split[k].cpu()) < 1e-5, k
    monkeypatch.delenv("DR4SR_ATTN_NOSPLIT")
    # with dropout: split and unsplit launches draw identical masks (element-indexed Philox), so they agree to atomics noise
    eng2 = SasrecEngine(N, 50, 64, 2, 128, 2, 1e-12, 0.5, B, "cuda", seed=7)
    eng2.load_named(params)
    plan2 = eng2.make_plan(b["in_item_id"].to(dev), b["item_id"].to(dev), b["seqlen"].to(dev),
                           neg_item=b["neg_item"].squeeze(-1).contiguous().to(dev), sample_neg=False)
    eng2.fwd_bwd(plan2)
    ga = {k: v.clone() for k, v in eng2.normalized_grads().items()}
    eng2.state[3] -= 1                                            # replay the same RNG step
    monkeypatch.setenv("DR4SR_ATTN_NOSPLIT", "1")
    eng2.fwd_bwd(plan2)
    for k, gv in eng2.normalized_grads().items():
        assert relerr(gv, ga[k].cpu()) < 1e-5, k


def test_ragged_edge_cases(dev):
    """seqlen 1, seqlen L, last-batch odd size, a row whose targets are all PAD."""
    from dr4sr_amd.engine import SasrecEngine
    from dr4sr_amd import _lib
    N, B = 300, 5
    gen = torch.Generator().manual_seed(3)
    sl = torch.tensor([1, 50, 2, 49, 3])
    idx = torch.zeros(B, 50, dtype=torch.long)
    tgt = torch.zeros(B, 50, dtype=torch.long)
    for i in range(B):
        idx[i, :sl[i]] = torch.randint(1, N, (int(sl[i]),), generator=gen)
        tgt[i, :sl[i]] = torch.randint(1, N, (int(sl[i]),), generator=gen)
    tgt[4] = 0                                         # fully masked row
    b = {"in_item_id": idx, "item_id": tgt, "seqlen": sl, "neg_item": torch.randint(1, N, (B, 50, 1), generator=gen)}
    params = _random_params(N, 64, 128, 2, seed=2)
    eng = SasrecEngine(N, 50, 64, 2, 128, 2, 1e-12, 0.0, 8, "cuda")     # max_batch 8 > B
    eng.load_named(params)
    plan = eng.make_plan(idx.to(dev), tgt.to(dev), sl.to(dev), neg_item=b["neg_item"].squeeze(-1).contiguous().to(dev),
                         sample_neg=False)
    eng.fwd_bwd(plan)
    loss, n = eng.loss_and_count()
    loss_o, q_o, grads_o = O.grads_of(params, b, 2, 2, 1e-12)
    assert n == int((tgt != 0).sum()) and abs(loss - float(loss_o)) < 2e-5
    for k, gv in eng.normalized_grads().items():
        assert relerr(gv, grads_o[k]) < REL, k
    q = eng.encode(plan, False, _lib.POOL_ORIGIN)
    assert relerr(q, q_o) < REL
    assert float(q[0, 1:].abs().max()) == 0.0          # rows >= seqlen are exactly zero ('origin' pooling)


def test_rows_indirection_equals_materialised_batch(dev):
    """a1: the batch is addressed as rows[] of the resident dataset tensors — same result as gathering first."""
    from dr4sr_amd.engine import SasrecEngine
    b, N = _toys_batch(64, False, seed=9)
    params = _random_params(N, 64, 128, 2, seed=4)
    eng = SasrecEngine(N, 50, 64, 2, 128, 2, 1e-12, 0.0, 16, "cuda")
    eng.load_named(params)
    rows = torch.tensor([5, 63, 0, 17, 17, 40, 2, 9, 33, 1, 8, 60, 21, 22, 23, 7], device=dev)
    neg = b["neg_item"].squeeze(-1)[rows.cpu()].contiguous().to(dev)
    full = {k: b[k].to(dev) for k in ("in_item_id", "item_id", "seqlen")}
    eng.fwd_bwd(eng.make_plan(full["in_item_id"], full["item_id"], full["seqlen"], rows=rows, neg_item=neg, sample_neg=False))
    l1, n1 = eng.loss_and_count()
    g1 = {k: v.clone() for k, v in eng.normalized_grads().items()}
    eng.fwd_bwd(eng.make_plan(full["in_item_id"][rows].contiguous(), full["item_id"][rows].contiguous(),
                              full["seqlen"][rows].contiguous(), neg_item=neg, sample_neg=False))
    l2, n2 = eng.loss_and_count()
    assert n1 == n2 and abs(l1 - l2) < 1e-6
    for k, v in eng.normalized_grads().items():
        assert relerr(v, g1[k].cpu()) < 1e-5, k


# ------------------------------------------------------------------------------------------------
def test_neg_sampler_uniform_never_pad(dev):
    from dr4sr_amd import _lib
    lib = _lib.load()
    n, N = 4000 * 50, 37
    out = torch.empty(n, dtype=torch.int64, device=dev)
    _lib.check(lib.dr4sr_neg_sample(_lib.ptr(out), n, N, 99, 1, _lib.cur_stream()), "neg")
    cnt = torch.bincount(out.cpu(), minlength=N).numpy()
    assert cnt[0] == 0 and out.min() >= 1 and out.max() <= N - 1
    exp = n / (N - 1)
    assert float(((cnt[1:] - exp) ** 2 / exp).sum()) < 80          # chi-square, 35 dof
    out2 = torch.empty(n, dtype=torch.int64, device=dev)
    _lib.check(lib.dr4sr_neg_sample(_lib.ptr(out2), n, N, 99, 2, _lib.cur_stream()), "neg")
    assert not torch.equal(out, out2)
    # in-step sampling: ids land in neg_item, in range, and feed the loss
    from dr4sr_amd.engine import SasrecEngine
    b, Nt = _toys_batch(32, False, seed=2)
    eng = SasrecEngine(Nt, 50, 64, 2, 128, 2, 1e-12, 0.0, 32, "cuda")
    eng.load_named(_random_params(Nt, 64, 128, 2, seed=6))
    negbuf = torch.zeros(32, 50, dtype=torch.int64, device=dev)
    plan = eng.make_plan(b["in_item_id"].to(dev), b["item_id"].to(dev), b["seqlen"].to(dev), neg_item=negbuf, sample_neg=True)
    eng.fwd_bwd(plan)
    assert int(negbuf.min()) >= 1 and int(negbuf.max()) <= Nt - 1
    bb = dict(b)
    bb["neg_item"] = negbuf.cpu().unsqueeze(-1)
    loss_o, _, _ = O.grads_of(_random_params(Nt, 64, 128, 2, seed=6), bb, 2, 2, 1e-12)
    assert abs(eng.loss_and_count()[0] - float(loss_o)) < 2e-5


@pytest.mark.parametrize("D", [64, 128])
def test_dense_scorer_fwd_bwd(dev, D):
    from dr4sr_amd import _lib
    lib = _lib.load()
    gen = torch.Generator().manual_seed(D)
    B, L, N = 9, 50, 500
    q = torch.randn(B, L, D, generator=gen)
    E = 0.3 * torch.randn(N, D, generator=gen)
    tgt = torch.randint(0, N, (B, L), generator=gen)
    tgt[:, 40:] = 0
    neg = torch.randint(1, N, (B, L, 1), generator=gen)
    w = torch.rand(B, L, generator=gen)
    qd, Ed, td, nd = q.to(dev), E.to(dev), tgt.to(dev), neg.squeeze(-1).contiguous().to(dev)
    pos = torch.empty(B, L, device=dev)
    ng = torch.empty(B, L, device=dev)
    lp = torch.empty(B, L, device=dev)
    st = torch.zeros(2, device=dev)
    _lib.check(lib.dr4sr_score_bce_fwd(_lib.ptr(qd), _lib.ptr(Ed), _lib.ptr(td), _lib.ptr(nd), _lib.ptr(pos), _lib.ptr(ng),
                                       _lib.ptr(lp), _lib.ptr(st), B, L, D, _lib.cur_stream()), "score fwd")
    qo = q.clone().requires_grad_(True)
    Eo = E.clone().requires_grad_(True)
    loss_nr, pos_o, ng_o = O.score_bce(qo, Eo, tgt, neg, reduce=False)
    n = int((tgt != 0).sum())
    assert int(st[0]) == n
    assert relerr(lp / n, loss_nr) < 1e-5
    valid = tgt != 0
    assert relerr(pos.cpu()[valid], pos_o[valid]) < 1e-5 and torch.isneginf(pos.cpu()[~valid]).all()
    assert relerr(ng.cpu().unsqueeze(-1), ng_o) < 1e-5
    (loss_nr * w).sum().backward()
    dq = torch.empty(B, L, D, device=dev)
    dE = torch.zeros(N, D, device=dev)
    scale = torch.tensor([1.0 / n], device=dev)
    _lib.check(lib.dr4sr_score_bce_bwd(_lib.ptr(qd), _lib.ptr(Ed), _lib.ptr(td), _lib.ptr(nd), _lib.ptr(w.to(dev)),
                                       _lib.ptr(scale), _lib.ptr(dq), _lib.ptr(dE), B, L, D, _lib.cur_stream()), "score bwd")
    assert relerr(dq, qo.grad) < 1e-5 and relerr(dE, Eo.grad) < 1e-5


@pytest.mark.parametrize("name", ["sasrec_d64", "sasrec_d128"])
def test_topk_vs_golden(dev, golden_dir, name):
    from dr4sr_amd import _lib
    lib = _lib.load()
    g, params, _ = load_golden(golden_dir, name)
    q = torch.from_numpy(g["eval.query_last"]).to(dev)
    E = params["item_embedding.weight"].to(dev)
    hist = torch.from_numpy(g["eval.user_hist"]).to(dev)
    B, D = q.shape
    k = g["eval.topk_items"].shape[1]
    sc = torch.empty(B, k, device=dev)
    it = torch.empty(B, k, dtype=torch.int64, device=dev)
    _lib.check(lib.dr4sr_full_score_topk(_lib.ptr(q), _lib.ptr(E), _lib.ptr(hist), _lib.ptr(sc), _lib.ptr(it), B, D,
                                         E.shape[0], hist.shape[1], k, _lib.cur_stream()), "topk")
    assert relerr(sc, g["eval.topk_score"]) < 1e-5
    same = float((it.cpu().numpy() == g["eval.topk_items"]).mean())
    # ids may only differ where two scores are equal to fp32 rounding (the GEMM sums in a different order than torch's matmul)
    assert same > 0.99, "top-k ids equal on %.4f of the positions (worst case allowed 0.99)" % same
    hit = torch.from_numpy(g["eval.item_id"]).view(-1, 1) == it.cpu()
    np.testing.assert_allclose(O.ndcg_at(hit, 20).numpy(), g["eval.ndcg@20"], rtol=1e-6)


@pytest.mark.parametrize("B,N,k,Lh", [(37, 50, 100, 20), (130, 2000, 20, 50), (64, 11925, 100, 50), (33, 3000, 100, 7), (40, 20034, 100, 50),
                                      (48, 6000, 100, 50), (70, 4096, 128, 50)])
@pytest.mark.parametrize("fused", [False, True])
def test_topk_workspace_path_equals_per_row_path(dev, monkeypatch, B, N, k, Lh, fused):
    """dr4sr_full_score_topk_ws returns what the per-row arg-max kernel returns: same ids wherever the scores are not within rounding of
    each other, scores of the returned ids, order, -inf handling (PAD, history, k > valid items).  fused (DR4SR_TOPK_FUSED, catalogs of
    >= 4 096 items): subset bound -> filtered emission -> wave-per-row candidate select instead of the [B, N] score matrix; N = 6000
    carries a 5 400-way tie at the top of every other row: the candidate buffers overflow and the batch falls back to the two kernels."""
    from dr4sr_amd import _lib
    lib = _lib.load()
    if fused:
        monkeypatch.setenv("DR4SR_TOPK_FUSED", "1")
        form = int(lib.dr4sr_full_score_topk_form(B, 64, N, Lh, k, int(lib.dr4sr_full_score_topk_workspace_bytes(B, N))))
        assert form >= 0, form
        if N == 4096:
            # the fused form's buffers (4 * 512 + 8 * 2048 + 8 = 18 440 bytes per row) do not fit in front of this catalog's score row
            # (16 384 bytes): under the switch this case runs the two-kernel form once more (it keeps running: it passed before the
            # form query could say so; tests/test_gpu_topk_exact.py holds the cases that ARE fused, from N = 4737 on)
            assert form & 1 == 0, form
        elif not form & 1:
            pytest.skip("dr4sr_full_score_topk_form = %d: the call is not fused for this shape (catalogs below 4096 items)" % form)
    g = torch.Generator().manual_seed(B + N)
    q = torch.randn(B, 64, generator=g).to(dev)
    E = (0.1 * torch.randn(N, 64, generator=g)).to(dev)
    E[0] = 0
    E[5] = E[7]                                                      # an exact tie: lower id first
    if N in (3000, 6000):
        E[100:N - 500] = E[100]                                      # 2400- / 5400-way tie: the candidate set overflows -> exact radix path
        q[::2] = E[100] * 50                                         # ... and it sits at the top for every other row
    hist = torch.randint(0, N, (B, Lh), generator=g).to(dev)
    outs = []
    for ws_path in (False, True):
        sc = torch.empty(B, k, device=dev)
        it = torch.empty(B, k, dtype=torch.int64, device=dev)
        if ws_path:
            nb = int(lib.dr4sr_full_score_topk_workspace_bytes(B, N))
            ws = torch.empty(nb // 4, device=dev)
            _lib.check(lib.dr4sr_full_score_topk_ws(_lib.ptr(q), _lib.ptr(E), _lib.ptr(hist), _lib.ptr(sc), _lib.ptr(it), B, 64, N, Lh, k,
                                                    _lib.ptr(ws), nb, _lib.cur_stream()), "topk_ws")
        else:
            _lib.check(lib.dr4sr_full_score_topk(_lib.ptr(q), _lib.ptr(E), _lib.ptr(hist), _lib.ptr(sc), _lib.ptr(it), B, 64, N, Lh, k,
                                                 _lib.cur_stream()), "topk")
        outs.append((sc.cpu(), it.cpu()))
    (sa, ia), (sb, ib) = outs
    fin = torch.isfinite(sa)
    assert bool((fin == torch.isfinite(sb)).all())
    assert float((sa[fin] - sb[fin]).abs().max()) < 1e-5
    assert float((ia == ib).float().mean()) > 0.999                 # fp32 summation order can swap near-ties only
    s = (q @ E.T).cpu()
    s[:, 0] = float("-inf")
    s.scatter_(1, hist.cpu(), float("-inf"))
    kk = min(k, N)
    assert float((s.gather(1, ib[:, :kk]) - sb[:, :kk])[torch.isfinite(sb[:, :kk])].abs().max()) < 1e-5
    assert bool((sb[:, 1:] <= sb[:, :-1]).all())
    srt = ib[:, :kk].sort(1)[0]
    assert bool((srt[:, 1:] != srt[:, :-1]).all())                   # no id twice
    if k > N:
        assert bool((ib[:, N:] == 0).all()) and bool(torch.isinf(sb[:, N:]).all())
    both = (ib == 5) | (ib == 7)                                     # the tie: whenever both ids are returned, 5 comes first
    for r in range(B):
        pos = both[r].nonzero().flatten().tolist()
        if len(pos) == 2 and bool(torch.isfinite(sb[r, pos]).all()):            # (not when the history masks one of them)
            assert int(ib[r, pos[0]]) == 5 and pos[1] == pos[0] + 1


@pytest.mark.parametrize("fused", [False, True])
def test_topk_workspace_path_large_catalog(dev, monkeypatch, fused):
    """N = 70 000 items: beyond what fits an LDS row — the selection reads the score workspace directly (history masked in place)"""
    from dr4sr_amd import _lib
    lib = _lib.load()
    if fused:
        monkeypatch.setenv("DR4SR_TOPK_FUSED", "1")
    B, N, k, Lh = 24, 70000, 100, 50
    g = torch.Generator().manual_seed(12)
    q = torch.randn(B, 64, generator=g).to(dev)
    E = (0.1 * torch.randn(N, 64, generator=g)).to(dev)
    hist = torch.randint(0, N, (B, Lh), generator=g).to(dev)
    sc = torch.empty(B, k, device=dev)
    it = torch.empty(B, k, dtype=torch.int64, device=dev)
    nb = int(lib.dr4sr_full_score_topk_workspace_bytes(B, N))
    ws = torch.empty(nb // 4, device=dev)
    _lib.check(lib.dr4sr_full_score_topk_ws(_lib.ptr(q), _lib.ptr(E), _lib.ptr(hist), _lib.ptr(sc), _lib.ptr(it), B, 64, N, Lh, k,
                                            _lib.ptr(ws), nb, _lib.cur_stream()), "topk_ws")
    s = q @ E.T
    s[:, 0] = float("-inf")
    s.scatter_(1, hist, float("-inf"))
    rs, ri = torch.topk(s, k, dim=1)
    assert float((rs - sc).abs().max()) < 1e-5
    assert float((ri == it).float().mean()) > 0.995
    assert float((s.gather(1, it) - sc).abs().max()) < 1e-5 and bool((sc[:, 1:] <= sc[:, :-1]).all())
    for r in range(B):
        assert not bool(torch.isin(it[r], hist[r]).any())          # no history item is ever recommended


@pytest.mark.parametrize("N,frac", [(3000, 0.5), (11925, 0.1), (500, 0.98)])
def test_topk_domain_item_mask_vs_oracle(dev, N, frac):
    """basemodel.py:358-360: items outside domain_item_mapping[eval_domain] are masked to -inf before the top-k (multi-domain
    datasets); item_blocked bytes through dr4sr_full_score_topk_masked_ws vs the oracle's full_score_topk(domain_items=...), incl. a
    domain with fewer than k items left"""
    from dr4sr_amd import _lib
    lib = _lib.load()
    B, k, Lh, D = 37, 100, 20, 64
    g = torch.Generator().manual_seed(N)
    q = torch.randn(B, D, generator=g)
    E = 0.1 * torch.randn(N, D, generator=g)
    hist = torch.randint(0, N, (B, Lh), generator=g)
    domain = torch.randperm(N - 1, generator=g)[:max(1, int((N - 1) * (1 - frac)))] + 1       # the items OF the domain (never PAD)
    blocked = torch.ones(N, dtype=torch.uint8)
    blocked[domain] = 0
    sc = torch.empty(B, k, device=dev)
    it = torch.empty(B, k, dtype=torch.int64, device=dev)
    nb = int(lib.dr4sr_full_score_topk_workspace_bytes(B, N))
    ws = torch.empty(nb // 4, device=dev)
    qd, Ed, hd, bd = q.to(dev), E.to(dev), hist.to(dev), blocked.to(dev)          # keep the device copies alive across the async launch
    _lib.check(lib.dr4sr_full_score_topk_masked_ws(_lib.ptr(qd), _lib.ptr(Ed), _lib.ptr(hd), _lib.ptr(bd),
                                                   _lib.ptr(sc), _lib.ptr(it), B, D, N, Lh, k, _lib.ptr(ws), nb, _lib.cur_stream()), "topk_masked")
    rs, ri = O.full_score_topk(q, E, hist, k, domain_items=domain)
    sc_c, it_c = sc.cpu(), it.cpu()
    finite = torch.isfinite(rs)
    assert torch.equal(torch.isfinite(sc_c), finite)
    assert float((rs[finite] - sc_c[finite]).abs().max()) < 1e-5
    assert float((ri[finite] == it_c[finite]).float().mean()) > 0.995, float((ri[finite] == it_c[finite]).float().mean())
    allowed = torch.zeros(N, dtype=torch.bool)
    allowed[domain] = True
    assert bool(allowed[it_c[finite]].all())                       # nothing outside the domain is ever recommended


def test_fuzz_odd_batches_vs_oracle(dev):
    """random odd batch sizes (1 .. 100), item counts down to 2, both widths, random lengths and PAD targets: tests/fuzz_parity.py"""
    import fuzz_parity
    assert fuzz_parity.main(trials=10, seed=3) < 5e-4


def test_training_trajectory_matches_oracle(dev):
    """25 consecutive Adam steps (dropout 0, given negatives, batches cycling through a small dataset): the loss curve and the final
    parameters of the fused step follow the oracle's trajectory (autograd restatement + torch.optim.Adam formula) — optimizer state,
    bias corrections and the tied table evolve identically, not just one step"""
    from dr4sr_amd.engine import SasrecEngine
    B, N, steps = 32, 200, 25
    b_all, _ = _toys_batch(4 * B, False, seed=21, n_items=N)
    params = _random_params(N, 64, 128, 2, seed=4)
    eng = SasrecEngine(N, 50, 64, 2, 128, 2, 1e-12, 0.0, B, "cuda", lr=1e-3)
    eng.load_named(params)
    p = {k: v.clone() for k, v in params.items() if k != "query_encoder.item_encoder.weight"}
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v = {k: torch.zeros_like(x) for k, x in p.items()}
    worst = 0.0
    for t in range(steps):
        sl = slice((t % 4) * B, (t % 4 + 1) * B)
        b = {k: x[sl].contiguous() for k, x in b_all.items()}
        plan = eng.make_plan(b["in_item_id"].to(dev), b["item_id"].to(dev), b["seqlen"].to(dev),
                             neg_item=b["neg_item"].squeeze(-1).contiguous().to(dev), sample_neg=False)
        eng.fwd_bwd(plan)
        loss, _ = eng.loss_and_count()
        eng.adam_step(plan)
        po = dict(p)
        po["query_encoder.item_encoder.weight"] = po["item_embedding.weight"]
        loss_o, _, g = O.grads_of(po, b, 2, 2, 1e-12)
        p = O.adam_step(p, g, m, v, t + 1, lr=1e-3)
        worst = max(worst, abs(loss - float(loss_o)))
    assert worst < 2e-4, worst
    got = eng.named_params() if hasattr(eng, "named_params") else {k: x.clone() for k, x in eng.views.items()}
    for k, x in p.items():
        d = (got[k].cpu() - x).abs()
        # Adam's normalised update amplifies fp32 noise where the true gradient is ~0 (e.g. the key part of in_proj_bias, exactly 0 by
        # softmax shift invariance: +-lr per step on both sides): bound the bulk tightly, the tail loosely
        assert float(d.mean()) < 1e-4 and float(d.max()) < 5e-3, (k, float(d.mean()), float(d.max()))


_SHAPES_OK = [(64, 1, 128, 2, 50), (64, 2, 256, 2, 50), (64, 1, 256, 1, 50), (128, 2, 128, 2, 50), (64, 2, 128, 1, 50), (64, 2, 128, 3, 50),
              (64, 2, 128, 4, 20), (64, 2, 128, 2, 1), (64, 2, 128, 2, 3), (128, 4, 128, 2, 20)]
_SHAPES_REFUSED = [(128, 4, 128, 2, 50), (64, 4, 128, 2, 50), (32, 2, 128, 2, 50), (64, 2, 64, 2, 50), (128, 2, 256, 2, 50),
                   (64, 2, 128, 2, 100), (128, 1, 128, 2, 50)]


@pytest.mark.gpu
@pytest.mark.parametrize("D,H,F,NL,L", _SHAPES_OK)
def test_every_accepted_encoder_shape_matches_oracle(D, H, F, NL, L):
    """head counts 1 / 2 / 4 (one-wave-per-head kernels next to the 2-head MFMA attention), FFN 128 / 256, 1-4 layers, L from 1 to 50:
    whatever check_shape (csrc/step.hip) accepts must reproduce the oracle's loss and every gradient (tests/config_probe.py)"""
    from dr4sr_amd.engine import SasrecEngine
    rng = np.random.default_rng(D + H + F + NL + L)
    B, N = 37, 211
    sl = rng.integers(1, L + 1, size=B); sl[0] = 1; sl[1] = L
    inp = np.zeros((B, L), dtype=np.int64); tgt = np.zeros((B, L), dtype=np.int64)
    for b in range(B):
        inp[b, :sl[b]] = rng.integers(1, N, size=sl[b]); tgt[b, :sl[b]] = rng.integers(0, N, size=sl[b])
    batch = {"in_item_id": torch.from_numpy(inp), "item_id": torch.from_numpy(tgt), "seqlen": torch.from_numpy(sl.astype(np.int64)),
             "neg_item": torch.from_numpy(rng.integers(1, N, size=(B, L, 1)))}
    params = _random_params(N, D, F, NL, L=L, seed=7)
    eng = SasrecEngine(N, L, D, H, F, NL, 1e-12, 0.0, B, "cuda")
    eng.load_named(params)
    plan = eng.make_plan(batch["in_item_id"].cuda(), batch["item_id"].cuda(), batch["seqlen"].cuda(),
                         neg_item=batch["neg_item"].squeeze(-1).contiguous().cuda(), sample_neg=False)
    eng.fwd_bwd(plan)
    loss, n = eng.loss_and_count()
    loss_o, _, grads_o = O.grads_of(params, batch, H, NL, 1e-12)
    assert n == int((batch["item_id"] != 0).sum())
    assert abs(loss - float(loss_o)) < 3e-5
    for k, v in eng.normalized_grads().items():
        assert relerr(v, grads_o[k]) < 5e-4, k


@pytest.mark.gpu
@pytest.mark.parametrize("D,L,separate,near", [(64, 64, False, False), (64, 64, True, False), (128, 64, False, False), (64, 50, False, False),
                                               (64, 64, False, True), (128, 50, False, True)])
def test_attention_in_tile_edge_cases(D, L, separate, near, monkeypatch):
    """csrc/attn_tile.h (the latency regime's attention, inside the 16-token tile kernels): sequences of the maximum length (the window's
    first row), lengths around the tile size (15 / 16 / 17 / 31 / 32 / 33: sequences that start or end on a tile boundary), single tokens,
    PAD ids INSIDE sequences (key_padding_mask, model/sasrec.py:48), and a batch whose token count is not a multiple of 16 — loss and every
    gradient against the oracle; `separate` = the one-workgroup-per-sequence launches on the same batch (DR4SR_ATTN_SEPARATE); `near` = the
    form short-sequence plans take at d = 128 (forced here: DR4SR_ATTN_TILE_NEAR): the tiles stage the near half of their window first and fetch the far
    rows on demand — which these long sequences demand in most tiles."""
    import ctypes as C
    from dr4sr_amd import _lib
    from dr4sr_amd.engine import SasrecEngine
    if separate:
        monkeypatch.setenv("DR4SR_ATTN_SEPARATE", "1")
    rng = np.random.default_rng(17 + D + L)
    N, H, F, NL = 157, 2, 128, 2
    sl = np.array([L, 1, L, 15, 16, 17, 1, 31, 32, 33, L - 1, 2, 16, 16, 1, 48, L, 3, 5, 8, 13], dtype=np.int64)
    B = len(sl)
    inp = np.zeros((B, L), dtype=np.int64); tgt = np.zeros((B, L), dtype=np.int64)
    for b in range(B):
        inp[b, :sl[b]] = rng.integers(1, N, size=sl[b]); tgt[b, :sl[b]] = rng.integers(0, N, size=sl[b])
    for b in (0, 3, 7, 16):                                  # PAD keys inside a sequence (never at position 0: that row would be all-masked)
        pos = rng.choice(np.arange(1, sl[b]), size=min(3, sl[b] - 1), replace=False)
        inp[b, pos] = 0
    batch = {"in_item_id": torch.from_numpy(inp), "item_id": torch.from_numpy(tgt), "seqlen": torch.from_numpy(sl),
             "neg_item": torch.from_numpy(rng.integers(1, N, size=(B, L, 1)))}
    assert int(sl.sum()) % 16 != 0
    params = _random_params(N, D, F, NL, L=L, seed=9)
    eng = SasrecEngine(N, L, D, H, F, NL, 1e-12, 0.0, B, "cuda")
    eng.load_named(params)
    plan = eng.make_plan(batch["in_item_id"].cuda(), batch["item_id"].cuda(), batch["seqlen"].cuda(),
                         neg_item=batch["neg_item"].squeeze(-1).contiguous().cuda(), sample_neg=False)
    if near:
        monkeypatch.setenv("DR4SR_ATTN_TILE_NEAR", "1")
    assert bool(int(_lib.load().dr4sr_sasrec_at_scale(C.byref(plan))) & 4) == (not separate)
    for _ in range(2):                                       # twice: the second pass finds the first one's dK | dV in the workspace
        eng.fwd_bwd(plan)
    loss, n = eng.loss_and_count()
    loss_o, _, grads_o = O.grads_of(params, batch, H, NL, 1e-12)
    assert n == int((batch["item_id"] != 0).sum())
    assert abs(loss - float(loss_o)) < 3e-5
    for k, v in eng.normalized_grads().items():
        assert relerr(v, grads_o[k]) < 5e-4, k


@pytest.mark.gpu
def test_second_backward_on_one_forward_gives_the_same_gradients():
    """dr4sr_sasrec_encode_bwd twice on one dr4sr_sasrec_encode (autograd's retain_graph case): with the attention inside the tile kernels
    the dK | dV rows are accumulated with atomics, so every backward pass zeroes them in the launch in front of their accumulation
    (k_pack for the last layer, k_post_bwd of the layer above for the others)"""
    from dr4sr_amd import _lib
    from dr4sr_amd.engine import SasrecEngine
    rng = np.random.default_rng(5)
    N, B, L, D = 120, 40, 50, 64
    sl = rng.integers(1, L + 1, size=B)
    inp = np.zeros((B, L), dtype=np.int64)
    for b in range(B):
        inp[b, :sl[b]] = rng.integers(1, N, size=sl[b])
    eng = SasrecEngine(N, L, D, 2, 128, 2, 1e-12, 0.0, B, "cuda")
    eng.load_named(_random_params(N, D, 128, 2, seed=11))
    plan = eng.make_plan(torch.from_numpy(inp).cuda(), None, torch.from_numpy(sl.astype(np.int64)).cuda())
    q = eng.encode(plan, True, _lib.POOL_MEAN)
    g = torch.randn_like(q)
    grads = []
    for _ in range(2):
        eng.grads.zero_()
        eng.encode_bwd(plan, True, _lib.POOL_MEAN, g)
        grads.append(eng.grads[:eng.n_params].cpu())
    assert relerr(grads[1], grads[0]) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("D,H,F,NL,L", _SHAPES_REFUSED)
def test_unsupported_encoder_shapes_are_refused_up_front(D, H, F, NL, L):
    """a shape without kernels is an error when the engine is built — not a failed launch, never a wrong number"""
    from dr4sr_amd.engine import SasrecEngine
    from dr4sr_amd import _lib
    with pytest.raises(_lib.Dr4srError, match="DR4SR_E_SHAPE"):
        SasrecEngine(211, L, D, H, F, NL, 1e-12, 0.0, 8, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("D,H,F,NL,L", [(64, 1, 128, 2, 50), (64, 2, 256, 3, 50), (128, 4, 128, 2, 20), (64, 2, 128, 1, 50), (64, 2, 128, 4, 20)])
def test_dropout_sites_of_every_shape_match_oracle_with_same_masks(D, H, F, NL, L):
    """the dropout sites (embedding, attention probabilities, projection, activation, FFN: 4 per layer) of the shapes beyond the golden
    fixtures' 2 layers x 2 heads: the library's own Philox masks, materialised through dr4sr_dropout_mask, fed to the oracle"""
    from dr4sr_amd.engine import SasrecEngine
    rng = np.random.default_rng(11 * D + H + F + NL + L)
    B, N, p = 23, 157, 0.3
    sl = rng.integers(1, L + 1, size=B); sl[0] = 1; sl[1] = L
    inp = np.zeros((B, L), dtype=np.int64); tgt = np.zeros((B, L), dtype=np.int64)
    for b in range(B):
        inp[b, :sl[b]] = rng.integers(1, N, size=sl[b]); tgt[b, :sl[b]] = rng.integers(1, N, size=sl[b])
    batch = {"in_item_id": torch.from_numpy(inp), "item_id": torch.from_numpy(tgt), "seqlen": torch.from_numpy(sl.astype(np.int64)),
             "neg_item": torch.from_numpy(rng.integers(1, N, size=(B, L, 1)))}
    params = _random_params(N, D, F, NL, L=L, seed=3)
    eng = SasrecEngine(N, L, D, H, F, NL, 1e-12, p, B, "cuda", seed=99)
    eng.load_named(params)
    plan = eng.make_plan(batch["in_item_id"].cuda(), batch["item_id"].cuda(), batch["seqlen"].cuda(),
                         neg_item=batch["neg_item"].squeeze(-1).contiguous().cuda(), sample_neg=False)
    eng.fwd_bwd(plan)
    step = int(eng.state[3])
    cu = torch.cat([torch.zeros(1, dtype=torch.long), batch["seqlen"].cumsum(0)])
    masks = _masks_from_engine(eng, cu, batch["seqlen"], B, L, D, H, F, NL, step)
    loss_o, _, grads_o = O.grads_of(params, batch, H, NL, 1e-12, masks=masks, pdrop=p)
    loss, n = eng.loss_and_count()
    assert abs(loss - float(loss_o)) < 2e-5 * max(1.0, abs(float(loss_o)))
    for k, gv in eng.normalized_grads().items():
        assert relerr(gv, grads_o[k]) < REL, k


@pytest.mark.gpu
@pytest.mark.parametrize("B,D,p", [(8192, 64, 0.0), (8192, 64, 0.5), (4096, 128, 0.3)])
def test_persistent_attention_lists_longer_than_the_grid(dev, monkeypatch, at_scale, B, D, p):
    """thousands of sequences per length class: every workgroup of the persistent attention launches walks SEVERAL list entries, i.e.
    the software-pipelined loop (rows of i+1 / cu words of i+2 / list entry of i+3 in flight) runs its steady state and its drain.
    Checked against the one-workgroup-per-sequence launch of the same step (itself checked against the oracle above); with dropout the
    two draw identical masks (element-indexed Philox).  (Round 6: DR4SR_ATTN_LISTS selects the lists; default = csrc/attn_wave.hip.)"""
    from dr4sr_amd.engine import SasrecEngine
    monkeypatch.setenv("DR4SR_ATTN_LISTS", "1")
    b, N = _toys_batch(B, False, seed=21)
    params = _random_params(N, D, 128, 2, seed=4)
    eng = SasrecEngine(N, 50, D, 2, 128, 2, 1e-12, p, B, "cuda", seed=11)
    eng.load_named(params)
    plan = eng.make_plan(b["in_item_id"].to(dev), b["item_id"].to(dev), b["seqlen"].to(dev),
                         neg_item=b["neg_item"].squeeze(-1).contiguous().to(dev), sample_neg=False)
    eng.fwd_bwd(plan)
    loss_a, n_a = eng.loss_and_count()
    ga = {k: v.clone() for k, v in eng.normalized_grads().items()}
    eng.state[3] -= 1                                             # replay the same RNG step
    monkeypatch.setenv("DR4SR_ATTN_NOSPLIT", "1")
    eng.fwd_bwd(plan)
    loss_b, n_b = eng.loss_and_count()
    assert n_a == n_b == int((b["item_id"] != 0).sum()) and abs(loss_a - loss_b) < 1e-6
    for k, gv in eng.normalized_grads().items():
        assert relerr(gv, ga[k].cpu()) < 1e-5, k
