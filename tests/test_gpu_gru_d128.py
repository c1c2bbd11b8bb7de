"""GRU4Rec at embed_dim 128 on the GPU (dr4sr_gru4rec_* with D = 128): the reference's own run (tests/golden/gru4rec_d128*.npz), the
oracle on every accepted shape, the fused glue kernels against the separate launches, the dropout element index, the at-scale launch
forms, deterministic mode, train_steps, refusals, and the model / MetaModel surface.  Bounds are those of tests/test_gpu_gru.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import gru4rec_oracle as GO  # noqa: E402
from oracle import metamodel_oracle as MO  # noqa: E402

import _gru_d128  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 3e-4
D = 128


def relerr(a, b):
    a = a.detach().cpu().double()
    b = torch.as_tensor(b).double()
    return float((a - b).abs().max() / max(1e-12, float(b.abs().max())))


def random_params(N, H, NL, gen):
    from dr4sr_amd.gru_engine import gru_param_names, gru_param_shapes
    params = {nme: 0.08 * torch.randn(shp, generator=gen) for nme, shp in zip(gru_param_names(NL), gru_param_shapes(N, D, H, NL))}
    params["item_embedding.weight"][0] = 0
    return params


def random_batch(B, L, N, gen, sl=None):
    """random lengths including 1 and L (first and last row), targets with PAD entries"""
    if sl is None:
        sl = torch.randint(1, L + 1, (B,), generator=gen)
    sl[0] = 1
    sl[-1] = L
    inp = torch.zeros(B, L, dtype=torch.int64)
    tgt = torch.zeros(B, L, dtype=torch.int64)
    for r in range(B):
        n = int(sl[r])
        inp[r, :n] = torch.randint(1, N, (n,), generator=gen)
        tgt[r, :n] = torch.randint(0, N, (n,), generator=gen)
    return {"in_item_id": inp, "item_id": tgt, "seqlen": sl, "neg_item": torch.randint(1, N, (B, L, 1), generator=gen)}


def engine_and_plan(params, b, H, NL, L, N, p_drop=0.0, sample_neg=False):
    from dr4sr_amd.gru_engine import GruEngine
    B = b["in_item_id"].shape[0]
    eng = GruEngine(N, L, D, H, NL, p_drop, B, "cuda", seed=5)
    eng.load_named(params)
    dev = eng.device
    neg = b["neg_item"].squeeze(-1).contiguous().to(dev)
    plan = eng.make_plan(b["in_item_id"].to(dev), b["item_id"].to(dev), b["seqlen"].to(dev), neg_item=neg, sample_neg=sample_neg)
    return eng, plan, neg


def check_vs_oracle(eng, params, b, NL, **kw):
    op = dict(params)
    op["query_encoder.0.1.weight"] = params["item_embedding.weight"]
    loss_o, _, grads_o = GO.grads_of(op, b, NL, **kw)
    loss, n = eng.loss_and_count()
    print("loss", loss, "oracle", float(loss_o))
    assert n == int((b["item_id"] != 0).sum()) and abs(loss - float(loss_o)) < 3e-5
    for k, gv in eng.normalized_grads().items():
        e = relerr(gv, grads_o[k])
        print(k, e)
        assert e < REL, k


def gru_case(B, H, NL, L, N=200, sl=None):
    gen = torch.Generator().manual_seed(1000 + B)
    b = random_batch(B, L, N, gen, sl)
    params = random_params(N, H, NL, gen)
    eng, plan, _ = engine_and_plan(params, b, H, NL, L, N)
    eng.fwd_bwd(plan)
    check_vs_oracle(eng, params, b, NL)
    eng.check_device_error()
    return eng, plan


# ------------------------------------------------------------------------------------------------ the reference's own run
def test_gru4rec_d128_vs_golden():
    from dr4sr_amd import _lib
    from dr4sr_amd.gru_engine import GruEngine
    g = _gru_d128.load()
    params = {k[6:]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith("param.")}
    b = {k[6:]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith("batch.")}
    B = b["in_item_id"].shape[0]
    eng = GruEngine(int(g["meta.num_items"]), 50, D, int(g["meta.hidden_size"]), int(g["meta.layer_num"]), 0.0, B, "cuda",
                    lr=float(g["meta.lr"]), weight_decay=float(g["meta.weight_decay"]))
    eng.load_named(params)
    dev = eng.device
    idx, tgt, sl = b["in_item_id"].to(dev), b["item_id"].to(dev), b["seqlen"].to(dev)
    neg = b["neg_item"].squeeze(-1).contiguous().to(dev)
    plan = eng.make_plan(idx, tgt, sl, neg_item=neg, sample_neg=False)
    q = eng.encode(plan, False, _lib.POOL_ORIGIN)
    assert q.shape[-1] == D and relerr(q, g["out.query"]) < REL
    ql = eng.encode(eng.make_plan(torch.from_numpy(g["eval.in_item_id"].copy()).to(dev), None,
                                  torch.from_numpy(g["eval.seqlen"].copy()).to(dev)), False, _lib.POOL_LAST)
    assert relerr(ql, g["eval.query_last"]) < REL
    eng.fwd_bwd(plan)
    loss, n = eng.loss_and_count()
    print("loss", loss, "reference", float(g["out.loss"]))
    assert n == int((b["item_id"] != 0).sum()) and abs(loss - float(g["out.loss"])) < 1e-5
    for k, gv in eng.normalized_grads().items():
        assert relerr(gv, g["grad." + k]) < REL, k
    eng.adam_step()
    for k, v in eng.views.items():
        well = np.abs(g["grad." + k]) > 1e-4
        d = v.cpu().numpy() - g["adam1." + k]
        assert np.abs(d[well]).max(initial=0) < 1e-5 and np.abs(d).max() < 1.1e-3, k


# ------------------------------------------------------------------------------------------------ oracle
@pytest.mark.parametrize("H,NL,L", [(128, 1, 64), (128, 2, 50), (256, 1, 50), (256, 2, 1), (256, 2, 50), (128, 3, 7), (256, 3, 20)])
def test_every_accepted_shape_vs_oracle(H, NL, L):
    """B = 37 (T is no multiple of 16 but for L = 1, where T = 37), lengths include 1 and L; two layers take the layer wavefront, one and
    three the per-layer launches"""
    gru_case(37, H, NL, L)


@pytest.mark.parametrize("B", [1, 3, 17, 100])
def test_odd_batch_sizes_vs_oracle(B):
    """partial 16-sequence groups and partial 16-token tiles"""
    gru_case(B, 256, 2, 50)


def test_fused_glue_equals_separate_launches():
    """the same plan and RNG step through k_gru_embed_gi / k_gru_mid / k_gru_dx_embed and through the separate launches
    (DR4SR_GRU_NOFUSE_GLUE), dropout 0.2, negatives drawn in the kernels"""
    from dr4sr_amd import _lib
    N, H, NL, L, B = 200, 256, 2, 50, 37
    gen = torch.Generator().manual_seed(77)
    b = random_batch(B, L, N, gen)
    params = random_params(N, H, NL, gen)
    eng, plan, neg = engine_and_plan(params, b, H, NL, L, N, p_drop=0.2, sample_neg=True)
    rng = eng.state[3:4].clone()
    out = []
    try:
        for nofuse in (None, "1"):
            _lib.set_env("DR4SR_GRU_NOFUSE_GLUE", nofuse)
            eng.state[3:4].copy_(rng)
            neg.fill_(-7)
            eng.fwd_bwd(plan)
            eng.check_device_error()
            out.append((eng.loss_and_count(), {k: v.clone() for k, v in eng.normalized_grads().items()}, neg.clone()))
    finally:
        _lib.set_env("DR4SR_GRU_NOFUSE_GLUE", None)
    ((la, na), ga, nega), ((lb, nb), gb, negb) = out
    print("fused", la, na, "separate", lb, nb)
    assert na == nb == int((b["item_id"] != 0).sum())
    assert abs(la - lb) < 3e-5
    assert torch.equal(nega, negb) and int(nega.min()) >= 1                  # same Philox draws, every position written
    for k in ga:
        e = relerr(ga[k], gb[k].cpu())
        print(k, e)
        assert e < REL, k


@pytest.mark.parametrize("nofuse", [False, True])
def test_dropout_element_index(monkeypatch, nofuse):
    """B = 64, p = 0.2: the mask of element ((b L + pos) 128 + c) read back from the library and handed to the oracle pins the index of the
    fused gather and of the masked scatter (and of k_embed_fwd / k_embed_bwd<128> with the separate launches)"""
    if nofuse:
        monkeypatch.setenv("DR4SR_GRU_NOFUSE_GLUE", "1")
    N, H, NL, L, B, p = 200, 256, 2, 50, 64, 0.2
    gen = torch.Generator().manual_seed(64)
    b = random_batch(B, L, N, gen)
    params = random_params(N, H, NL, gen)
    eng, plan, _ = engine_and_plan(params, b, H, NL, L, N, p_drop=p)
    eng.fwd_bwd(plan)
    step = int(eng.state[3])
    mask = eng.dropout_mask(B * L * D, 0, step).view(B, L, D).cpu()
    assert 0.15 < float((mask == 0).float().mean()) < 0.25
    check_vs_oracle(eng, params, b, NL, mask=mask, pdrop=p)


def test_at_scale_launch_forms_vs_oracle():
    """B L = 16 400 is above the latency boundary (16 384 tokens of capacity): 64-row GEMM tiles with K or N = 128, the separate glue launches"""
    B, L = 328, 50
    gen = torch.Generator().manual_seed(328)
    sl = torch.randint(1, 6, (B,), generator=gen)
    gru_case(B, 128, 1, L, sl=sl)


@pytest.mark.parametrize("B", [37, 100])
def test_deterministic_mode(monkeypatch, B):
    """DR4SR_DETERMINISTIC: k_gru_det_rows<128>, the owner-computed table gradient on rows of 128 floats and the stored weight-gradient
    blocks: two fwd_bwd runs from the same state are bit-identical and match the oracle"""
    monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    eng, plan = gru_case(B, 256, 2, 50)
    g_a = eng.grads.clone()
    eng.fwd_bwd(plan)
    torch.cuda.synchronize()
    assert torch.equal(g_a, eng.grads)
    # ... and with dropout and in-kernel negatives from the same RNG step
    N, H, NL, L = 200, 256, 2, 50
    gen = torch.Generator().manual_seed(B)
    b = random_batch(B, L, N, gen)
    eng2, plan2, _ = engine_and_plan(random_params(N, H, NL, gen), b, H, NL, L, N, p_drop=0.2, sample_neg=True)
    rng = eng2.state[3:4].clone()
    eng2.fwd_bwd(plan2)
    g_b = eng2.grads.clone()
    eng2.state[3:4].copy_(rng)
    eng2.fwd_bwd(plan2)
    torch.cuda.synchronize()
    assert torch.equal(g_b, eng2.grads) and bool(torch.isfinite(g_b).all())


def test_train_steps_equal_repeated_single_steps():
    """tests/test_gpu_gru.py's train_steps case at D = 128 (n = 5, B = 96, U = 700, dropout 0.2, in-kernel negatives)"""
    from dr4sr_amd.data.synthetic import make_rows
    from dr4sr_amd.gru_engine import GruEngine
    N, U, B, H, n = 3000, 700, 96, 256, 5
    rows = make_rows(n_rows=U, n_items=N, seed=8)
    params = random_params(N, H, 2, torch.Generator().manual_seed(2))
    out = []
    for mode in ("steps", "single"):
        eng = GruEngine(N, 50, D, H, 2, 0.2, B, "cuda", seed=5, lr=1e-3, weight_decay=1e-4)
        eng.load_named(params)
        dev = eng.device
        data = {k: torch.from_numpy(rows[k]).to(dev) for k in ("in_item_id", "item_id", "seqlen")}
        perm = torch.randperm(U, generator=torch.Generator().manual_seed(3)).to(dev)
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        rows_buf = torch.zeros(B, dtype=torch.int64, device=dev)
        log = torch.zeros(16, dtype=torch.float32, device=dev)
        plan = eng.make_plan(data["in_item_id"], data["item_id"], data["seqlen"], rows=rows_buf, sample_neg=True,
                             perm_sel=(perm, B, 0, counter), loss_log=log)
        if mode == "steps":
            eng.train_steps(plan, n)
        else:
            for _ in range(n):
                eng.train_step(plan)
        eng.check_device_error()
        assert int(counter) == n and int(eng.state[0]) == n
        assert torch.equal(rows_buf, perm[(n - 1) * B:n * B])
        out.append((eng.params.clone(), log.clone()))
    (pa, la), (pb, lb) = out
    assert float(la[:n].min()) > 0 and torch.allclose(la, lb, rtol=1e-5, atol=1e-6), (la, lb)
    assert float((pa - pb).abs().max()) < 2e-5 * float(pb.abs().max())      # fp32 atomics order only


@pytest.mark.parametrize("Dbad", [32, 96, 192, 256])
def test_other_widths_are_refused(Dbad):
    from dr4sr_amd import _lib
    from dr4sr_amd.gru_engine import GruEngine
    with pytest.raises(_lib.Dr4srError):
        GruEngine(200, 50, Dbad, 256, 2, 0.0, 8, "cuda", seed=5)
    p = _lib.GruPlan()
    p.abi_version = _lib.ABI_VERSION
    p.B, p.L, p.D, p.H, p.n_layer, p.n_items = 8, 50, Dbad, 256, 2, 200
    assert _lib.load().dr4sr_gru4rec_workspace_bytes(C.byref(p)) == -2          # DR4SR_E_SHAPE (include/dr4sr_hip.h)
    p.D = D
    assert _lib.load().dr4sr_gru4rec_workspace_bytes(C.byref(p)) > 0


# ------------------------------------------------------------------------------------------------ model level
def model_config(n_items=150, n_rows=600, batch=64, epochs=3):
    return {
        "data": {"dataset": "synthetic-toys", "domain_name_list": ["toy"], "max_seq_len": 50, "dataset_class": "synthetic",
                 "train_file": "", "n_items": n_items, "n_rows": n_rows, "n_eval_rows": 128, "seed": 5},
        "model": {"model": "GRU4Rec", "embed_dim": D, "loss_fn": "bce", "hidden_size": 128, "layer_num": 2, "head_num": 2,
                  "dropout_rate": 0.2, "activation": "gelu", "layer_norm_eps": 1e-12},
        "train": {"batch_size": batch, "early_stop_mode": "max", "early_stop_patience": 20, "epochs": epochs, "device": "cuda",
                  "optimizer": "adam", "learning_rate": 0.001, "weight_decay": 1e-4, "num_neg": 1, "seed": 2023, "hip_graph": True},
        "eval": {"batch_size": 128, "cutoff": [20, 10], "val_metrics": ["ndcg", "recall"], "test_metrics": ["ndcg", "recall"],
                 "topk": 100, "save_path": "./saved/"},
    }


def test_model_fit_checkpoint_evaluate(tmp_path, monkeypatch):
    from dr4sr_amd.utils import prepare_datasets, prepare_model, seed_everything
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("DR4SR_CONFIG_DIR", os.path.join(ROOT, "configs"))
    cfg = model_config()
    seed_everything(cfg["train"]["seed"])
    ds = prepare_datasets(cfg)
    model = prepare_model(cfg, ds)
    N = model.num_items
    losses = []
    orig_end = model.training_epoch_end

    def record(output_list):
        r = orig_end(output_list)
        losses.append(float(model.logged_metrics["train_loss_0"]))          # the epoch's mean training loss
        return r
    model.training_epoch_end = record
    model.fit()
    torch.cuda.synchronize()
    print("epoch losses", losses)
    assert len(losses) == 3 and all(np.isfinite(losses)) and losses[-1] < losses[0]
    sd = model.state_dict()
    want = {"item_embedding.weight": (N, D), "query_encoder.0.1.weight": (N, D), "query_encoder.1.weight": (D, 128),
            "query_encoder.1.bias": (D,)}
    for l in range(2):
        want[f"query_encoder.0.3.gru.weight_ih_l{l}"] = (384, D if l == 0 else 128)
        want[f"query_encoder.0.3.gru.weight_hh_l{l}"] = (384, 128)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    path = os.path.join(cfg["eval"]["save_path"], model.ckpt_path)          # written by fit()'s early-stopping callback
    saved = torch.load(path, weights_only=False, map_location="cpu")["parameters"]
    assert {k: tuple(v.shape) for k, v in saved.items()} == want
    seed_everything(1)
    model2 = prepare_model(cfg, ds)
    model2._init_model(ds[0])
    assert not torch.equal(model2.state_dict()["query_encoder.1.weight"].cpu(), saved["query_encoder.1.weight"])
    model2.load_checkpoint(path)
    for k, v in model2.state_dict().items():
        assert torch.equal(v.cpu(), saved[k]), k
    out = model.evaluate()
    assert {"ndcg@20", "recall@20"} <= set(out) and all(np.isfinite(v) for v in out.values())


def meta_config(**kw):
    from test_gpu_meta import make_config
    cfg = make_config(150, sub="GRU4Rec", **kw)
    cfg["model"]["embed_dim"] = D
    cfg["model"]["sub_overrides"]["model"].update({"embed_dim": D, "hidden_size": 128})
    return cfg


def test_metamodel_fit_end_to_end(tmp_path, monkeypatch):
    """tests/test_gpu_meta.py test_metamodel_fit_end_to_end[GRU4Rec] at embed_dim 128"""
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("DR4SR_CONFIG_DIR", os.path.join(ROOT, "configs"))
    from dr4sr_amd import quickstart
    out = quickstart.run(meta_config(dropout=0.2, n_rows=300, batch=64, epochs=3, warmup=0, interval=2))
    assert {"ndcg@20", "recall@20"} <= set(out) and all(np.isfinite(v) for v in out.values())


def test_metamodel_weighted_inner_step_vs_oracle(monkeypatch):
    """one weighted inner step (dense composition: encode, dr4sr_score_bce_*, dr4sr_meta_select_*_d, encode_bwd): the sub-model's
    gradients against autograd of oracle.metamodel_oracle.train_loss over gru4rec_losses (oracle/gru4rec_oracle.py), explicit Gumbel
    noise, dropout 0; bound 1e-4 relative, as tests/test_gpu_meta.py between its two forms"""
    from test_gpu_meta import build, rel
    cfg = meta_config(dropout=0.0, n_rows=128, batch=32)
    ds, m = build(cfg, monkeypatch)
    m.train()
    eng = m.engine
    assert eng.D == D and m.embed_dim == D and not m._fused_ok()
    loader = ds[0].get_loader()
    bt = m._local_batch(loader, m._perm(loader), 0)
    bt["neg_item"] = m._neg_sampling(bt)
    B, L = bt["item_id"].shape
    gum = -torch.empty(B * L, 2).exponential_(generator=torch.Generator().manual_seed(9)).log()
    m._gumbel = gum.to(m.device).contiguous()
    w, lp = m._weighted_fwd_bwd(bt)
    nv = float(eng.grads[eng.n_params])
    p = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in eng.views.items()}
    p["query_encoder.0.1.weight"] = p["item_embedding.weight"]
    meta = {k: v.detach().cpu().clone() for k, v in m.meta_module.state_dict().items()}
    cb = {k: v.cpu() for k, v in bt.items() if torch.is_tensor(v)}
    loss = MO.train_loss(MO.gru4rec_losses(2), p, meta, cb, gum.view(B, L, 2), m._tau_eff(), cfg["model"]["tau_min"])
    names = list(eng.views)
    grads = torch.autograd.grad(loss, [p[k] for k in names])
    # the oracle's per-position losses carry the 1 / n_valid of the reduced loss (oracle/sasrec_oracle.py score_bce); the step leaves sums
    lsum = float(eng.grads[eng.n_params + 1])
    print("weighted loss: kernel sum", lsum, "n_valid", nv, "oracle", float(loss))
    assert abs(lsum / nv - float(loss)) < 3e-5 * max(1.0, abs(float(loss)))
    for k, g in zip(names, grads):
        e = rel((eng.grad_views[k] / nv).cpu().numpy(), g.numpy())
        print(k, e)
        assert e < 1e-4, k
