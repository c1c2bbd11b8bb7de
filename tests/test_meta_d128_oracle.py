"""Pin the DR4SR+ fixture at embed_dim 128 (tests/golden/metamodel_sasrec_d128*.npz, made by RUNNING the reference's MetaModel with
model.embed_dim = 128: tools/make_meta_d128_golden.py) with the unchanged oracle/metamodel_oracle.py.  CPU only.  The bars are those of
tests/test_meta_oracle.py; the finite-difference form is checked at rel_step 3e-4 and 5e-4 (the product's default) — at this width
rel_step 1e-3 measures 2.9e-4 .. 3.0e-4, on the 3e-4 bar, and is not a case here."""
import numpy as np
import pytest
import torch

from oracle import metamodel_oracle as MO

import _meta_d128


def rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.fixture(scope="module")
def case():
    g = _meta_d128.load()
    pick = lambda pre: {k[len(pre):]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith(pre)}
    p = pick("param.")
    p.pop("query_encoder.item_encoder.weight", None)            # tied to item_embedding.weight
    cfg = {"H": int(g["meta.head_num"]), "n_layer": int(g["meta.layer_num"]), "eps": float(g["meta.layer_norm_eps"])}
    return g, p, pick("meta_param."), pick("train."), pick("val."), cfg


def scalars(g):
    return (torch.from_numpy(g["inner.gumbel"].copy()), float(g["meta.tau"][0]), float(g["meta.tau_min"]),
            float(g["meta.hpo_learning_rate"]))


def test_fixture_is_d128(case):
    g, p, meta, bt, bv, cfg = case
    assert meta["0.weight"].shape == (128, 128) and meta["2.weight"].shape == (2, 128)
    assert p["item_embedding.weight"].shape == (int(g["meta.num_items"]), 128)
    assert g["inner.query"].shape[-1] == 128 and str(g["meta.sub_model"]) == "SASRec"
    assert sum(v.numel() for v in meta.values()) == 16770


def test_weighted_inner_step(case):
    g, p, meta, bt, bv, cfg = case
    gum, tau, tmin, _ = scalars(g)
    f = MO.sasrec_losses(cfg)
    P = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    M = {k: v.clone().requires_grad_(True) for k, v in meta.items()}
    lp, q = f(P, bt, False)
    loss, w = MO.weighted_loss(lp, q, M, gum, tau, tmin, bt["user_id"], bt["item_id"])
    np.testing.assert_allclose(q.detach().numpy(), g["inner.query"], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(lp.detach().numpy(), g["inner.loss_pos"], rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(w.detach().numpy(), g["inner.weight"], rtol=1e-5, atol=1e-7)
    assert (w.detach().numpy()[1][bt["item_id"][1].numpy() != 0] == 1.0).all()     # the user_id == 0 row
    print("weighted loss", float(loss.detach()), "reference", float(g["inner.loss"]))
    np.testing.assert_allclose(float(loss.detach()), float(g["inner.loss"]), rtol=2e-6)
    loss.backward()
    worst = 0.0
    for k, v in P.items():
        e = rel(v.grad.numpy() if v.grad is not None else np.zeros(v.shape), g["inner.grad." + k])
        if np.abs(g["inner.grad." + k]).max() >= 1e-7:
            worst = max(worst, e)
            assert e < 2e-4, (k, e)
    for k, v in M.items():
        e = rel(v.grad.numpy(), g["inner.meta_grad." + k])
        print("phi gradient", k, e)
        assert e < 2e-4, (k, e)
    print("worst inner gradient rel. error", worst)


def test_hypergradient_exact_and_meta_sgd(case):
    g, p, meta, bt, bv, cfg = case
    gum, tau, tmin, hlr = scalars(g)
    f = MO.sasrec_losses(cfg)
    hg, gval, _ = MO.hypergrad_exact(f, p, meta, bt, bv, gum, tau, tmin, hlr)
    for k, v in gval.items():
        assert rel(v.numpy(), g["outer.grad_val." + k]) < 2e-4 or np.abs(g["outer.grad_val." + k]).max() < 1e-7, k
    ref = np.concatenate([g["outer.hypergrad." + k].ravel() for k in MO.META_NAMES])
    print("exact hyper-gradient rel. error", rel(np.concatenate([hg[k].numpy().ravel() for k in MO.META_NAMES]), ref))
    for k in MO.META_NAMES:
        assert rel(hg[k].numpy(), g["outer.hypergrad." + k]) < 5e-4, (k, rel(hg[k].numpy(), g["outer.hypergrad." + k]))
    # two MetaOptimizer steps (clip 10, SGD momentum 0.9 + weight decay); the first one reuses the hyper-gradient above
    M = {k: v.clone() for k, v in meta.items()}
    bufs = [None] * 4
    for s in (1, 2):
        if s > 1:
            hg, _, _ = MO.hypergrad_exact(f, p, M, bt, bv, gum, tau, tmin, hlr)
        grads, _ = MO.clip_grad_norm_([hg[k] for k in MO.META_NAMES], 10.0)
        new, bufs = MO.sgd_momentum_step([M[k] for k in MO.META_NAMES], grads, bufs, float(g["meta.meta_learning_rate"]), 0.9,
                                         float(g["meta.meta_weight_decay"]))
        M = dict(zip(MO.META_NAMES, new))
        for k in MO.META_NAMES:
            np.testing.assert_allclose(M[k].numpy(), g[f"outer.step{s}.{k}"], rtol=1e-5, atol=2e-7)


@pytest.mark.parametrize("forward_hvp", [False, True])
@pytest.mark.parametrize("rel_step", [3e-4, 5e-4])
def test_first_order_formulation_matches_exact(case, rel_step, forward_hvp):
    """the finite-difference form the GPU path uses reproduces the reference's double-backward hyper-gradient at d = 128"""
    g, p, meta, bt, bv, cfg = case
    gum, tau, tmin, hlr = scalars(g)
    f = MO.sasrec_losses(cfg)
    hg, _, _ = MO.hypergrad_fd(f, p, meta, bt, bv, gum, tau, tmin, hlr, rel_step=rel_step, forward_hvp=forward_hvp)
    ref = np.concatenate([g["outer.hypergrad." + k].ravel() for k in MO.META_NAMES])
    err = rel(np.concatenate([hg[k].numpy().ravel() for k in MO.META_NAMES]), ref)
    print("rel_step", rel_step, "forward_hvp", forward_hvp, "hypergrad rel err", err)
    assert err < 3e-4, err
