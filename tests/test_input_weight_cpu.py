"""tests/_inw_ref.py (the CPU restatement of SASRec's encoder with batch['input_weight'], composed from oracle.sasrec_oracle) against
tests/golden/sasrec_input_weight.npz, which tools/make_input_weight_golden.py recorded by running the reference's own model/sasrec.py.
No GPU."""
import os

import numpy as np
import pytest
import torch

import _inw_ref as R

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-5            # the bar tests/_gnn_ref.py met against its golden


@pytest.fixture(scope="module")
def golden():
    return R.load_golden(GOLDEN_DIR)


@pytest.fixture(scope="module")
def step(golden):
    p, batch = R.golden_params(golden), R.golden_batch(golden)
    w = torch.from_numpy(golden["weight"])
    m = golden
    return R.step_grads(p, batch, w, int(m["meta.head_num"]), int(m["meta.layer_num"]), float(m["meta.layer_norm_eps"]))


def test_golden_holds_what_the_issue_asks(golden):
    b = R.golden_batch(golden)
    w = golden["weight"]
    B, L = b["in_item_id"].shape
    assert w.shape == (B, L, 1) and golden["grad_weight"].shape == (B, L, 1) and B == 8
    assert {1, 2, 47, 50} <= set(b["seqlen"].tolist())
    live = np.arange(L)[None, :] < b["seqlen"].numpy()[:, None]
    assert ((w[..., 0] == 0) & live).sum() == 2, "two valid entries of the weight are 0"
    assert any((w[r] == 1).all() for r in range(B)), "one row of the weight is all 1"
    assert w.min() >= 0 and w.max() <= 1.75
    pad_inside = (b["in_item_id"].numpy() == 0) & live
    assert pad_inside.sum() == 1 and not pad_inside[:, 0].any(), "one PAD id inside a valid range, not at position 0"
    assert os.path.getsize(os.path.join(GOLDEN_DIR, R.GOLDEN)) < (1 << 20)


def test_restatement_reproduces_reference_query_and_loss(golden, step):
    loss, q, _, _ = step
    print("query", R.rel(q, golden["out.query"]), "loss", abs(float(loss) - float(golden["out.loss"])))
    assert R.rel(q, golden["out.query"]) < TOL
    assert abs(float(loss) - float(golden["out.loss"])) < TOL * abs(float(golden["out.loss"]))


def test_restatement_reproduces_reference_gradients(golden, step):
    _, _, g, gw = step
    names = [k[len("grad."):] for k in golden if k.startswith("grad.")]
    assert len(names) >= 2 + 12 * int(golden["meta.layer_num"])
    for n in names:
        if n == R.TIED:
            continue
        e = R.rel(g[n], golden["grad." + n])
        print(n, e)
        assert e < TOL, (n, e)
    e = R.rel(gw, golden["grad_weight"])
    print("weight.grad", e)
    assert gw.shape == golden["grad_weight"].shape and e < TOL
    assert np.abs(golden["grad_weight"]).max() > 0


def test_reference_weight_grad_is_zero_past_seqlen(golden):
    """what lets the HIP backward write d_input_weight for pos < seqlen only, into a zero-filled buffer"""
    b = R.golden_batch(golden)
    L = b["in_item_id"].shape[1]
    dead = np.arange(L)[None, :] >= b["seqlen"].numpy()[:, None]
    assert dead.any()
    assert (golden["grad_weight"][..., 0][dead] == 0).all()


def test_weight_of_ones_is_the_plain_oracle(golden):
    """the restatement adds the scale and nothing else: weight None / all ones = oracle.sasrec_oracle.sasrec_encode"""
    from oracle import sasrec_oracle as O
    p, b, m = R.golden_params(golden), R.golden_batch(golden), golden
    H, NL, eps = int(m["meta.head_num"]), int(m["meta.layer_num"]), float(m["meta.layer_norm_eps"])
    ref = O.sasrec_encode(p, b["in_item_id"], b["seqlen"], H, NL, eps, "origin")
    assert torch.equal(R.encode(p, b["in_item_id"], b["seqlen"], None, H, NL, eps, "origin"), ref)
    assert torch.equal(R.encode(p, b["in_item_id"], b["seqlen"], torch.ones(1, 1, 1), H, NL, eps, "origin"), ref)
