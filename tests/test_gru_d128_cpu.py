"""GRU4Rec at embed_dim 128, the parts that need no GPU: parameter layout, the fixture's loader, the oracle against the reference's own
run (tests/golden/gru4rec_d128*.npz, tools/make_gru_d128_golden.py), and the config override."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import gru4rec_oracle as GO
from oracle import sasrec_oracle as O

import _gru_d128

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("N,H,nl", [(131, 128, 2), (20034, 256, 2), (200, 256, 1), (200, 128, 4)])
def test_param_layout_at_d128(N, H, nl):
    from dr4sr_amd import _lib
    from dr4sr_amd.gru_engine import gru_param_names, gru_param_shapes
    lib = _lib.load()
    names, shapes = gru_param_names(nl), gru_param_shapes(N, 128, H, nl)
    off = (C.c_int64 * (3 + 2 * 4))()
    n = lib.dr4sr_gru4rec_param_layout(N, 128, H, nl, off)
    assert n == sum(int(np.prod(s)) for s in shapes)
    o = 0
    for i, (nm, sh) in enumerate(zip(names, shapes)):
        assert off[i] == o, nm
        o += int(np.prod(sh))


def test_golden_loader_reassembles_the_parts():
    from dr4sr_amd.gru_engine import gru_param_names, gru_param_shapes
    g = _gru_d128.load()
    n_parts = int(g["meta.n_parts"])
    assert n_parts >= 2 and all(os.path.getsize(os.path.join(_gru_d128.GOLDEN, f"gru4rec_d128.part{i}.npz")) < (1 << 20)
                                for i in range(n_parts))
    N, H, nl = int(g["meta.num_items"]), int(g["meta.hidden_size"]), int(g["meta.layer_num"])
    assert int(g["meta.embed_dim"]) == 128 and H == 128
    for nm, sh in zip(gru_param_names(nl), gru_param_shapes(N, 128, H, nl)):
        for pre in ("param.", "grad.", "adam1."):
            assert tuple(g[pre + nm].shape) == tuple(sh), pre + nm
    assert tuple(g["param.query_encoder.0.1.weight"].shape) == (N, 128)          # the tied table under its second name
    assert g["batch.in_item_id"].shape == (10, 50) and g["out.query"].shape[-1] == 128


def test_oracle_reproduces_the_reference_at_d128():
    """the d64 bounds of tests/test_gru_oracle.py"""
    g = _gru_d128.load()
    p = {k[6:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param.")}
    b = {k[6:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("batch.")}
    nl = int(g["meta.layer_num"])
    loss, q, grads = GO.grads_of(p, b, nl)
    np.testing.assert_allclose(q.numpy(), g["out.query"], rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(float(loss), float(g["out.loss"]), rtol=2e-6)
    for k, gv in grads.items():
        ref = g["grad." + k]
        assert float(np.abs(gv.numpy() - ref).max()) < 3e-4 * max(1e-8, float(np.abs(ref).max())), k
    params = {k: v.clone() for k, v in p.items() if k != "query_encoder.0.1.weight"}
    m = {k: torch.zeros_like(v) for k, v in params.items()}
    v = {k: torch.zeros_like(x) for k, x in params.items()}
    new = O.adam_step(params, grads, m, v, 1, lr=float(g["meta.lr"]), wd=float(g["meta.weight_decay"]))
    for k in new:
        well = np.abs(g["grad." + k]) > 1e-4
        np.testing.assert_allclose(new[k].numpy()[well], g["adam1." + k][well], rtol=0, atol=5e-6)
    ql = GO.gru4rec_encode(p, torch.from_numpy(g["eval.in_item_id"]), torch.from_numpy(g["eval.seqlen"]), nl, "last")
    np.testing.assert_allclose(ql.numpy(), g["eval.query_last"], rtol=2e-4, atol=2e-6)


def test_load_config_embed_dim_override_for_gru4rec(monkeypatch):
    from dr4sr_amd.utils import load_config
    monkeypatch.setenv("DR4SR_CONFIG_DIR", os.path.join(ROOT, "configs"))
    monkeypatch.delenv("DR4SR_EMBED_DIM", raising=False)
    assert load_config({"model": "GRU4Rec", "dataset": "yelp"})["model"]["embed_dim"] == 64
    monkeypatch.setenv("DR4SR_EMBED_DIM", "128")
    cfg = load_config({"model": "GRU4Rec", "dataset": "yelp"})
    assert cfg["model"]["embed_dim"] == 128 and cfg["model"]["model"] == "GRU4Rec" and cfg["model"]["hidden_size"] == 256
