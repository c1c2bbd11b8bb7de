"""GNN target model, the parts that need no GPU: the graph builder against the reference's norm_adj, the CPU restatement of the step
(tests/_gnn_ref.py, the GPU tests' yardstick) against the golden vectors made by running the reference, model / config resolution and
the library's new exports."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _gnn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return R.load_golden(golden_dir)


@pytest.mark.parametrize("mode", ["old", "new"])
def test_build_graph_equals_the_reference_adjacency(golden, mode):
    """identical index sets, values bitwise equal as fp32, symmetric, A[0, 0] == 2 (PAD holds only its self loop)"""
    from dr4sr_amd.model.gnn import build_graph
    shared, _ = golden
    N = int(shared["meta.num_items"])
    ids, sl, drop_last = R.golden_rows(shared, mode)
    row_ptr, col, val = build_graph(ids, sl, N, int(shared["meta.window"]), drop_last)
    assert row_ptr.dtype == torch.int64 and col.dtype == torch.int32 and val.dtype == torch.float32
    ref_ptr, ref_col, ref_val = R.coo_to_csr(shared[f"adj.{mode}.row"], shared[f"adj.{mode}.col"], shared[f"adj.{mode}.val"], N)
    assert torch.equal(row_ptr, ref_ptr) and torch.equal(col, ref_col)
    assert np.array_equal(val.numpy().view(np.uint32), ref_val.numpy().view(np.uint32))
    A = R.csr_to_sparse(row_ptr, col, val).to_dense()
    assert torch.equal(A, A.t())
    assert float(A[0, 0]) == 2.0 and int((A[0] != 0).sum()) == 1
    for r in range(N):                                   # every row's columns ascending: the order the kernel sums in
        c = col[int(row_ptr[r]):int(row_ptr[r + 1])]
        assert bool((c[1:] > c[:-1]).all())


@pytest.mark.parametrize("mode", ["old", "new"])
def test_restatement_equals_the_reference_step(golden, mode):
    """G, query, both losses, every gradient and the Adam step of the CPU restatement against the reference's, to 1e-5 relative to max-abs.
    The Adam step is taken from the REFERENCE's gradients: the first step moves a parameter by lr * g / (|g| + eps), whose slope at a
    gradient near eps = 1e-8 is lr / eps = 1e5, so fed with the restatement's own gradients (equal to 1e-7 of the largest) the comparison
    would measure that amplification at a handful of near-zero elements, not the step formula (tools/make_gnn_golden.py measures it on
    the fixture: the reference is up to 5e-6 from a float64 evaluation of its own step)"""
    shared, parts = golden
    g = parts[mode]
    N = int(shared["meta.num_items"])
    H, n_layer, eps, n_hop = (int(shared["meta.head_num"]), int(shared["meta.layer_num"]), float(shared["meta.layer_norm_eps"]),
                              int(shared["meta.gnn_layer"]))
    A = R.csr_to_sparse(*R.coo_to_csr(shared[f"adj.{mode}.row"], shared[f"adj.{mode}.col"], shared[f"adj.{mode}.val"], N))
    params, batch = R.golden_params(shared), R.golden_batch(shared)
    loss, q, G, grads = R.gnn_step(params, A, batch, H, n_layer, eps, n_hop)
    assert R.rel(G, g["out.G"]) < 1e-5
    live = (torch.arange(q.shape[1]).view(1, -1) < batch["seqlen"].view(-1, 1)).unsqueeze(-1)
    assert R.rel(torch.where(live, q, torch.zeros(())), g["out.query"]) < 1e-5
    assert abs(float(loss) - float(g["out.loss"])) < 1e-5 * abs(float(g["out.loss"]))
    loss_nr, _, _, _ = R.gnn_step(params, A, batch, H, n_layer, eps, n_hop, reduce=False)
    assert R.rel(loss_nr, g["out.loss_noreduce"]) < 1e-5
    for k, v in grads.items():
        assert R.rel(v, g["grad." + k]) < 1e-5, k
    after = R.adam1(params, {k: torch.from_numpy(g["grad." + k]) for k in grads}, float(shared["meta.lr"]), float(shared["meta.weight_decay"]))
    for k, v in after.items():
        assert R.rel(v, g["adam1." + k]) < 1e-5, k
    assert float(G[0].abs().max()) == 0.0               # PAD: E[0] = 0 and row 0 of A holds only the self loop


def test_model_class_and_config_resolve(monkeypatch):
    monkeypatch.setenv("DR4SR_CONFIG_DIR", os.path.join(ROOT, "configs"))
    from dr4sr_amd.utils.config import get_model_class, load_config
    cls = get_model_class("GNN")
    assert cls.__name__ == "GNN"
    config = load_config({"model": "GNN", "dataset": "amazon-toys"})
    mc = config["model"]
    assert (mc["hidden_size"], mc["layer_num"], mc["head_num"], mc["dropout_rate"], mc["activation"], mc["layer_norm_eps"], mc["graph"],
            mc["gnn_layer"], mc["window"]) == (128, 2, 2, 0.5, "gelu", 1e-12, "old", 3, 2)
    assert mc["model"] == "GNN" and "embed_dim" in mc and "batch_size" in config["train"]


def test_library_exports_the_propagation_entry_points():
    from dr4sr_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("dr4sr_gnn_split_rows", "dr4sr_gnn_workspace_bytes", "dr4sr_gnn_propagate"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    lib.dr4sr_abi_version.restype = C.c_int
    lib.dr4sr_sasrec_plan_sizeof.restype = C.c_int
    assert lib.dr4sr_abi_version() == 10 == _lib.ABI_VERSION
    assert lib.dr4sr_sasrec_plan_sizeof() == C.sizeof(_lib.SasrecPlan)
    # host-side argument checks (no device is touched before they return)
    lib.dr4sr_gnn_workspace_bytes.restype = C.c_int64
    lib.dr4sr_gnn_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int64]
    lib.dr4sr_gnn_split_rows.restype = C.c_int32
    assert lib.dr4sr_gnn_split_rows() >= 64
    assert lib.dr4sr_gnn_workspace_bytes(300, 64, 4418) > 3 * 300 * 64 * 4
    assert lib.dr4sr_gnn_workspace_bytes(300, 128, 4418) > lib.dr4sr_gnn_workspace_bytes(300, 64, 4418)
    assert lib.dr4sr_gnn_workspace_bytes(300, 96, 4418) == -2 and lib.dr4sr_gnn_workspace_bytes(0, 64, 10) == -1
