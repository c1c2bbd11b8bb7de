"""GPU tests of the GNN target model: dr4sr_gnn_propagate (csrc/gnn.hip) against a float64 restatement, its adjointness, the whole step
of dr4sr_amd.model.gnn.GNN against golden vectors made by RUNNING the reference (tools/make_gnn_golden.py), eval, the captured step,
determinism, fit + evaluate, and the unsupported combinations."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _gnn_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 50


def make_config(n_items=300, n_rows=300, batch=64, epochs=1, dropout=0.0, graph="old", hip_graph=True, deterministic=None, model="GNN"):
    cfg = {
        "data": {"dataset": "synthetic-toys", "domain_name_list": ["toy"], "max_seq_len": L, "dataset_class": "synthetic",
                 "train_file": "", "n_items": n_items, "n_rows": n_rows, "n_eval_rows": 128, "seed": 5, "markov": 0.9},
        "model": {"model": model, "embed_dim": 64, "loss_fn": "bce", "hidden_size": 128, "layer_num": 2, "head_num": 2,
                  "dropout_rate": dropout, "activation": "gelu", "layer_norm_eps": 1e-12, "graph": graph, "gnn_layer": 3, "window": 2},
        "train": {"batch_size": batch, "early_stop_mode": "max", "early_stop_patience": 20, "epochs": epochs, "device": "cuda",
                  "optimizer": "adam", "learning_rate": 0.001, "weight_decay": 0, "num_neg": 1, "seed": 2023, "hip_graph": hip_graph},
        "eval": {"batch_size": 128, "cutoff": [20, 10], "val_metrics": ["ndcg", "recall"], "test_metrics": ["ndcg", "recall"],
                 "topk": 100, "save_path": "./saved/"},
    }
    if deterministic is not None:
        cfg["train"]["deterministic"] = deterministic
    return cfg


def build(cfg, init=True):
    from dr4sr_amd.utils import prepare_datasets, prepare_model, seed_everything
    seed_everything(cfg["train"]["seed"])
    ds = prepare_datasets(cfg)
    model = prepare_model(cfg, ds)
    if init:
        model._init_model(ds[0])
    return ds, model


# ---------------------------------------------------------------------------------------------- 1. the propagation kernel
def crafted_rows(N, hub_deg, mid_deg=90):
    """item rows whose graph holds: PAD, an item in no sequence (N - 1: self loop only), a leaf with one neighbour (N - 2), item 2 with
    mid_deg + 1 non-zeros (two 64-edge batches), item 1 (the hub) with hub_deg + 1, and random rows around them"""
    rng = np.random.default_rng(N)
    pool = np.arange(3, N - 2)
    assert hub_deg <= len(pool) and mid_deg <= len(pool)
    rows = []

    def alternate(center, others):                      # [x0, c, x1, c, ...]: c neighbours every x (distance 1), x_i neighbours x_i+1 (distance 2)
        for i in range(0, len(others), L // 2):
            xs = others[i:i + L // 2]
            rows.append(np.stack([xs, np.full(len(xs), center)], 1).ravel().tolist())
    alternate(1, pool[:hub_deg])
    alternate(2, pool[len(pool) - mid_deg:])
    rows.append([int(pool[0]), N - 2])
    for _ in range(40):
        rows.append(rng.integers(3, N - 2, size=int(rng.integers(1, L + 1))).tolist())
    ids = torch.zeros(len(rows), L, dtype=torch.int64)
    for i, r in enumerate(rows):
        ids[i, :len(r)] = torch.tensor(r)
    return ids, torch.tensor([len(r) for r in rows])


@pytest.fixture(scope="module")
def graphs():
    """'small': N = 257, the longest row below the split threshold; 'hub': N raised just enough for a row above twice the threshold"""
    from dr4sr_amd import _lib
    from dr4sr_amd.model.gnn import build_graph
    split = int(_lib.load().dr4sr_gnn_split_rows())
    out = {}
    for name, N, hub_deg in (("small", 257, 200), ("hub", max(257, 2 * split + 8), 2 * split + 1)):
        ids, sl = crafted_rows(N, hub_deg)
        row_ptr, col, val = build_graph(ids.cuda(), sl.cuda(), N, 2, False)
        deg = (row_ptr[1:] - row_ptr[:-1]).cpu()
        assert int(deg[0]) == 1 and int(deg[N - 1]) == 1 and int(deg[N - 2]) == 2 and 65 <= int(deg[2]) <= 128
        assert int(deg[1]) == hub_deg + 1 and (int(deg[1]) > 2 * split if name == "hub" else int(deg.max()) <= split)
        A64 = R.csr_to_sparse(row_ptr, col, val, torch.float64).to_dense()
        out[name] = dict(N=N, csr=(row_ptr, col, val), A64=A64, A32=R.csr_to_sparse(row_ptr, col, val), ref={})
    return out


def hip_propagate(csr, N, D, n_hop, x, out, accumulate, ws=None):
    from dr4sr_amd import _lib
    lib = _lib.load()
    row_ptr, col, val = csr
    if ws is None:
        ws = torch.empty(int(lib.dr4sr_gnn_workspace_bytes(N, D, int(col.numel()))), dtype=torch.uint8, device="cuda")
    return lib.dr4sr_gnn_propagate(_lib.ptr(row_ptr), _lib.ptr(col), _lib.ptr(val), N, D, n_hop, _lib.ptr(x), _lib.ptr(out), accumulate,
                                   _lib.ptr(ws), ws.numel(), _lib.cur_stream())


@pytest.mark.parametrize("n_hop", [0, 1, 3])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("graph", ["small", "hub"])
def test_propagate_against_float64(graphs, graph, D, n_hop):
    """error of HIP against float64, relative to max-abs, at most twice the error of fp32 torch.sparse.mm on CPU against the same float64
    result (floor 1e-6); n_hop = 0 bit-exact; accumulate = 1 adds onto a non-zero out; `in` unchanged; two calls bitwise equal"""
    g = graphs[graph]
    N = g["N"]
    x = torch.randn(N, D, generator=torch.Generator().manual_seed(100 * D + n_hop))
    ref = R.propagate(g["A64"], x.double(), n_hop)
    scale = float(ref.abs().max())
    err_ref = float((R.propagate(g["A32"], x, n_hop).double() - ref).abs().max()) / scale
    tol = max(2.0 * err_ref, 1e-6)
    xd = x.cuda()
    out = torch.full((N, D), float("nan"), device="cuda")
    assert hip_propagate(g["csr"], N, D, n_hop, xd, out, 0) == 0
    err = float((out.cpu().double() - ref).abs().max()) / scale
    print(f"gnn propagate {graph} D={D} n_hop={n_hop}: hip err {err:.3e}, torch.sparse.mm fp32 err {err_ref:.3e}, tol {tol:.3e}")
    assert torch.equal(xd.cpu(), x)
    if n_hop == 0:
        assert torch.equal(out.cpu(), x)
    assert err <= tol
    out2 = torch.zeros(N, D, device="cuda")
    assert hip_propagate(g["csr"], N, D, n_hop, xd, out2, 0) == 0
    assert torch.equal(out, out2)
    base = torch.randn(N, D, generator=torch.Generator().manual_seed(7)).cuda()
    acc = base.clone()
    assert hip_propagate(g["csr"], N, D, n_hop, xd, acc, 1) == 0
    assert torch.equal(acc, base + out)


def test_propagate_argument_checks(graphs):
    g = graphs["small"]
    N = g["N"]
    x, out = torch.zeros(N, 64, device="cuda"), torch.zeros(N, 64, device="cuda")
    small_ws = torch.empty(1024, dtype=torch.uint8, device="cuda")
    assert hip_propagate(g["csr"], N, 96, 1, x, out, 0, ws=small_ws) == -2      # DR4SR_E_SHAPE
    assert hip_propagate(g["csr"], N, 64, 1, x, out, 0, ws=small_ws) == -3      # DR4SR_E_WS
    assert hip_propagate(g["csr"], N, 64, 1, x, x, 0) == -1              # in == out: DR4SR_E_ARG
    assert hip_propagate(g["csr"], N, 64, -1, x, out, 0) == -1 and hip_propagate(g["csr"], N, 64, 1, x, out, 2) == -1


@pytest.mark.parametrize("D", [64, 128])
def test_propagate_is_self_adjoint(graphs, D):
    """<u, P v> == <P u, v> to 1e-5 relative: the backward reuses the forward operator.  u, v are uniform on [0, 1): with every term of
    both dot products non-negative (A >= 0) the relative figure measures the operator, not a cancellation in the dot product"""
    g = graphs["hub"]
    N = g["N"]
    gen = torch.Generator().manual_seed(D)
    u, v = torch.rand(N, D, generator=gen).cuda(), torch.rand(N, D, generator=gen).cuda()
    Pu, Pv = torch.empty_like(u), torch.empty_like(v)
    assert hip_propagate(g["csr"], N, D, 3, u, Pu, 0) == 0 and hip_propagate(g["csr"], N, D, 3, v, Pv, 0) == 0
    a, b = float((u.double() * Pv.double()).sum()), float((Pu.double() * v.double()).sum())
    print(f"gnn adjointness D={D}: <u, Pv> = {a:.9e}, <Pu, v> = {b:.9e}, rel {abs(a - b) / max(abs(a), abs(b)):.3e}")
    assert abs(a - b) <= 1e-5 * max(abs(a), abs(b))
    # a signed pair (standard normal): the dot products cancel, so the figure is taken relative to sum |u| |P v|, the size of the terms
    u, v = torch.randn(N, D, generator=gen).cuda(), torch.randn(N, D, generator=gen).cuda()
    assert hip_propagate(g["csr"], N, D, 3, u, Pu, 0) == 0 and hip_propagate(g["csr"], N, D, 3, v, Pv, 0) == 0
    a, b = float((u.double() * Pv.double()).sum()), float((Pu.double() * v.double()).sum())
    size = float((u.double().abs() * Pv.double().abs()).sum())
    print(f"gnn adjointness D={D}, signed: <u, Pv> = {a:.9e}, <Pu, v> = {b:.9e}, sum |u||Pv| = {size:.3e}, rel {abs(a - b) / size:.3e}")
    assert abs(a - b) <= 1e-5 * size


@pytest.mark.parametrize("D", [64, 128])
def test_propagate_with_a_workspace_too_small_for_the_chunks(graphs, D):
    """a workspace that holds the tables but not the hub's chunks (sized for nnz = 0: room for one chunk, the hub has three): the hub row
    is summed whole by its row wave — same bound against float64 as the chunked form, two calls bitwise equal"""
    from dr4sr_amd import _lib
    g = graphs["hub"]
    N = g["N"]
    x = torch.randn(N, D, generator=torch.Generator().manual_seed(11 * D))
    ref = R.propagate(g["A64"], x.double(), 3)
    scale = float(ref.abs().max())
    tol = max(2.0 * float((R.propagate(g["A32"], x, 3).double() - ref).abs().max()) / scale, 1e-6)
    small = int(_lib.load().dr4sr_gnn_workspace_bytes(N, D, 0))
    assert small < int(_lib.load().dr4sr_gnn_workspace_bytes(N, D, int(g["csr"][1].numel())))
    outs = []
    for _ in range(2):
        ws = torch.empty(small, dtype=torch.uint8, device="cuda")
        out = torch.full((N, D), float("nan"), device="cuda")
        assert hip_propagate(g["csr"], N, D, 3, x.cuda(), out, 0, ws=ws) == 0
        outs.append(out)
    err = float((outs[0].cpu().double() - ref).abs().max()) / scale
    print(f"gnn propagate hub D={D}, workspace without room for the chunks: hip err {err:.3e}, tol {tol:.3e}")
    assert err <= tol and torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------- 3./4. the model against the golden
@pytest.fixture(scope="module")
def golden(golden_dir):
    return R.load_golden(golden_dir)


def golden_model(shared, mode):
    from dr4sr_amd.model.gnn import build_graph
    N = int(shared["meta.num_items"])
    ds, model = build(make_config(n_items=N, n_rows=64, batch=32, graph=mode))
    ids, sl, drop_last = R.golden_rows(shared, mode)
    graph = build_graph(ids.cuda(), sl.cuda(), N, int(shared["meta.window"]), drop_last)           # the builder on device tensors
    ref = R.coo_to_csr(shared[f"adj.{mode}.row"], shared[f"adj.{mode}.col"], shared[f"adj.{mode}.val"], N)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(graph, ref))
    model.set_graph(graph)
    sd = R.golden_params(shared)
    assert sorted(model.state_dict()) == sorted(str(k) for k in shared["meta.state_dict_keys"])
    model.load_state_dict(sd, strict=True)
    return model, sd


@pytest.mark.parametrize("mode", ["old", "new"])
def test_whole_step_against_the_reference(golden, mode):
    """loss (reduce True / False), query, G and every gradient within the project's parity gate (1e-3 relative); the
    parameters after one optimizer step within 1e-5"""
    shared, parts = golden
    g = parts[mode]
    model, _ = golden_model(shared, mode)
    names = [n for n, _ in model.named_parameters()]
    assert set(names) == {k[len("grad."):] for k in g if k.startswith("grad.")}                    # G is no parameter
    dev = model.device
    bd = {k: v.to(dev) for k, v in R.golden_batch(shared).items()}
    model.train()
    model.optimizer.zero_grad()
    loss, query = model.training_step(bd, reduce=True, return_query=True)
    loss.backward()
    live = (torch.arange(L, device=dev).view(1, -1) < bd["seqlen"].view(-1, 1)).unsqueeze(-1)
    figures = {"G": R.rel(model.engine.table.cpu(), g["out.G"]),
               "query": R.rel(torch.where(live, query.detach(), torch.zeros((), device=dev)).cpu(), g["out.query"]),
               "loss": abs(float(loss.detach()) - float(g["out.loss"])) / abs(float(g["out.loss"]))}
    with torch.no_grad():
        figures["loss_noreduce"] = R.rel(model.training_step(bd, reduce=False).cpu(), g["out.loss_noreduce"])
    for n, p in model.named_parameters():
        figures["grad." + n] = R.rel(p.grad.cpu(), g["grad." + n])
    model.optimizer.step()
    after = {n: float(np.abs(p.detach().cpu().numpy() - g["adam1." + n]).max()) for n, p in model.named_parameters()}
    print(f"gnn step {mode}: " + ", ".join(f"{k} {v:.2e}" for k, v in figures.items()))
    print(f"gnn step {mode} after Adam: " + ", ".join(f"{k} {v:.2e}" for k, v in after.items()))
    for k, v in figures.items():
        assert v < 1e-3, k
    for k, v in after.items():
        assert v < 1e-5, k


@pytest.mark.parametrize("mode", ["old", "new"])
def test_eval_topk_and_repropagation(golden, mode):
    shared, parts = golden
    g = parts[mode]
    model, _ = golden_model(shared, mode)
    dev = model.device
    vb = {k: v.to(dev) for k, v in R.golden_batch(shared, "eval.").items()}
    model.eval()
    model.set_eval_domain("toy")
    with torch.no_grad():
        score, items = model.topk(vb, 20, vb["user_hist"])
        q0 = model.forward(vb).clone()
    score, items = score.cpu().numpy(), items.cpu().numpy()
    ref_s, ref_i = g["eval.topk_score"], g["eval.topk_items"]
    assert float(np.abs(score - ref_s).max()) < 1e-4
    excused = 0
    for b, j in zip(*np.nonzero(items != ref_i)):                   # a tie: the item sits at a neighbouring rank whose golden score is within 1e-5
        where = np.nonzero(ref_i[b] == items[b, j])[0]
        assert len(where) == 1 and abs(float(ref_s[b, where[0]]) - float(ref_s[b, j])) < 1e-5, (b, j)
        excused += 1
    assert excused <= 0.01 * items.size
    assert R.rel(q0.cpu(), g["eval.query_last"]) < 1e-3
    # one optimizer step, then the next forward sees the G of the NEW E
    bd = {k: v.to(dev) for k, v in R.golden_batch(shared).items()}
    model.train()
    model.optimizer.zero_grad()
    model.training_step(bd).backward()
    model.optimizer.step()
    model.eval()
    with torch.no_grad():
        q1 = model.forward(vb)
    assert float((q1 - q0).abs().max()) > 1e-4
    A = R.csr_to_sparse(*model.query_encoder.norm_adj)
    G_now = R.propagate(A, model.item_embedding.weight.detach().cpu(), 3)
    assert R.rel(model.engine.table.cpu(), G_now) < 1e-5


# ---------------------------------------------------------------------------------------------- 5. - 8.
def test_captured_step_equals_eager_step():
    """4 API steps on a 300-row synthetic set with train.hip_graph on and off, equal seeds, dropout 0: the parameters agree to 1e-5;
    so does the reference-shaped loop body (training_step -> loss.backward() -> optimizer.step()) the direct step body stands for"""
    from dr4sr_amd.model.basemodel import BaseModel
    res = {}
    for form in ("eager", "captured", "autograd"):
        ds, model = build(make_config(hip_graph=form == "captured"))
        model.train()
        assert model._api_graph_ok() == (form == "captured") and not model._fast_path_ok()
        batches = [b for b, _ in zip(ds[0].get_loader(shuffle=False), range(4))]
        losses = []
        for b in batches:
            step = model._api_step_graph if form == "captured" else model._api_step_body if form == "eager" else \
                (lambda bb: BaseModel._api_step_body(model, bb))
            losses.append(float(step(b)))
        assert int(model.engine.inner.state[0]) == 4 and int(model.engine.raw_state[0]) == 4       # one step count
        res[form] = (losses, {n: p.detach().clone() for n, p in model.named_parameters()})
    for form in ("captured", "autograd"):
        worst = max(float((res["eager"][1][n] - res[form][1][n]).abs().max()) for n in res["eager"][1])
        print(f"gnn {form} vs eager after 4 steps: max parameter difference {worst:.3e}; losses {res[form][0]} vs {res['eager'][0]}")
        assert np.allclose(res[form][0], res["eager"][0], rtol=1e-5, atol=1e-6)
        assert worst < 1e-5, form


def test_deterministic_fits_are_bitwise_equal(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    sds = []
    for _ in range(2):
        ds, model = build(make_config(dropout=0.5, deterministic=True), init=False)
        model.fit()
        sds.append({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
    for k in sds[0]:
        assert torch.equal(sds[0][k], sds[1][k]), k


def test_fit_and_evaluate_end_to_end(tmp_path, monkeypatch):
    """quickstart.run for 2 epochs: finite loss, lower in epoch 2 than in epoch 1; metrics present; the checkpoint reloads"""
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("DR4SR_CONFIG_DIR", os.path.join(ROOT, "configs"))
    from dr4sr_amd import quickstart
    from dr4sr_amd.model.gnn import GNN
    seen = []
    real = GNN.training_epoch_end

    def spy(self, output_list):
        real(self, output_list)
        seen.append((self, float(self.logged_metrics["train_loss_0"])))
    monkeypatch.setattr(GNN, "training_epoch_end", spy)
    out = quickstart.run(make_config(epochs=2, dropout=0.5))
    losses = [l for _, l in seen]
    assert len(losses) == 2 and all(np.isfinite(losses)) and losses[1] < losses[0], losses
    assert {"ndcg@20", "recall@20"} <= set(out) and all(np.isfinite(v) for v in out.values())
    model = seen[0][0]
    path = os.path.join(model.config["eval"]["save_path"], model.ckpt_path)
    kept = {k: v.detach().clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        model.item_embedding.weight.add_(1.0)
    model.load_checkpoint(path)
    for k, v in model.state_dict().items():
        assert torch.equal(v, kept[k]), k


def test_unsupported_combinations_raise(monkeypatch):
    monkeypatch.setenv("DR4SR_CONFIG_DIR", os.path.join(ROOT, "configs"))
    from dr4sr_amd.utils import prepare_datasets, prepare_model
    cfg = make_config(n_rows=64)
    cfg["model"]["bidirectional"] = True
    ds = prepare_datasets(cfg)
    with pytest.raises(NotImplementedError, match="bidirectional"):
        prepare_model(cfg, ds)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="WORLD_SIZE"):
        prepare_model(make_config(n_rows=64), ds)
    monkeypatch.delenv("WORLD_SIZE")
    meta = make_config(n_rows=64, model="MetaModel")
    meta["model"].update({"sub_model": "GNN", "tau_min": 1})
    meta["train"].update({"interval": 2, "meta_optimizer": "sgd", "meta_learning_rate": 0.001, "hpo_learning_rate": 0.001,
                          "meta_weight_decay": 0.001, "descent_step": 30, "warmup_epoch": -1, "hypergrad_rel_step": 5e-4})
    mds = prepare_datasets(meta)
    mm = prepare_model(meta, mds)
    with pytest.raises(NotImplementedError, match="GNN"):
        mm._init_model(mds[0])
