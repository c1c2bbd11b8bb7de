"""Evaluation by target rank on the MI355X (csrc/rank.hip): dr4sr_target_rank against the definition of the rank on exact integer
scores and against the top-k call on arbitrary floats, repeat / graph capture, dr4sr_rank_metrics_accumulate against
evaluation.rank_metrics in float64, the torch op, and eval.rank_eval at model level against the top-k evaluation.

Exactness is the method of tests/test_gpu_topk_exact.py (helpers restated here): q and E hold small integers stored in fp32, every dot
product is an integer far below 2^24 and therefore exact in fp32 in any summation order, so the reference — an int64 matmul on the CPU
plus the definition

    rank(b) = #{ valid j : s(b, j) > s(b, t_b), or s(b, j) == s(b, t_b) and j < t_b }        (NONE for a target that is not valid)

— is compared with torch.equal."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NONE = 2 ** 31 - 1
NAMES = ["ndcg", "recall", "precision", "map", "mrr", "hit", "f1"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dr4sr_amd import _lib
    _lib.load()
    assert _lib.RANK_NONE == NONE
    return torch.device("cuda")


# ------------------------------------------------------------------------------------------------ inputs (CPU, integers in fp32)
def make_tables(values, B, N, D, gen):
    """u8: uniform in [-8, 8].  neg: q = -(|q| + 1), E = |E| + 1 (every score negative).  tern: E in {-1, 0, 1}, row b of q has
    (1, 2, 3, D)[b % 4] entries of +-1: a row's scores take few values, tie groups of N / 3 at m = 1."""
    if values in ("u8", "neg"):
        q = torch.randint(-8, 9, (B, D), generator=gen)
        E = torch.randint(-8, 9, (N, D), generator=gen)
        if values == "neg":
            q, E = -(q.abs() + 1), E.abs() + 1
    else:
        E = torch.randint(-1, 2, (N, D), generator=gen)
        q = torch.zeros(B, D, dtype=torch.int64)
        for b in range(B):
            m = (1, 2, 3, D)[b % 4]
            cols = torch.randperm(D, generator=gen)[:m]
            q[b, cols] = torch.randint(0, 2, (m,), generator=gen) * 2 - 1
    return q, E


def best_two(s):
    v = s.double().clone()
    v[:, 0] = float("-inf")
    return v.topk(min(2, s.shape[1] - 1), dim=1)[1]


def make_targets(B, N, blocked, gen):
    """random items, then per row class: 0 (PAD), N, 2^32 + 1 (out of range), a blocked item"""
    t = torch.randint(1, N, (B,), generator=gen)
    rows = torch.arange(B)
    t[rows % 7 == 3] = 0
    t[rows % 7 == 4] = N
    t[rows % 7 == 6] = 2 ** 32 + 1
    if blocked is not None and bool(blocked[1:].any()):
        t[rows % 7 == 5] = int(blocked[1:].nonzero()[0]) + 1
    return t


def make_hist(s, target, Lh, gen):
    """everything a history may hold: the row's best item (it must not be counted), the same id again, PAD, words that name no item
    (-1, N, N + 7, 2^31 + 3, 2^32 + the row's second-best item: that one must still be counted), random ids; the row's own target in
    rows b % 4 == 1 (as the best item) and b % 4 == 2 (in the LAST word) -> NONE"""
    B, N = s.shape
    assert Lh >= 8
    top = best_two(s)
    hist = torch.randint(0, N, (B, Lh), generator=gen)
    hist[:, 0] = top[:, 0]
    hist[:, 1] = top[:, 0]
    hist[:, 2] = 0
    hist[:, 3] = -1
    hist[:, 4] = N
    hist[:, 5] = N + 7
    hist[:, 6] = 2 ** 31 + 3
    hist[:, 7] = 2 ** 32 + top[:, -1]
    target = target.clone()
    rows = torch.arange(B)
    own = rows % 4 == 1
    target[own] = top[own, 0]
    last = (rows % 4 == 2) & (target >= 1) & (target < N)
    hist[last, Lh - 1] = target[last]
    return hist, target


def hist_mask(hist, B, N):
    m = torch.zeros(B, N, dtype=torch.bool)
    if hist is not None:
        ok = (hist >= 0) & (hist < N)
        rows = torch.arange(B).view(-1, 1).expand_as(hist)
        m[rows[ok], hist[ok]] = True
    return m


def valid_items(B, N, hist, blocked):
    v = torch.ones(B, N, dtype=torch.bool)
    v[:, 0] = False
    if blocked is not None:
        v[:, blocked.bool()] = False
    return v & ~hist_mask(hist, B, N)


def reference_rank(s, target, hist, blocked):
    """the definition, on exact (int64 or float64) scores s [B, N]"""
    B, N = s.shape
    valid = valid_items(B, N, hist, blocked)
    rows = torch.arange(B)
    tc = target.clamp(0, N - 1)
    t_valid = (target >= 1) & (target < N) & valid[rows, tc]
    st = s[rows, tc].view(B, 1)
    before = valid & ((s > st) | ((s == st) & (torch.arange(N).view(1, N) < tc.view(B, 1))))
    rank = before.sum(1).to(torch.int32)
    rank[~t_valid] = NONE
    return rank


# ------------------------------------------------------------------------------------------------ the calls
def call_rank(q, E, target, hist, blocked, out=None):
    from dr4sr_amd import _lib
    lib = _lib.load()
    B, D = q.shape
    nb = int(lib.dr4sr_target_rank_workspace_bytes(B))
    assert nb >= 0
    ws = torch.empty(max(nb // 4, 1), dtype=torch.int32, device=q.device)
    rank = torch.full((B,), -5, dtype=torch.int32, device=q.device) if out is None else out
    _lib.check(lib.dr4sr_target_rank(_lib.ptr(q), _lib.ptr(E), _lib.ptr(target), _lib.ptr(hist), _lib.ptr(blocked), _lib.ptr(rank), B, D,
                                     E.shape[0], 0 if hist is None else hist.shape[1], _lib.ptr(ws), nb, _lib.cur_stream()), "target_rank")
    return rank


def call_topk(q, E, hist, blocked, k):
    """dr4sr_full_score_topk_masked_ws in the two-kernel form (scores from the MFMA GEMM k_score_gemm)"""
    from dr4sr_amd import _lib
    lib = _lib.load()
    B, D = q.shape
    N = E.shape[0]
    Lh = 0 if hist is None else hist.shape[1]
    nb = int(lib.dr4sr_full_score_topk_workspace_bytes(B, N))
    form = int(lib.dr4sr_full_score_topk_form(B, D, N, Lh, k, nb))
    assert form in (0, 2), "the call must be the two-kernel form scored by the MFMA GEMM, not %d" % form
    ws = torch.empty(nb // 4, dtype=torch.float32, device=q.device)
    sc = torch.full((B, k), float("nan"), device=q.device)
    it = torch.full((B, k), -5, dtype=torch.int64, device=q.device)
    _lib.check(lib.dr4sr_full_score_topk_masked_ws(_lib.ptr(q), _lib.ptr(E), _lib.ptr(hist), _lib.ptr(blocked), _lib.ptr(sc), _lib.ptr(it),
                                                   B, D, N, Lh, k, _lib.ptr(ws), nb, _lib.cur_stream()), "topk_masked_ws")
    return sc.cpu(), it.cpu()


def assert_agrees_with_topk(rank, target, sc, it, k, what):
    """rank < k: the top-k call returns the target at position rank; otherwise the target is at no finite-score position"""
    B = rank.numel()
    rows = torch.arange(B)
    inside = rank < k
    at = it[rows, rank.long().clamp(max=k - 1)]
    bad = inside & ((at != target) | ~torch.isfinite(sc[rows, rank.long().clamp(max=k - 1)]))
    assert not bool(bad.any()), "%s: rows %s: rank %s but the top-k has %s there, target %s" % (
        what, bad.nonzero().flatten()[:4].tolist(), rank[bad][:4].tolist(), at[bad][:4].tolist(), target[bad][:4].tolist())
    listed = ((it == target.view(B, 1)) & torch.isfinite(sc)).any(1)
    bad = ~inside & listed
    assert not bool(bad.any()), "%s: rows %s have rank %s >= k but the top-k lists the target" % (
        what, bad.nonzero().flatten()[:4].tolist(), rank[bad][:4].tolist())


# ------------------------------------------------------------------------------------------------ exact rank
# N: 2 (one item), 63 / 64 / 65 (the 64-item tile edge), 513 (the 512-item chunk edge: a last chunk with a single tile), 1100 (three chunks)
@pytest.mark.parametrize("N", [2, 63, 64, 65, 513, 1100])
@pytest.mark.parametrize("values", ["u8", "neg", "tern"])
@pytest.mark.parametrize("D", [64, 128])
def test_rank_exact(dev, monkeypatch, D, values, N):
    monkeypatch.delenv("DR4SR_TOPK_FUSED", raising=False)
    k = 100
    for B in (1, 65, 130):
        gen = torch.Generator().manual_seed(100000 * D + 100 * N + B + len(values))
        q, E = make_tables(values, B, N, D, gen)
        s = q.long() @ E.long().T
        half = (torch.rand(N, generator=gen) < 0.5).to(torch.uint8)
        qd, Ed = q.float().to(dev), E.float().to(dev)
        none_seen = 0
        for Lh in (0, 8, 50):
            for bname, blocked in (("null", None), ("zeros", torch.zeros(N, dtype=torch.uint8)), ("half", half)):
                target = make_targets(B, N, blocked, gen)
                hist = None
                if Lh:
                    hist, target = make_hist(s, target, Lh, gen)
                what = "D=%d %s N=%d B=%d Lh=%d blocked=%s" % (D, values, N, B, Lh, bname)
                td = target.to(dev)
                hd = None if hist is None else hist.to(dev)
                bd = None if blocked is None else blocked.to(dev)
                got = call_rank(qd, Ed, td, hd, bd).cpu()
                ref = reference_rank(s, target, hist, None if bname == "zeros" else blocked)
                assert torch.equal(got, ref), "%s: rows %s: got %s, reference %s" % (
                    what, (got != ref).nonzero().flatten()[:6].tolist(), got[got != ref][:6].tolist(), ref[got != ref][:6].tolist())
                if bname == "zeros":                       # a mask of zeros is no mask
                    assert torch.equal(call_rank(qd, Ed, td, hd, None).cpu(), got), what
                none_seen += int((ref == NONE).sum())
                if Lh == 8 and bname != "zeros":
                    sc, it = call_topk(qd, Ed, hd, bd, k)
                    assert_agrees_with_topk(got, target, sc, it, k, what)
        assert B == 1 or none_seen > 0


# ------------------------------------------------------------------------------------------------ arbitrary floats: agreement with the top-k
@pytest.mark.parametrize("D", [64, 128])
def test_rank_agrees_with_topk_on_floats(dev, monkeypatch, D):
    """randn tables: no exact reference exists, but the target's score comes from the same MFMA loop as its column of the score
    matrix, so the rank and the top-k list must agree exactly; the rank itself is checked against float64 scores up to near-ties"""
    monkeypatch.delenv("DR4SR_TOPK_FUSED", raising=False)
    B, N, k, Lh = 130, 1100, 100, 50
    gen = torch.Generator().manual_seed(7 + D)
    q, E = torch.randn(B, D, generator=gen), torch.randn(N, D, generator=gen)
    s64 = q.double() @ E.double().T
    half = (torch.rand(N, generator=gen) < 0.5).to(torch.uint8)
    for blocked in (None, half):
        target = make_targets(B, N, blocked, gen)
        hist, target = make_hist(s64, target, Lh, gen)
        qd, Ed, td, hd = q.to(dev), E.to(dev), target.to(dev), hist.to(dev)
        bd = None if blocked is None else blocked.to(dev)
        got = call_rank(qd, Ed, td, hd, bd).cpu()
        sc, it = call_topk(qd, Ed, hd, bd, k)
        assert_agrees_with_topk(got, target, sc, it, k, "randn D=%d blocked=%s" % (D, blocked is not None))
        ref = reference_rank(s64, target, hist, blocked)
        assert torch.equal(got == NONE, ref == NONE)
        # fp32 scores may swap the target with items whose float64 score is within the fp32 error of the target's
        margin = 2.0 * float(((q @ E.T).double() - s64).abs().max())
        rows = torch.arange(B)
        st = s64[rows, target.clamp(0, N - 1)].view(B, 1)
        near = (valid_items(B, N, hist, blocked) & ((s64 - st).abs() <= margin)).sum(1)
        ok = (ref == NONE) | ((got.long() - ref.long()).abs() <= near)
        assert bool(ok.all()), (got[~ok][:4].tolist(), ref[~ok][:4].tolist())
        assert int(((got < k) & (got != NONE)).sum()) > 0 and int((got >= k).sum()) > 0


# ------------------------------------------------------------------------------------------------ repeat, capture, errors
@pytest.mark.parametrize("D", [64, 128])
def test_rank_repeats_bitwise_and_replays_from_a_graph(dev, D):
    B, N, Lh = 130, 1100, 50
    gen = torch.Generator().manual_seed(11 + D)
    q, E = torch.randn(B, D, generator=gen).to(dev), torch.randn(N, D, generator=gen).to(dev)
    target = torch.randint(1, N, (B,), generator=gen).to(dev)
    hist = torch.randint(0, N, (B, Lh), generator=gen).to(dev)
    a = call_rank(q, E, target, hist, None)
    b = call_rank(q, E, target, hist, None)
    assert torch.equal(a, b)
    from dr4sr_amd import _lib
    lib = _lib.load()
    nb = int(lib.dr4sr_target_rank_workspace_bytes(B))
    ws = torch.empty(nb // 4, dtype=torch.int32, device=dev)
    out = torch.full((B,), -5, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = lib.dr4sr_target_rank(_lib.ptr(q), _lib.ptr(E), _lib.ptr(target), _lib.ptr(hist), None, _lib.ptr(out), B, D, N, Lh,
                                   _lib.ptr(ws), nb, _lib.cur_stream())
    assert rc == 0
    for _ in range(2):
        out.fill_(-5)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, a)


def test_rank_argument_errors(dev):
    from dr4sr_amd import _lib
    lib = _lib.load()
    B, D, N = 4, 64, 100
    q, E = torch.zeros(B, D, device=dev), torch.zeros(N, D, device=dev)
    t = torch.ones(B, dtype=torch.int64, device=dev)
    out = torch.zeros(B, dtype=torch.int32, device=dev)
    nb = int(lib.dr4sr_target_rank_workspace_bytes(B))
    ws = torch.empty(nb // 4, dtype=torch.int32, device=dev)

    def call(B=B, D=D, N=N, Lh=0, ws=ws, nb=nb):
        return lib.dr4sr_target_rank(_lib.ptr(q), _lib.ptr(E), _lib.ptr(t), None, None, _lib.ptr(out), B, D, N, Lh, _lib.ptr(ws), nb,
                                     _lib.cur_stream())
    assert call() == 0 and call(B=0) == 0
    assert call(D=96) == -2 and call(B=-1) == -1 and call(N=1) == -1 and call(Lh=-1) == -1
    assert call(Lh=3) == -1                                # a history width without a history
    assert call(nb=B * 8 - 1) == -3 and call(ws=None) == -3
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.zeros(B, dtype=torch.int32))      # all-zero scores: nothing precedes item 1


# ------------------------------------------------------------------------------------------------ the accumulator
def test_metrics_accumulate_against_float64(dev):
    from dr4sr_amd import _lib, evaluation
    lib = _lib.load()
    topk, cutoffs = 100, [1, 10, 20]
    gen = torch.Generator().manual_seed(3)
    fixed = [0, 1, 9, 10, 11, 19, 20, 21, 99, 100, 5000, NONE, NONE]
    rank = torch.cat([torch.tensor(fixed), torch.randint(0, 40, (135 - len(fixed),), generator=gen)]).to(torch.int32)
    rank = rank[torch.randperm(135, generator=gen)]
    label = torch.ones(135)
    cuts = (C.c_int32 * 3)(*cutoffs)

    def run():
        acc = torch.zeros(1 + 7 * 3, dtype=torch.float64, device=dev)
        for lo, hi in ((0, 64), (64, 128), (128, 135)):    # three batches, the last ragged
            r, l = rank[lo:hi].contiguous().to(dev), label[lo:hi].contiguous().to(dev)
            _lib.check(lib.dr4sr_rank_metrics_accumulate(_lib.ptr(r), _lib.ptr(l), hi - lo, cuts, 3, topk, _lib.ptr(acc),
                                                         _lib.cur_stream()), "accumulate")
        return acc.cpu()
    a, b = run(), run()
    assert torch.equal(a, b), "the accumulator must be bitwise reproducible"
    assert float(a[0]) == 135.0
    ref = evaluation.rank_metrics(rank, label, NAMES, cutoffs, topk, dtype=torch.float64)
    for ci, c in enumerate(cutoffs):
        for si, n in enumerate(_lib.RANK_METRICS):
            got, want = float(a[1 + 7 * ci + si]) / 135.0, float(ref[f"{n}@{c}"])
            print(f"{n}@{c}: device {got!r} float64 {want!r}")
            assert abs(got - want) <= 1e-12 * abs(want), (n, c, got, want)
    acc = torch.zeros(22, dtype=torch.float64, device=dev)
    r, l = rank.to(dev), label.to(dev)
    bad = (C.c_int32 * 3)(1, 10, 101)
    assert lib.dr4sr_rank_metrics_accumulate(_lib.ptr(r), _lib.ptr(l), 135, bad, 3, topk, _lib.ptr(acc), _lib.cur_stream()) == -1
    bad = (C.c_int32 * 3)(0, 10, 20)
    assert lib.dr4sr_rank_metrics_accumulate(_lib.ptr(r), _lib.ptr(l), 135, bad, 3, topk, _lib.ptr(acc), _lib.cur_stream()) == -1
    torch.cuda.synchronize()
    assert float(acc.abs().sum()) == 0.0                   # a refused call launches nothing


# ------------------------------------------------------------------------------------------------ the torch op
@pytest.mark.parametrize("D", [64, 128])
def test_rank_through_the_torch_op(dev, D):
    import dr4sr_amd.ops  # noqa: F401  (registers the ops)
    B, N, Lh = 65, 513, 8
    gen = torch.Generator().manual_seed(5 + D)
    q, E = make_tables("u8", B, N, D, gen)
    s = q.long() @ E.long().T
    half = (torch.rand(N, generator=gen) < 0.5).to(torch.uint8)
    hist, target = make_hist(s, make_targets(B, N, half, gen), Lh, gen)
    qd, Ed, td, hd, bd = q.float().to(dev), E.float().to(dev), target.to(dev), hist.to(dev), half.to(dev)
    for h, bl in ((hd, bd), (None, None), (hd, None)):
        got = torch.ops.dr4sr_hip.target_rank(qd, Ed, td, h, bl)
        assert got.dtype == torch.int32 and torch.equal(got, call_rank(qd, Ed, td, h, bl))
    assert torch.equal(torch.ops.dr4sr_hip.target_rank(qd, Ed, td, hd, bd).cpu(), reference_rank(s, target, hist, half))


# ------------------------------------------------------------------------------------------------ model level
def make_config(model="SASRec", epochs=2, rank_eval=None, topk=100):
    cfg = {
        "data": {"dataset": "synthetic-toys", "domain_name_list": ["toy"], "max_seq_len": 50, "dataset_class": "synthetic",
                 "train_file": "", "n_items": 300, "n_rows": 600, "n_eval_rows": 128, "seed": 5},
        "model": {"model": model, "embed_dim": 64, "loss_fn": "bce", "hidden_size": 128, "layer_num": 2, "head_num": 2,
                  "dropout_rate": 0.0, "activation": "gelu", "layer_norm_eps": 1e-12},
        "train": {"batch_size": 64, "early_stop_mode": "max", "early_stop_patience": 20, "epochs": epochs, "device": "cuda",
                  "optimizer": "adam", "learning_rate": 0.001, "weight_decay": 0, "num_neg": 1, "seed": 2023, "hip_graph": True},
        "eval": {"batch_size": 48, "cutoff": [20, 10], "val_metrics": ["ndcg", "recall"], "test_metrics": ["ndcg", "recall"],
                 "topk": topk, "save_path": "./saved/"},
    }
    if model == "GNN":
        cfg["data"]["markov"] = 0.9
        cfg["model"].update({"graph": "old", "gnn_layer": 3, "window": 2})
    if rank_eval is not None:
        cfg["eval"]["rank_eval"] = rank_eval
    return cfg


def build(cfg):
    from dr4sr_amd.utils import prepare_datasets, prepare_model, seed_everything
    seed_everything(cfg["train"]["seed"])
    ds = prepare_datasets(cfg)
    return ds, prepare_model(cfg, ds)


def evaluate_checkpoint(model, rank_eval):
    """BaseModel.evaluate()'s loop on the fitted checkpoint with the seven metrics, the rank path off or on"""
    model.load_checkpoint(os.path.join(model.config["eval"]["save_path"], model.ckpt_path))
    model.eval()
    model.config["eval"]["test_metrics"] = list(NAMES)
    model.config["eval"]["rank_eval"] = rank_eval
    test_data = model.dataset_list[-1]
    out = {}
    for domain in model.domain_name_list:
        test_data.set_eval_domain(domain)
        model.set_eval_domain(domain)
        out.update(model.test_epoch_end(model.test_epoch(test_data.get_loader()), domain))
    return out


def assert_same_metrics(off, on):
    assert list(off) == list(on) and set(off) == {f"toy_{n}@{c}" for n in NAMES for c in (20, 10)}
    for k in off:
        print(f"{k}: top-k path {off[k]!r} rank path {on[k]!r}")
        assert abs(on[k] - off[k]) <= 2e-6 * abs(off[k]) + 1e-9, (k, off[k], on[k])
    assert off["toy_hit@20"] > 0 and off["toy_hit@20"] < 1      # the comparison sees hits and misses


def test_model_rank_eval_equals_topk_eval_sasrec(tmp_path, monkeypatch):
    """fit() validates through the rank path (early stopping sees ndcg@20); the checkpoint evaluated both ways logs the same names and
    values: the top-k path is an fp32 pairwise mean of fp32 per-row values, batch-weighted (~7e-7 worst case), the rank path fp64"""
    monkeypatch.chdir(tmp_path)
    _, model = build(make_config("SASRec", epochs=2, rank_eval=True))
    model.fit()
    assert "ndcg@20" in model.logged_metrics and "toy_recall@20" in model.logged_metrics
    assert np.isfinite(model.logged_metrics["ndcg@20"])
    ckpt = torch.load(os.path.join(model.config["eval"]["save_path"], model.ckpt_path), weights_only=False)
    assert "ndcg@20" in ckpt["metric"] and ckpt["config"]["eval"]["rank_eval"] is True
    off = evaluate_checkpoint(model, False)
    on = evaluate_checkpoint(model, True)
    assert_same_metrics(off, on)


def test_model_rank_eval_equals_topk_eval_gnn(tmp_path, monkeypatch):
    """GNN encodes on the propagated table G but scores on the raw table E: the rank path must do the same"""
    monkeypatch.chdir(tmp_path)
    _, model = build(make_config("GNN", epochs=1))
    model.fit()
    off = evaluate_checkpoint(model, False)
    on = evaluate_checkpoint(model, True)
    assert_same_metrics(off, on)


def test_model_rank_eval_refuses_a_cutoff_above_topk(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    ds, model = build(make_config("SASRec", rank_eval=True, topk=15))
    model._init_model(ds[0])
    model.eval()
    ds[1].set_eval_domain("toy")
    model.set_eval_domain("toy")
    with pytest.raises(ValueError, match=r"20.*15"):
        model.validation_epoch(0, ds[1].get_loader())
    model.config["eval"]["rank_eval"] = False
    assert len(model.validation_epoch(0, ds[1].get_loader())) >= 1        # the top-k path takes the config as before
