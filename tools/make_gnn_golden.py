#!/usr/bin/env python3
"""Generate the GNN golden vectors by RUNNING the reference's own model/gnn.py on CPU (tools/make_golden.py's stubs and dataset writer,
by import).  Like make_golden.py this only works where the reference checkout exists; only DATA is committed.

Data: a Zipf-shaped set — N = 300 items, 200 training rows, L = 50 — whose first 32 rows (the batch) contain a seqlen 1, 2, 47 and 50 row.
For model.graph 'old' (validation rows without their last item) and 'new' (training rows), gnn_layer 3, window 2, dropout 0:
  tests/golden/gnn_small.npz            what both modes share: every initial parameter (state-dict keys), the batch with its negatives, the
                                        16 validation rows, the rows of the training and validation splits (what the graphs are built
                                        from), the coalesced COO of norm_adj of both modes, hyper-parameters
  tests/golden/gnn_small.part_<mode>.npz  G, the query (padded positions zeroed), the loss with reduce True / False, every parameter
                                        gradient, the parameters after one Adam step, topk(16 validation rows, k = 20) ids and scores
(three files because one mode's gradients + stepped parameters + shared parameters alone pass the 1 MiB limit of a committed file).

Note on the reference: _build_graph_old (model/gnn.py:112-114) decrements the validation split's seqlen tensor IN PLACE when the dataset
lives on the CPU (`.cpu()` is then no copy); on a GPU it does not.  The GPU behaviour is the one pinned here: the lengths are restored
after the model is built.

Usage:  python tools/make_gnn_golden.py [--out tests/golden]
"""
import argparse
import os
import shutil
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402

N_ITEMS, N_ROWS, BATCH, N_EVAL, TOPK, SEED = 300, 200, 32, 16, 20, 43


class ZipfRng:
    """the one method make_golden.build_dataset calls, drawing item ids with probability ~ 1 / rank (ranks shuffled over the ids)"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.perm = None

    def integers(self, lo, hi, size):
        if self.perm is None:
            self.perm = self.rng.permutation(np.arange(lo, hi))
            p = 1.0 / np.arange(1, hi - lo + 1)
            self.p = p / p.sum()
        return self.perm[self.rng.choice(hi - lo, size=size, p=self.p)]


def seqlens():
    rng = np.random.default_rng(SEED + 9)
    head = [2, 47, 1, 50, 3, 5]
    rest = np.minimum(50, 2 + rng.exponential(11.0, size=N_ROWS - len(head)).astype(np.int64)).tolist()
    return head + rest


def run_mode(work, mode, shared):
    import torch
    from utils import load_config, setup_environment, prepare_datasets, prepare_model
    config = load_config({"model": "GNN", "dataset": "amazon-toys"})
    config["train"]["device"] = "cpu"
    config["train"]["batch_size"] = BATCH
    config["data"]["train_file"] = "_ori"
    config["model"].update({"dropout_rate": 0.0, "embed_dim": 64, "graph": mode, "gnn_layer": 3, "window": 2})
    setup_environment(config["train"])
    torch.manual_seed(SEED)
    ds = prepare_datasets(config)
    dom = ds[1].eval_domain
    keep_len = ds[1].data[dom][3].clone()
    model = prepare_model(config, ds)
    ds[1].data[dom][3].copy_(keep_len)                 # (see the module docstring)
    model._init_model(ds[0])
    g = torch.Generator().manual_seed(SEED + 1)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "item_embedding" in n or "item_encoder" in n:
                continue
            p.add_(0.05 * torch.randn(p.shape, generator=g))
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    adj = model.query_encoder.norm_adj.coalesce()
    shared[f"adj.{mode}.row"] = adj.indices()[0].numpy().astype(np.int32)
    shared[f"adj.{mode}.col"] = adj.indices()[1].numpy().astype(np.int32)
    shared[f"adj.{mode}.val"] = adj.values().numpy()
    assert adj.values().dtype == torch.float32
    batch = next(iter(ds[0].get_loader(batch_size=BATCH, shuffle=False)))
    model.train()
    torch.manual_seed(SEED + 2)
    batch["neg_item"] = model._neg_sampling(batch)
    if "meta.state_dict_keys" not in shared:
        for k, v in sd0.items():
            if k != "query_encoder.item_encoder.weight":            # the tied table, stored once
                shared["param." + k] = v.numpy()
        shared["meta.state_dict_keys"] = np.array(list(sd0))
        for k, v in batch.items():
            shared["batch." + k] = v.numpy()
        # the rows both graphs are built from: the training split ('new') and the validation split of the eval domain ('old')
        shared["rows.train.in_item_id"], shared["rows.train.seqlen"] = ds[0].data[1].numpy().astype(np.int16), ds[0].data[3].numpy().astype(np.int16)
        shared["rows.val.in_item_id"], shared["rows.val.seqlen"] = ds[1].data[dom][1].numpy().astype(np.int16), ds[1].data[dom][3].numpy().astype(np.int16)
    else:                                                            # same seeds: both modes start from the same parameters and batch
        for k, v in sd0.items():
            if k != "query_encoder.item_encoder.weight":
                assert np.array_equal(shared["param." + k], v.numpy()), k
        for k, v in batch.items():
            assert np.array_equal(shared["batch." + k], v.numpy()), k
    out = {}
    with torch.no_grad():
        out["out.G"] = model.query_encoder.get_gnn_embeddings().numpy().copy()
    model.optimizer.zero_grad()
    loss, query = model.training_step(batch, reduce=True, return_query=True)
    loss.backward()
    live = (torch.arange(query.shape[1]).view(1, -1) < batch["seqlen"].view(-1, 1)).unsqueeze(-1)
    out["out.query"] = torch.where(live, query.detach(), torch.zeros(())).numpy()
    out["out.loss"] = loss.detach().numpy()
    for n, p in model.named_parameters():
        out["grad." + n] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy().copy()
    with torch.no_grad():
        out["out.loss_noreduce"] = model.training_step(batch, reduce=False).numpy()
    model.optimizer.step()
    for n, p in model.named_parameters():
        out["adam1." + n] = p.detach().numpy().copy()
    # The Adam pin must be well conditioned.  The first step moves a parameter by lr * g / (|g| + eps), whose slope at a gradient below
    # eps = 1e-8 is lr / eps = 1e5: the reference's OWN fp32 rounding of such an element then moves its stepped value by more than any
    # useful bound (seed 41 left one table gradient of 4e-9 beside a largest of 0.13 in mode 'new': a FLOAT64 evaluation of the same step
    # missed the reference's stepped table by 2.1e-5, in mode 'old' by 5e-8).  So the reference's step is compared with a float64
    # evaluation of it (tests/_gnn_ref.py) and a seed on which the two differ by more than 5e-6 anywhere is refused: half of the 1e-5 the
    # GPU test allows, which leaves an fp32 implementation the same distance from the exact step as the reference takes itself.
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import _gnn_ref as R
    p64 = {k: v.double() for k, v in sd0.items()}
    b64 = {k: v for k, v in batch.items()}
    _, _, _, g64 = R.gnn_step(p64, model.query_encoder.norm_adj.coalesce().double(), b64, int(config["model"]["head_num"]),
                              int(config["model"]["layer_num"]), float(config["model"]["layer_norm_eps"]), 3, dtype=torch.float64)
    a64 = R.adam1(p64, g64, float(config["train"]["learning_rate"]), float(config["train"]["weight_decay"]))
    for n in a64:
        d = float((a64[n] - torch.from_numpy(out["adam1." + n]).double()).abs().max())
        assert d < 5e-6, f"{mode}/{n}: ill-conditioned Adam pin (the reference is {d:.1e} from a float64 evaluation of its own step); choose another SEED"
    model.load_state_dict(sd0)
    model.eval()
    ds[1].set_eval_domain(dom)
    model.set_eval_domain(dom)
    vb = next(iter(ds[1].get_loader(batch_size=N_EVAL)))
    with torch.no_grad():
        score, items = model.topk(vb, TOPK, vb["user_hist"])
        q_last = model.forward(vb)
    if "eval.in_item_id" not in shared:
        for kk, v in vb.items():
            shared["eval." + kk] = v.numpy()
    out["eval.topk_score"], out["eval.topk_items"], out["eval.query_last"] = score.numpy(), items.numpy(), q_last.numpy()
    if "meta.num_items" not in shared:
        mc, tc = config["model"], config["train"]
        shared["meta.num_items"], shared["meta.embed_dim"] = np.int64(model.num_items), np.int64(mc["embed_dim"])
        for k in ("head_num", "hidden_size", "layer_num", "gnn_layer", "window"):
            shared["meta." + k] = np.int64(mc[k])
        shared["meta.layer_norm_eps"] = np.float64(mc["layer_norm_eps"])
        shared["meta.lr"], shared["meta.weight_decay"] = np.float64(tc["learning_rate"]), np.float64(tc["weight_decay"])
        shared["meta.torch_version"] = np.array(torch.__version__)
    deg = np.bincount(shared[f"adj.{mode}.row"], minlength=N_ITEMS)
    print(f"gnn_small/{mode}: nnz {adj.values().numel()}, degree max {deg.max()} median {int(np.median(deg))}, loss {float(loss.detach()):.6f}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "tests", "golden"))
    out_dir = os.path.abspath(ap.parse_args().out)
    if not os.path.isdir(mg.REF):
        sys.exit("reference not present; golden vectors can only be regenerated where the reference checkout exists")
    mg._install_stubs()
    sys.path.insert(0, mg.REF)
    work = tempfile.mkdtemp(prefix="dr4sr_golden_")
    cwd = os.getcwd()
    try:
        os.symlink(os.path.join(mg.REF, "configs"), os.path.join(work, "configs"))
        sl = seqlens()
        assert len(sl) == N_ROWS and {2, 47} <= set(sl[:BATCH])
        mg.build_dataset(work, N_ITEMS, sl, ZipfRng(SEED))
        os.chdir(work)
        shared, parts = {}, {}
        for mode in ("old", "new"):
            parts[mode] = run_mode(work, mode, shared)
        os.chdir(cwd)
        os.makedirs(out_dir, exist_ok=True)
        for name, arrays in [("gnn_small", shared)] + [(f"gnn_small.part_{m}", a) for m, a in parts.items()]:
            path = os.path.join(out_dir, name + ".npz")
            np.savez_compressed(path, **arrays)
            print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")
            assert os.path.getsize(path) < (1 << 20), "a committed file must stay under 1 MiB"
    finally:
        os.chdir(cwd)
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
