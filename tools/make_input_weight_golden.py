#!/usr/bin/env python3
"""Generate the input_weight golden vectors by RUNNING the reference's own model/sasrec.py on CPU with batch['input_weight'] set
(model/sasrec.py:61-64; tools/make_golden.py's stubs and dataset writer, by import).  Like make_golden.py this only works where the
reference checkout exists; only DATA is committed.

Data: N = 120 items, B = 8 rows (one batch) of seqlen 1, 2, 47, 50, 3, 7, 12, 20, L = 50, embed_dim 64, dropout 0.  One PAD id 0 is put
INSIDE a valid range (row 6, position 4: a masked key, an input row that takes no table gradient).
Weight: input_weight = U[0.25, 1.75] of shape [B, L, 1] with requires_grad; two valid entries are 0 and one row is all 1.
  tests/golden/sasrec_input_weight.npz   param.* (state-dict keys, the tied table once), batch.* (with its negatives), weight,
                                         out.query (origin pooling), out.loss (training_step, reduce=True), grad.* of every parameter,
                                         grad_weight (= weight.grad, [B, L, 1]), meta.*

Usage:  python tools/make_input_weight_golden.py [--out tests/golden]
"""
import argparse
import os
import shutil
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402

N_ITEMS, SEED = 120, 47
SEQLENS = [1, 2, 47, 50, 3, 7, 12, 20]
PAD_AT = (6, 4)                    # (row, position) of the PAD id inside a valid range
ZERO_AT = ((2, 5), (3, 49))        # valid entries of the weight set to 0
ONES_ROW = 5


def make_weight(B, L):
    import torch
    g = torch.Generator().manual_seed(SEED + 3)
    w = 0.25 + 1.5 * torch.rand(B, L, 1, generator=g)
    for b, l in ZERO_AT:
        w[b, l, 0] = 0.0
    w[ONES_ROW] = 1.0
    return w


def run(work):
    import torch
    from utils import load_config, setup_environment, prepare_datasets, prepare_model
    config = load_config({"model": "SASRec", "dataset": "amazon-toys"})
    config["train"]["device"] = "cpu"
    config["train"]["batch_size"] = len(SEQLENS)
    config["data"]["train_file"] = "_ori"
    config["model"].update({"dropout_rate": 0.0, "embed_dim": 64})
    setup_environment(config["train"])
    torch.manual_seed(SEED)
    ds = prepare_datasets(config)
    model = prepare_model(config, ds)
    model._init_model(ds[0])
    g = torch.Generator().manual_seed(SEED + 1)
    with torch.no_grad():                       # the reference zero-inits biases: perturb so that every path is pinned
        for n, p in model.named_parameters():
            if "item_embedding" in n or "item_encoder" in n:
                continue
            p.add_(0.05 * torch.randn(p.shape, generator=g))
    out = {}
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for k, v in sd0.items():
        if k != "query_encoder.item_encoder.weight":            # the tied table, stored once
            out["param." + k] = v.numpy()
    out["meta.state_dict_keys"] = np.array(list(sd0))
    batch = next(iter(ds[0].get_loader(batch_size=len(SEQLENS), shuffle=False)))
    assert batch["seqlen"].tolist() == SEQLENS
    batch["in_item_id"][PAD_AT] = 0
    model.train()
    torch.manual_seed(SEED + 2)
    batch["neg_item"] = model._neg_sampling(batch)
    for k, v in batch.items():
        out["batch." + k] = v.numpy()
    B, L = batch["in_item_id"].shape
    w = make_weight(B, L).requires_grad_(True)
    out["weight"] = w.detach().numpy().copy()
    batch["input_weight"] = w
    model.optimizer.zero_grad()
    loss, query = model.training_step(batch, reduce=True, return_query=True)
    loss.backward()
    live = (torch.arange(L).view(1, -1) < batch["seqlen"].view(-1, 1)).unsqueeze(-1)
    out["out.query"] = torch.where(live, query.detach(), torch.zeros(())).numpy()
    out["out.loss"] = loss.detach().numpy()
    for n, p in model.named_parameters():
        out["grad." + n] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy().copy()
    assert w.grad is not None and w.grad.shape == w.shape
    out["grad_weight"] = w.grad.numpy().copy()
    # the weight really entered the step: the same batch without it gives another loss
    del batch["input_weight"]
    with torch.no_grad():
        loss0 = model.training_step(batch, reduce=True)
    assert abs(float(loss0) - float(loss.detach())) > 1e-4, "input_weight did not reach the reference's encoder"
    mc = config["model"]
    out["meta.num_items"], out["meta.embed_dim"] = np.int64(model.num_items), np.int64(mc["embed_dim"])
    for k in ("head_num", "hidden_size", "layer_num"):
        out["meta." + k] = np.int64(mc[k])
    out["meta.layer_norm_eps"] = np.float64(mc["layer_norm_eps"])
    out["meta.torch_version"] = np.array(torch.__version__)
    print(f"sasrec_input_weight: loss {float(loss.detach()):.6f} (unweighted {float(loss0):.6f}), |weight.grad| max {float(w.grad.abs().max()):.3e}")
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
        mg.build_dataset(work, N_ITEMS, SEQLENS, np.random.default_rng(SEED))
        os.chdir(work)
        arrays = run(work)
        os.chdir(cwd)
        os.makedirs(out_dir, exist_ok=True)
        path = os.path.join(out_dir, "sasrec_input_weight.npz")
        np.savez_compressed(path, **arrays)
        print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")
        assert os.path.getsize(path) < (1 << 20), "a committed file must stay under 1 MiB"
    finally:
        os.chdir(cwd)
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
