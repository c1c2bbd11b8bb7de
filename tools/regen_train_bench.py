#!/usr/bin/env python3
"""Measurement of one pre-training step of the regenerator (dr4sr_amd/regen_train.py RegenTrainer.step) on one GPU.

Toys-shaped pairs (tools/regen_score_bench.py toys_pairs) at the toys widths (50, 19), N = 11 925 items, K = 5, batch 256, dropout 0.5,
a random regenerator with a condition encoder.  Three routes to the same step (forward, backward, Adam), each timed over windows of
--steps consecutive steps with the host clock around a window that ends in a device synchronise (what a training run pays per step:
host work included), the routes alternating inside every repeat; the median window is reported:
  trainer        RegenTrainer.step(): the batch gathered on the device, the condition head in HIP, dr4sr_adam_flat, no read-back
  parent_route   the same step with what the library had before the trainer: RegenModel.loss_and_grad(backend="hip", dropout=...) on
                 the batch's Python lists (packing, the membership check, two read-backs, the [n, K] autograd between the HIP calls),
                 then torch.optim.Adam on the returned tensors, stepping views of the model's flat buffer in place
  torch          fp32 autograd through the eager restatement with torch's own random masks at the 30 sites, then torch.optim.Adam
The trainer's window is also timed between device events (trainer_device_ms_per_step).  One JSON line on stdout and in --out.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--pairs", type=int, default=2560)
    ap.add_argument("--steps", type=int, default=30, help="steps per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dropout", type=float, default=0.5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regen_train_bench.json"))
    a = ap.parse_args()
    import torch
    from dr4sr_amd import regen, regen_torch
    from dr4sr_amd.regen_train import RegenTrainer, lr_at, tau_at
    from regen_score_bench import toys_pairs
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    width, seed, epochs = (50, 19), 2024, 40
    pairs = toys_pairs(400)[:a.pairs]
    assert len(pairs) == a.pairs, "raise toys_pairs' sequence count"
    sd = regen.random_state_dict(seed=3, std=0.1, condition_encoder=True)
    total = a.warmup + a.repeats * a.steps

    # ---- the trainer
    tr = RegenTrainer(regen.RegenModel.from_state_dict(sd, dev), pairs, epochs=epochs, batch_size=a.batch, dropout=a.dropout, seed=seed, width=width)
    assert total <= tr.loss_log.numel(), "fewer steps, or more pairs"

    def trainer_window(n):
        for _ in range(n):
            tr.step()

    # ---- the parent's route: loss_and_grad(backend="hip") + torch.optim.Adam on views of the model's flat buffer
    pm = regen.RegenModel.from_state_dict(sd, dev)
    p_views = [v.requires_grad_(True) for v in pm.grads_from_flat(pm.score_flat()).values()]
    p_names = list(pm.grads_from_flat(pm.score_flat()))
    p_opt = torch.optim.Adam(p_views, lr=1e-3, betas=(0.9, 0.98), eps=1e-9)
    perm = torch.randperm(len(pairs), generator=torch.Generator().manual_seed(0)).tolist()
    state = {"parent": 0, "torch": 0}

    def batch_of(s):
        lo = (s * a.batch) % (len(pairs) - a.batch + 1)
        return [pairs[i] for i in perm[lo:lo + a.batch]]

    def gumbel(n):
        return -torch.log(-torch.log(torch.rand(n, pm.K, device=dev).clamp_min(1e-9)))

    def parent_window(n):
        for _ in range(n):
            s = state["parent"]
            drop = regen.RegenDropout(a.dropout, seed, s) if a.dropout > 0 else None
            r = pm.loss_and_grad(batch_of(s), "encoder", True, width, "hip", noise=gumbel(a.batch), tau=tau_at(s), entropy_weight=1.0, dropout=drop)
            for g in p_opt.param_groups:
                g["lr"] = lr_at(s, 1e-3, epochs)
            for v, k in zip(p_views, p_names):
                v.grad = r.grads[k]
            p_opt.step()
            state["parent"] = s + 1

    # ---- fp32 torch autograd with torch's own dropout
    tm = regen.RegenModel.from_state_dict(sd, dev)
    leaves = {k: v.clone().requires_grad_(True) for k, v in tm.p.items()}
    t_opt = torch.optim.Adam(list(leaves.values()), lr=1e-3, betas=(0.9, 0.98), eps=1e-9)

    class TorchRandomDrop:                  # torch's own masks at the restatement's sites
        def rows(self, s, x):
            return (torch.rand_like(x) >= a.dropout).to(x.dtype) / (1.0 - a.dropout)
        probs = rows

    tdrop = TorchRandomDrop() if a.dropout > 0 else None
    packed = tm._pack_pairs(pairs, width)
    src_d, tgt_d, tl_d = packed[0].to(dev), packed[2].to(dev), packed[3].to(dev)
    n_tok_cpu = (packed[2][:, 1:] != 0).sum(1)

    def torch_window(n):
        for _ in range(n):
            s = state["torch"]
            lo = (s * a.batch) % (len(pairs) - a.batch + 1)
            idx = torch.tensor(perm[lo:lo + a.batch])
            n_tok = int(n_tok_cpu[idx].sum())
            idx = idx.to(dev)
            src, tgt, tl = src_d[idx], tgt_d[idx], tl_d[idx]
            t_opt.zero_grad(set_to_none=True)
            c = regen_torch.score_forward(tm, src, tgt, tl, None, True, True, torch.float32, leaves, tdrop)[1]
            w0 = torch.softmax((c + gumbel(a.batch)) / tau_at(s), -1)
            ent = -(w0 * torch.log(w0 + 1e-12)).sum(-1).mean()
            nll, _ = regen_torch.score_forward(tm, src, tgt, tl, w0[None], False, True, torch.float32, leaves, tdrop)
            (nll.sum() / n_tok + ent).backward()
            for g in t_opt.param_groups:
                g["lr"] = lr_at(s, 1e-3, epochs)
            t_opt.step()
            state["torch"] = s + 1

    routes = {"trainer": trainer_window, "parent_route": parent_window}
    if not a.no_torch:
        routes["torch"] = torch_window
    for fn in routes.values():
        fn(a.warmup)
    torch.cuda.synchronize()
    wall = {k: [] for k in routes}
    device_ms = []
    for _ in range(a.repeats):
        for k, fn in routes.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn(a.steps)
            e1.record()
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
            if k == "trainer":
                device_ms.append(e0.elapsed_time(e1) / a.steps)
    r = {"metric": "regen_train_step", "batch": a.batch, "pairs": len(pairs), "width": list(width), "n_rows": tr.model.n_rows, "K": tr.model.K,
         "dropout": a.dropout, "n_params": tr.n_params, "steps_per_window": a.steps, "repeats": a.repeats, "warmup_steps": a.warmup,
         "trainer_device_ms_per_step": round(float(np.median(device_ms)), 3)}
    for k in routes:
        med = float(np.median(wall[k]))
        r[f"{k}_ms_per_step"] = round(med, 3)
        r[f"{k}_ms_per_step_min_max"] = [round(min(wall[k]), 3), round(max(wall[k]), 3)]
        r[f"{k}_steps_per_s"] = round(1e3 / med, 2)
    for k in routes:
        if k != "trainer":
            r[f"{k}_over_trainer"] = round(r[f"{k}_ms_per_step"] / r["trainer_ms_per_step"], 2)
    losses = tr.loss_log[:tr.s].double().cpu()
    r["trainer_loss_first_last"] = [round(float(losses[:5].mean()), 4), round(float(losses[-5:].mean()), 4)]
    assert math.isfinite(r["trainer_loss_first_last"][1])
    line = json.dumps(r)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
