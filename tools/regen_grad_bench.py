#!/usr/bin/env python3
"""Measurement of the gradient of the regenerator's teacher-forced loss (RegenModel.loss_and_grad, csrc/regen_score_bwd.hip) on one GPU.

Toys-shaped pairs (tools/regen_score_bench.py toys_pairs), K = 5, a random regenerator with a condition encoder, at 256 pairs (the
reference's batch) and 4 096 pairs, with explicit [2, n, 5] weights and with "encoder" (noise, tau 0.7, entropy weight 1).  Per case:
  fwd_ms        RegenModel.score_device (+ condition_device in "encoder" mode) alone, the forward the backward runs again
  hip_ms        the device calls of loss_and_grad(backend="hip") on tensors already on the device, SCORE_BWD_PAIRS_PER_CALL pairs per
                call, workspace and gradient buffer reused: score_bwd_device, and in "encoder" mode condition_device, the [n, K]
                autograd and condition_bwd_device; between HIP events, median of --repeats after --warmup
  loss_and_grad_wall_ms   RegenModel.loss_and_grad(backend="hip") itself, host wall clock around the whole call (packing the pairs, the
                per-pair membership check, copies, every chunk, synchronised): median of 3 after one warm-up
  torch_ms      fp32 autograd through the eager restatement on the same GPU over the same rows (forward + backward of the same scalar)
One JSON line per case on stdout and in --out.  --profile runs only the HIP path (for rocprofv3 --kernel-trace --stats).
--dropout P measures TRAIN MODE instead: the HIP calls take RegenDropout(P, seed 1, step 1) with pair0 = the chunk's first pair (the
DropPhilox kernels), and torch_ms is the same autograd with torch's own random masks of the same shapes at the same 30 sites (what
model.train() costs in torch; not the host mirror's masks, whose numpy generation is no part of a training step).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--dropout", type=float, default=0.0, help="train mode with this drop probability (0: eval mode)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from dr4sr_amd import regen, regen_torch
    from regen_score_bench import median_ms, toys_pairs
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    m = regen.RegenModel.from_state_dict(regen.random_state_dict(seed=3, std=0.3, condition_encoder=True), dev)
    all_pairs = toys_pairs(1200)
    lib = regen._lib.load()
    drop = regen.RegenDropout(a.dropout, 1, 1) if a.dropout > 0 else None

    class TorchRandomDrop:                  # torch's own masks at the restatement's sites
        def rows(self, s, x):
            return (torch.rand_like(x) >= a.dropout).to(x.dtype) / (1.0 - a.dropout)
        probs = rows

    tdrop = TorchRandomDrop() if drop is not None else None
    step = regen.SCORE_BWD_PAIRS_PER_CALL
    lines = []
    for n in a.sizes:
        pairs = all_pairs[:n]
        assert len(pairs) == n, "raise toys_pairs' sequence count"
        src, src_len, tgt, tgt_len, Ls, T = m._pack_pairs(pairs, None)
        n_tok = int((tgt[:, 1:] != 0).sum())
        g = torch.Generator().manual_seed(0)
        mixed = torch.softmax(2 * torch.randn(2, n, m.K, generator=g), -1).to(dev)
        noise = -torch.log(-torch.log(torch.rand(n, m.K, generator=g).clamp_min(1e-9))).to(dev)
        chunks = [[t[lo:lo + step].to(dev).contiguous() for t in (src, src_len, tgt, tgt_len)] + [lo] for lo in range(0, n, step)]
        grad = torch.empty(m.score_flat().numel(), device=dev)
        for mode in ("weights", "encoder"):
            n_w = 2 if mode == "weights" else 1
            ws = torch.empty(int(lib.dr4sr_regen_score_bwd_workspace_bytes(regen.C.byref(m.score_plan()), min(n, step), Ls, T, n_w)),
                             dtype=torch.uint8, device=dev)
            wsc = torch.empty(int(lib.dr4sr_regen_score_condition_bwd_workspace_bytes(regen.C.byref(m.score_plan()), min(n, step), T)),
                              dtype=torch.uint8, device=dev)

            def weights_of(c, lo, hi):
                if mode == "weights":
                    return mixed[:, lo:hi].contiguous(), None, None
                w0 = torch.softmax((c + noise[lo:hi]) / 0.7, -1)
                return w0.detach()[None].contiguous(), w0, -(w0 * torch.log(w0 + 1e-12)).sum(-1).sum() / n

            def run_hip():
                for i, (s, sl, t, tl, lo) in enumerate(chunks):
                    hi = lo + s.shape[0]
                    c = m.condition_device(t, tl, wsc, drop, lo).requires_grad_(True) if mode == "encoder" else None
                    w, w0, ent = weights_of(c, lo, hi)
                    dnll = torch.full((n_w, hi - lo, T), 1.0 / n_tok, device=dev)
                    _, dw, _ = m.score_bwd_device(s, sl, t, tl, w, dnll, True, grad, i > 0, ws, drop, lo)
                    if mode == "encoder":
                        (dl,) = torch.autograd.grad((w0 * dw[0]).sum() + ent, c)
                        m.condition_bwd_device(t, tl, dl.contiguous(), grad, True, wsc, drop, lo)

            def run_fwd():
                for s, sl, t, tl, lo in chunks:
                    c = m.condition_device(t, tl, wsc, drop, lo) if mode == "encoder" else None
                    m.score_device(s, sl, t, tl, weights_of(c, lo, lo + s.shape[0])[0], True, ws, drop, lo)

            if a.profile:
                run_hip()
                run_hip()
                torch.cuda.synchronize()
                continue
            leaves = {k: v.clone().requires_grad_(True) for k, v in m.p.items()}

            def run_torch():
                for v in leaves.values():
                    v.grad = None
                for lo in range(0, n, regen.ROWS_PER_TORCH):
                    s, t, tl = (x[lo:lo + regen.ROWS_PER_TORCH].to(dev) for x in (src, tgt, tgt_len))
                    hi = lo + s.shape[0]
                    c = regen_torch.score_forward(m, s, t, tl, None, True, True, torch.float32, leaves, tdrop)[1] if mode == "encoder" else None
                    w, w0, ent = weights_of(c, lo, hi)
                    if mode == "encoder":
                        w = w0[None]
                    nll, _ = regen_torch.score_forward(m, s, t, tl, w, False, True, torch.float32, leaves, tdrop)
                    (nll.sum() / n_tok + (ent if ent is not None else 0.0)).backward()

            r = {"metric": "regen_loss_and_grad", "mode": mode, "pairs": n, "n_w": n_w, "live_tokens": n_tok * n_w, "K": m.K, "width": [Ls, T],
                 "pairs_per_call": step, "dropout": a.dropout, "workspace_mb": round(ws.numel() / 2 ** 20, 1), "repeats": a.repeats}
            for key, fn in (("fwd_ms", run_fwd), ("hip_ms", run_hip), ("torch_ms", run_torch)):
                med, lo_, hi_ = median_ms(torch, fn, a.warmup, a.repeats)
                r.update({key: round(med, 3), key + "_min": round(lo_, 3), key + "_max": round(hi_, 3)})
            r["hip_speedup_vs_torch"] = round(r["torch_ms"] / r["hip_ms"], 2)
            # the method itself, as a user calls it: host packing, the per-pair membership check, copies to the device, every chunk
            call = dict(noise=noise.cpu(), tau=0.7, entropy_weight=1.0) if mode == "encoder" else {}
            cond = "encoder" if mode == "encoder" else mixed.cpu()
            wall = []
            for _ in range(1 + 3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m.loss_and_grad(pairs, cond, True, None, "hip", dropout=drop, **call)
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
            r["loss_and_grad_wall_ms"] = round(float(np.median(wall[1:])), 3)
            print(json.dumps(r), flush=True)
            lines.append(json.dumps(r))
    if a.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
