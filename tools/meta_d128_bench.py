#!/usr/bin/env python3
"""Measurement of DR4SR+ at embed_dim 128 on one GPU -> profiles/meta_d128_bench.json (one JSON line per record).

  select   dr4sr_meta_select_fwd_d (gate_out recorded) and dr4sr_meta_select_bwd_d (d_query + d_phi; it evaluates the forward itself) at
           12 800 positions (B 256 x L 50, 37 live targets per row), Philox noise, between HIP events, against fp32 torch autograd of the
           same function on the same GPU (forward under no_grad; forward + backward), in alternating rounds; D = 128 and, for scale, D = 64
  step     the weighted inner step (MetaModel._train_batch: captured graph of negatives, dense weighted fwd/bwd, Adam) and the outer step
           (MetaModel._outter_loop: hyper-gradient + meta SGD) at B = 256 on toys-sized synthetic rows, d = 128, and the d = 64 DENSE path
           (DR4SR_META_DENSE=1: the same composition; d = 64's default is the fused step) beside it; host clock around synchronised work,
           alternating rounds
Every figure is a median over --rounds rounds, each round timing --inner calls; min and max over rounds are kept.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("DR4SR_CONFIG_DIR", os.path.join(ROOT, "configs"))
os.environ["DR4SR_META_DENSE"] = "1"                      # read by MetaModel._fused_ok only where d = 64


def stats(xs, key):
    return {key: round(float(np.median(xs)), 4), key + "_min": round(float(min(xs)), 4), key + "_max": round(float(max(xs)), 4)}


def select_records(torch, rounds, inner):
    from dr4sr_amd import _lib
    lib, P = _lib.load(), _lib.ptr
    B, L, tau = 256, 50, 3.0
    n = B * L
    cases = {}
    for D in (128, 64):
        g = torch.Generator().manual_seed(D)
        W1, b1 = (torch.randn(D, D, generator=g) * (1.6 / D ** 0.5)).cuda(), (torch.randn(D, generator=g) * 0.1).cuda()
        W2, b2 = (torch.randn(2, D, generator=g) * 0.3).cuda(), (torch.randn(2, generator=g) * 0.1).cuda()
        phi = torch.cat([W1.reshape(-1), b1, W2.reshape(-1), b2]).contiguous()
        q = torch.randn(n, D, generator=g).cuda()
        tgt = torch.randint(1, 100, (B, L), generator=g)
        tgt[:, 37:] = 0
        tgt = tgt.cuda()
        uid = torch.arange(1, B + 1).cuda()
        up = torch.randn(n, generator=g).cuda()
        gum = -torch.empty(n, 2).exponential_(generator=g).log().cuda()
        w, gate = torch.empty(n, device="cuda"), torch.empty(n * (D // 64), dtype=torch.int64, device="cuda")
        dq, dphi = torch.zeros(n, D, device="cuda"), torch.zeros(phi.numel(), device="cuda")
        ws = torch.empty(int(lib.dr4sr_meta_select_workspace_floats_d(n, D)), device="cuda")
        live = (tgt != 0).reshape(-1).float()

        def hip_fwd(D=D, q=q, phi=phi, uid=uid, tgt=tgt, gate=gate, w=w):
            _lib.check(lib.dr4sr_meta_select_fwd_d(P(q), P(phi), None, 5, 1, None, tau, P(uid), P(tgt), B, L, D, None, P(gate), P(w),
                                                 _lib.cur_stream()), "fwd")

        def hip_bwd(D=D, q=q, phi=phi, uid=uid, tgt=tgt, up=up, dq=dq, dphi=dphi, ws=ws):
            _lib.check(lib.dr4sr_meta_select_bwd_d(P(q), P(phi), None, 5, 1, None, tau, P(uid), P(tgt), B, L, D, None, P(up), None, P(dq), P(dphi),
                                                 P(ws), _lib.cur_stream()), "bwd")
        leaves = [t.clone().requires_grad_(True) for t in (q, W1, b1, W2, b2)]

        def torch_fn(ls, gum=gum, live=live):
            qq, a, b, c, d = ls
            logits = torch.relu(qq @ a.T + b) @ c.T + d
            return ((logits + gum) / tau).softmax(-1)[:, 0] * live

        def torch_fwd(leaves=leaves):
            with torch.no_grad():
                torch_fn(leaves)

        def torch_fwd_bwd(leaves=leaves, up=up):
            for t in leaves:
                t.grad = None
            (torch_fn(leaves) * up).sum().backward()
        cases[D] = {"hip_fwd_us": hip_fwd, "hip_bwd_us": hip_bwd, "torch_fwd_us": torch_fwd, "torch_fwd_bwd_us": torch_fwd_bwd}
    times = {(D, k): [] for D in cases for k in cases[D]}
    for r in range(rounds + 1):                                # round 0 warms every shape up
        for D in cases:
            for k, fn in cases[D].items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                fn()
                e0.record()
                for _ in range(inner):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if r:
                    times[(D, k)].append(e0.elapsed_time(e1) * 1e3 / inner)
    out = []
    for D in cases:
        rec = {"metric": "meta_select", "D": D, "positions": n, "live_positions": B * 37, "noise": "philox", "rounds": rounds, "inner": inner}
        for k in cases[D]:
            rec.update(stats(times[(D, k)], k))
        rec["hip_fwd_plus_bwd_us"] = round(rec["hip_fwd_us"] + rec["hip_bwd_us"], 4)
        rec["torch_over_hip_fwd"] = round(rec["torch_fwd_us"] / rec["hip_fwd_us"], 2)
        rec["torch_fwd_bwd_over_hip_bwd"] = round(rec["torch_fwd_bwd_us"] / rec["hip_bwd_us"], 2)
        out.append(rec)
    return out


def step_records(torch, rounds, inner):
    from test_gpu_meta import make_config
    from dr4sr_amd.utils import prepare_datasets, prepare_model, seed_everything
    models = {}
    for D in (128, 64):
        cfg = make_config(11925, dropout=0.5, n_rows=1024, batch=256, epochs=1, warmup=-1, interval=10 ** 9)
        cfg["model"]["embed_dim"] = D
        cfg["model"]["sub_overrides"]["model"]["embed_dim"] = D
        seed_everything(cfg["train"]["seed"])
        ds = prepare_datasets(cfg)
        m = prepare_model(cfg, ds)
        m._init_model(ds[0])
        m.train()
        assert not m._fused_ok()
        loader = ds[0].get_loader()
        models[D] = (m, m._local_batch(loader, m._perm(loader), 0))
    times = {(D, k): [] for D in models for k in ("weighted_step_us", "outer_step_us")}
    for r in range(rounds + 1):
        for D, (m, batch) in models.items():
            for k, fn, reps in (("weighted_step_us", lambda: m._train_batch(batch, 0), inner), ("outer_step_us", lambda: m._outter_loop(0), max(1, inner // 10))):
                fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
                if r:
                    times[(D, k)].append((time.perf_counter() - t0) * 1e6 / reps)
    out = []
    for D, (m, batch) in models.items():
        rec = {"metric": "metamodel_dense_step", "embed_dim": D, "batch": 256, "n_items": 11925, "dropout": 0.5, "path": "dense weighted step (hip_graph)",
               "n_phi": m._phi.n, "rounds": rounds, "inner": inner}
        for k in ("weighted_step_us", "outer_step_us"):
            rec.update(stats(times[(D, k)], k))
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meta_d128_bench.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    torch.cuda.set_device(0)
    lines = [json.dumps(r) for r in select_records(torch, a.rounds, a.inner) + step_records(torch, a.rounds, a.inner)]
    for ln in lines:
        print(ln, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
