#!/usr/bin/env python3
"""Forward + backward of TWO FMLP layers through torch.ops.dr4sr_hip.fmlp_layer (GPU box) at B = 256, L = 50, D = 64, p = 0.5, in ms per
forward + backward, bracketed by device events around blocks of calls after warm-up, against
  (a) the same computation in fp32 torch (torch.fft.rfft / irfft + F.layer_norm + F.linear + F.gelu + F.dropout, autograd) on the same
      GPU — what a reference-side user replaces;
  (b) FmlpEngine.encode + encode_bwd at the same shape — the project's plan-based path.  It computes the same B * L positions as the op
      (FMLP has no packed form), and ALSO the embedding gather + LayerNorm and the x[:, -1] selection and their backward, which the op
      chain timed here does not: the engine does slightly more work.
The variants are timed in alternation, block by block.  The op is timed twice: through autograd (what a user runs) and as bare op calls
(forward launches and backward launches apart, which names the larger phase).  Writes profiles/fmlp_op_bench.json.

Usage:  python tools/fmlp_op_bench.py [--out profiles/fmlp_op_bench.json] [--calls 200] [--blocks 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dr4sr_amd.ops  # noqa: E402,F401
from dr4sr_amd.data.synthetic import TOYS_N_ITEMS  # noqa: E402
from dr4sr_amd.fmlp_engine import FmlpEngine, fmlp_param_names, fmlp_param_shapes  # noqa: E402

B, L, D, F, NL, P_DROP, EPS = 256, 50, 64, 256, 2, 0.5, 1e-12
LAYER = ("filterlayer.complex_weight", "filterlayer.LayerNorm.weight", "filterlayer.LayerNorm.bias", "intermediate.dense_1.weight",
         "intermediate.dense_1.bias", "intermediate.dense_2.weight", "intermediate.dense_2.bias", "intermediate.LayerNorm.weight",
         "intermediate.LayerNorm.bias")


def block_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def timed_alternating(fns, calls, blocks, warmup=50):
    """{name: fn} -> {name: {"ms_blocks", "median_ms"}}: every variant warmed up, then one block of each in turn, `blocks` times"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(blocks):
        for k, fn in fns.items():
            t[k].append(block_ms(fn, calls))
    return {k: {"ms_blocks": v, "median_ms": statistics.median(v)} for k, v in t.items()}


def measure(dev, calls, blocks):
    gen = torch.Generator().manual_seed(D)
    params = {}
    for n, s in zip(fmlp_param_names(NL), fmlp_param_shapes(TOYS_N_ITEMS, L, D, F, NL)):
        params[n] = (1.0 if n.endswith("LayerNorm.weight") else 0.0) + 0.05 * torch.randn(s, generator=gen)
    params["item_embedding.weight"][0] = 0
    idx = torch.zeros(B, L, dtype=torch.long)
    for i in range(B):                                      # left-padded prefixes
        n = int(torch.randint(1, L + 1, (1,), generator=gen))
        idx[i, L - n:] = torch.randint(1, TOYS_N_ITEMS, (n,), generator=gen)
    idx = idx.to(dev)
    x = torch.randn(B, L, D, generator=gen).to(dev)
    d_out = torch.randn(B, L, D, generator=gen).to(dev)
    w = [[params[f"item_encoder.layer.{i}.{n}"].to(dev).requires_grad_(True) for n in LAYER] for i in range(NL)]
    o = torch.ops.dr4sr_hip
    xg = x.clone().requires_grad_(True)
    step = [0]

    def op_autograd():
        step[0] += 1
        y = xg
        for i in range(NL):
            y, _ = o.fmlp_layer(y, *w[i], EPS, P_DROP, 7, step[0], i)
        torch.autograd.grad(y, [xg] + w[0] + w[1], d_out)

    wd = [[t.detach() for t in wi] for wi in w]
    kept = {}

    def op_fwd():
        ys, sv = [x], []
        for i in range(NL):
            y, s = o.fmlp_layer(ys[-1], *wd[i], EPS, P_DROP, 7, 1, i)
            ys.append(y)
            sv.append(s)
        kept["ys"], kept["sv"] = ys, sv

    def op_bwd():
        dy = d_out
        for i in reversed(range(NL)):
            dy = o.fmlp_layer_backward(kept["ys"][i], *wd[i], EPS, P_DROP, 7, 1, i, kept["sv"][i], dy)[0]

    # (a) the reference's formulas (module/layers.py:740-791) in fp32 torch, training mode
    xt = x.clone().requires_grad_(True)
    wt = [[t.detach().clone().requires_grad_(True) for t in wi] for wi in w]

    def torch_layers():
        y = xt
        for cw, fw, fb, w1, b1, w2, b2, iw, ib in wt:
            f = torch.fft.irfft(torch.fft.rfft(y, dim=1, norm="ortho") * torch.view_as_complex(cw), n=L, dim=1, norm="ortho")
            y = Fn.layer_norm(Fn.dropout(f, P_DROP, True) + y, (D,), fw, fb, EPS)
            h = Fn.linear(Fn.gelu(Fn.linear(y, w1, b1)), w2, b2)
            y = Fn.layer_norm(Fn.dropout(h, P_DROP, True) + y, (D,), iw, ib, EPS)
        torch.autograd.grad(y, [xt] + wt[0] + wt[1], d_out)

    # (b) the engine on the same shape (item ids in, x[:, -1] out)
    eng = FmlpEngine(TOYS_N_ITEMS, L, D, F, NL, EPS, P_DROP, B, dev)
    eng.load_named(params)
    plan = eng.make_plan(idx, None)
    out = torch.empty(B, D, device=dev)
    d_last = torch.randn(B, D, generator=gen).to(dev)

    def engine():
        eng.encode(plan, True, out)
        eng.encode_bwd(plan, True, d_last)

    op_fwd()
    r = timed_alternating({"op_autograd": op_autograd, "op_forward_launches": op_fwd, "op_backward_launches": op_bwd,
                           "torch_fp32": torch_layers, "engine": engine}, calls, blocks)
    m = {k: v["median_ms"] for k, v in r.items()}
    r["op_vs_torch"] = m["op_autograd"] / m["torch_fp32"]
    r["op_vs_engine"] = m["op_autograd"] / m["engine"]
    r["op_launches_vs_engine"] = (m["op_forward_launches"] + m["op_backward_launches"]) / m["engine"]
    r["largest_phase"] = "backward launches" if m["op_backward_launches"] > m["op_forward_launches"] else "forward launches"
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fmlp_op_bench.json"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    assert a.calls * a.blocks >= 200, "at least 200 timed calls"
    dev = torch.device("cuda", 0)
    res = {"what": f"two FMLP layers, forward + backward, B = {B}, L = {L}, D = {D}, F = {F}, p = {P_DROP}, fp32; ms per forward + backward, "
                   "host-enqueued (no graph), device events around blocks of calls after 50 warm-up calls, variants alternating block by block",
           "device": torch.cuda.get_device_name(0), "calls_per_block": a.calls}
    r = measure(dev, a.calls, a.blocks)
    print(f"op {r['op_autograd']['median_ms']:.4f} ms (forward launches {r['op_forward_launches']['median_ms']:.4f}, backward launches "
          f"{r['op_backward_launches']['median_ms']:.4f}), torch fp32 {r['torch_fp32']['median_ms']:.4f} ms, engine "
          f"{r['engine']['median_ms']:.4f} ms; op / torch {r['op_vs_torch']:.3f}, op / engine {r['op_vs_engine']:.3f}, bare op launches / "
          f"engine {r['op_launches_vs_engine']:.3f}", flush=True)
    res.update(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
