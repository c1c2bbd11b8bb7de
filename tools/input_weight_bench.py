#!/usr/bin/env python3
"""Cost of SASRec's per-token input weight on the HIP encoder (GPU box): encode + encode_bwd (training mode, origin pooling) with and
without an input_weight / d_input_weight, timed with device events after 30 warm-up calls, on toys-shaped rows at B = 256 and B = 8 192,
d = 64 and d = 128.  Every shape is timed in alternating blocks (plain, weighted, plain, ...) so that clock drift hits both alike; the
spread of the plain blocks is the yardstick for the ratio.  Writes profiles/input_weight_bench.json.

Usage:  python tools/input_weight_bench.py [--out profiles/input_weight_bench.json] [--calls 100] [--blocks 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dr4sr_amd import _lib  # noqa: E402
from dr4sr_amd.data.synthetic import make_rows, TOYS_N_ITEMS  # noqa: E402
from dr4sr_amd.engine import SasrecEngine, param_names, param_shapes  # noqa: E402

L, H, F, NL = 50, 2, 128, 2


def engine(B, D, dev):
    gen = torch.Generator().manual_seed(D)
    eng = SasrecEngine(TOYS_N_ITEMS, L, D, H, F, NL, 1e-12, 0.5, B, dev)
    p = {}
    for n, s in zip(param_names(NL), param_shapes(TOYS_N_ITEMS, L, D, F, NL)):
        p[n] = (1.0 if n.endswith(("norm1.weight", "norm2.weight")) else 0.0) + 0.05 * torch.randn(s, generator=gen)
    p["item_embedding.weight"][0] = 0
    eng.load_named(p)
    return eng


def block_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def measure(B, D, dev, calls, blocks, warmup=30):
    eng = engine(B, D, dev)
    rows = make_rows(n_rows=B, n_items=TOYS_N_ITEMS, seed=5, dense=False)
    idx, sl = torch.from_numpy(rows["in_item_id"]).to(dev), torch.from_numpy(rows["seqlen"]).to(dev)
    plan = eng.make_plan(idx, None, sl)
    gen = torch.Generator().manual_seed(1)
    w = (0.25 + 1.5 * torch.rand(B, L, generator=gen)).to(dev)
    dw = torch.zeros(B, L, device=dev)
    d_out = torch.randn(B, L, D, generator=gen).to(dev)
    out = torch.empty(B, L, D, device=dev)

    def plain():
        eng.encode(plan, True, _lib.POOL_ORIGIN, out)
        eng.encode_bwd(plan, True, _lib.POOL_ORIGIN, d_out)

    def weighted():
        eng.encode(plan, True, _lib.POOL_ORIGIN, out, input_weight=w)
        eng.encode_bwd(plan, True, _lib.POOL_ORIGIN, d_out, input_weight=w, d_input_weight=dw)
    for _ in range(warmup):
        plain()
        weighted()
    torch.cuda.synchronize()
    t = {"plain": [], "weighted": []}
    for _ in range(blocks):
        t["plain"].append(block_ms(plain, calls))
        t["weighted"].append(block_ms(weighted, calls))
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"B": B, "D": D, "tokens": int(sl.clamp(0, L).sum()), "at_scale_bits": int(eng.lib.dr4sr_sasrec_at_scale(_lib.C.byref(plan))),
            "ms_plain": t["plain"], "ms_weighted": t["weighted"], "median_plain": med["plain"], "median_weighted": med["weighted"],
            "ratio": med["weighted"] / med["plain"], "plain_spread": (max(t["plain"]) - min(t["plain"])) / med["plain"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_weight_bench.json"))
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    res = {"what": "encode + encode_bwd, training mode, origin pooling, toys-shaped rows; ms per pair of calls, host-enqueued (no graph)",
           "device": torch.cuda.get_device_name(0), "calls_per_block": a.calls, "cases": []}
    for B in (256, 8192):
        for D in (64, 128):
            r = measure(B, D, dev, a.calls, a.blocks)
            print(f"B={B} d={D}: plain {r['median_plain']:.4f} ms, weighted {r['median_weighted']:.4f} ms, ratio {r['ratio']:.4f} "
                  f"(plain blocks spread {100 * r['plain_spread']:.1f} %)", flush=True)
            res["cases"].append(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
