#!/usr/bin/env python3
"""Forward + backward of TWO encoder layers through torch.ops.dr4sr_hip.sasrec_layer_packed (GPU box; there is no CPU path) against the
dense torch.ops.dr4sr_hip.sasrec_layer, SasrecEngine.encode + encode_bwd and torch's fp32 nn.TransformerEncoder, at L = 50, F = 128, H = 2,
p = 0.5, d = 64 and 128, B = 256 and 8192, on two length sets:
  toys   the length histogram of dr4sr_amd.data.synthetic.make_rows (about 11 % of the positions valid): many sequences per tile;
  full   every length 50: one sequence per tile, the worst case for packing — the packed op should cost what the dense op costs, plus
         its plan launches and row table.
Each path runs through autograd (what a user runs); the packed and the dense op also as bare C-ABI launches on preallocated buffers,
forward and backward apart.  Times are ms per call from device events around blocks of calls after a warm-up of every path; the paths
ALTERNATE block by block inside one run, and the dense op is timed twice (dense_a, dense_b) so that the run carries its own spread.
The tile count and the mean tile fill of the plan stand beside each case.  Writes profiles/layer_packed_bench.json.

Usage:  python tools/layer_packed_bench.py [--out profiles/layer_packed_bench.json] [--calls 100] [--blocks 3] [--batches 256,8192]
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
import dr4sr_amd.ops  # noqa: E402,F401
from dr4sr_amd.data.synthetic import make_rows, TOYS_N_ITEMS  # noqa: E402
from dr4sr_amd.engine import SasrecEngine, param_names, param_shapes  # noqa: E402

L, H, F, NL, P_DROP, EPS = 50, 2, 128, 2, 0.5, 1e-12
LAYER = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias", "linear1.weight",
         "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")


def block_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def alternate(paths, calls, blocks, warmup):
    """{name: fn} -> {name: {ms_blocks, median_ms}}: every path warmed up, then one block of each path in turn, `blocks` times"""
    for fn in paths.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in paths}
    for _ in range(blocks):
        for k, fn in paths.items():
            t[k].append(block_ms(fn, calls))
    return {k: {"ms_blocks": v, "median_ms": statistics.median(v)} for k, v in t.items()}


def plan_figures(sl, B):
    lib = _lib.load()
    tile_of, row_of = (torch.empty(B, dtype=torch.int32, device=sl.device) for _ in range(2))
    n_tiles = torch.empty(1, dtype=torch.int32, device=sl.device)
    nb = lib.dr4sr_sasrec_layer_packed_workspace_bytes(B, L, 64, H, F, 0)
    ws = torch.empty(nb // 4, dtype=torch.int32, device=sl.device)
    plan = _lib.probe("dr4sr_sasrec_layer_packed_plan")
    _lib.check(plan(_lib.ptr(sl), B, L, _lib.ptr(tile_of), _lib.ptr(row_of), _lib.ptr(n_tiles), _lib.ptr(ws), nb, _lib.cur_stream()),
               "dr4sr_sasrec_layer_packed_plan")
    tiles, tokens = int(n_tiles), int(sl.clamp(0, L).sum())
    return {"tiles": tiles, "mean_tile_fill_rows": tokens / max(tiles, 1), "valid_token_fraction": tokens / (B * L),
            "sequences_per_tile": int((tile_of >= 0).sum()) / max(tiles, 1)}


def bare_launches(packed, x, sl, key_pad, wd, d_out, D):
    """(forward, backward) closures of the two layers' bare C-ABI launches on buffers allocated here, once"""
    lib = _lib.load()
    B = x.shape[0]
    dev = x.device
    if packed:
        n = lib.dr4sr_sasrec_layer_packed_saved_floats(B, L, D, H, F)
        nf, nb = (lib.dr4sr_sasrec_layer_packed_workspace_bytes(B, L, D, H, F, k) for k in (0, 1))
    else:
        n, nf, nb = lib.dr4sr_sasrec_layer_saved_floats(B, L, D, H, F), 0, lib.dr4sr_sasrec_layer_workspace_bytes(B, L, D, H, F)
    ys = [x] + [torch.empty_like(x) for _ in range(NL)]
    saved = [torch.empty(n, device=dev) for _ in range(NL)]
    dxs = [torch.empty_like(x) for _ in range(NL)] + [d_out]
    ws = torch.empty(max(nb, 16) // 4, device=dev)
    w = [_lib.LayerWeights(*[_lib.ptr(t) for t in wi]) for wi in wd]
    dws = [[torch.empty_like(t) for t in wi] for wi in wd]
    g = [_lib.LayerGrads(*[_lib.ptr(t) for t in gi]) for gi in dws]
    kp = key_pad.view(torch.uint8)
    st = _lib.cur_stream()

    def fwd():
        for i in range(NL):
            if packed:
                rc = lib.dr4sr_sasrec_layer_packed_fwd(_lib.ptr(ys[i]), _lib.ptr(sl), 1, w[i], B, L, D, H, F, EPS, P_DROP, 7, 1, i,
                                                       _lib.ptr(ys[i + 1]), _lib.ptr(saved[i]), _lib.ptr(ws), nf, st)
            else:
                rc = lib.dr4sr_sasrec_layer_fwd(_lib.ptr(ys[i]), _lib.ptr(kp), 1, w[i], B, L, D, H, F, EPS, P_DROP, 7, 1, i,
                                                _lib.ptr(ys[i + 1]), _lib.ptr(saved[i]), st)
            _lib.check(rc, "forward")

    def bwd():
        for i in reversed(range(NL)):
            if packed:
                rc = lib.dr4sr_sasrec_layer_packed_bwd(_lib.ptr(ys[i]), _lib.ptr(sl), 1, w[i], B, L, D, H, F, EPS, P_DROP, 7, 1, i,
                                                       _lib.ptr(saved[i]), _lib.ptr(dxs[i + 1]), _lib.ptr(dxs[i]), g[i], _lib.ptr(ws), nb, st)
            else:
                rc = lib.dr4sr_sasrec_layer_bwd(_lib.ptr(ys[i]), _lib.ptr(kp), 1, w[i], B, L, D, H, F, EPS, P_DROP, 7, 1, i,
                                                _lib.ptr(saved[i]), _lib.ptr(dxs[i + 1]), _lib.ptr(dxs[i]), g[i], _lib.ptr(ws), nb, st)
            _lib.check(rc, "backward")
    return fwd, bwd


def measure(B, D, lengths, dev, calls, blocks, warmup):
    gen = torch.Generator().manual_seed(D)
    params = {}
    for n, s in zip(param_names(NL), param_shapes(TOYS_N_ITEMS, L, D, F, NL)):
        params[n] = (1.0 if n.endswith(("norm1.weight", "norm2.weight")) else 0.0) + 0.05 * torch.randn(s, generator=gen)
    params["item_embedding.weight"][0] = 0
    if lengths == "toys":
        rows = make_rows(n_rows=B, n_items=TOYS_N_ITEMS, seed=5, dense=False)
        idx, sl = torch.from_numpy(rows["in_item_id"]).to(dev), torch.from_numpy(rows["seqlen"]).to(dev)
    else:
        idx = torch.randint(1, TOYS_N_ITEMS, (B, L), generator=gen).to(dev)
        sl = torch.full((B,), L, dtype=torch.int64, device=dev)
    key_pad = (idx == 0).contiguous()
    assert bool((key_pad == (torch.arange(L, device=dev).view(1, L) >= sl.view(B, 1))).all()), "post-padded rows"
    x = torch.randn(B, L, D, generator=gen).to(dev)
    d_out = torch.randn(B, L, D, generator=gen).to(dev)
    pre = "query_encoder.transformer_layer.layers."
    w = [[params[f"{pre}{i}.{n}"].to(dev).requires_grad_(True) for n in LAYER] for i in range(NL)]
    wd = [[t.detach() for t in wi] for wi in w]
    o = torch.ops.dr4sr_hip
    xg = x.clone().requires_grad_(True)
    step = [0]

    def packed():
        step[0] += 1
        y = xg
        for i in range(NL):
            y, _ = o.sasrec_layer_packed(y, sl, True, *w[i], H, EPS, P_DROP, 7, step[0], i)
        torch.autograd.grad(y, [xg] + w[0] + w[1], d_out)

    def dense():
        step[0] += 1
        y = xg
        for i in range(NL):
            y, _ = o.sasrec_layer(y, key_pad, True, *w[i], H, EPS, P_DROP, 7, step[0], i)
        torch.autograd.grad(y, [xg] + w[0] + w[1], d_out)

    layer = torch.nn.TransformerEncoderLayer(d_model=D, nhead=H, dim_feedforward=F, dropout=P_DROP, activation="gelu", layer_norm_eps=EPS,
                                             batch_first=True, norm_first=False)
    enc = torch.nn.TransformerEncoder(layer, num_layers=NL).to(dev).train()
    causal = torch.triu(torch.ones(L, L, dtype=torch.bool, device=dev), 1)
    xt = x.clone().requires_grad_(True)
    tp = list(enc.parameters())

    def torch_encoder():
        y = enc(src=xt, mask=causal, src_key_padding_mask=key_pad)
        torch.autograd.grad(y, [xt] + tp, d_out)

    eng = SasrecEngine(TOYS_N_ITEMS, L, D, H, F, NL, EPS, P_DROP, B, dev)
    eng.load_named(params)
    plan = eng.make_plan(idx, None, sl)
    out = torch.empty(B, L, D, device=dev)

    def engine():
        eng.encode(plan, True, _lib.POOL_ORIGIN, out)
        eng.encode_bwd(plan, True, _lib.POOL_ORIGIN, d_out)

    r = {"B": B, "D": D, "lengths": lengths, "plan": plan_figures(sl, B)}
    r["autograd"] = alternate({"packed": packed, "dense_a": dense, "engine": engine, "torch_encoder": torch_encoder, "dense_b": dense}, calls,
                              blocks, warmup)
    pf, pb = bare_launches(True, x, sl, key_pad, wd, d_out, D)
    df, db = bare_launches(False, x, sl, key_pad, wd, d_out, D)
    df(), pf()                                               # the backwards read what the forwards saved
    r["bare_launches"] = alternate({"packed_forward": pf, "dense_forward_a": df, "packed_backward": pb, "dense_backward_a": db,
                                    "dense_forward_b": df, "dense_backward_b": db}, calls, blocks, warmup)
    m = {k: v["median_ms"] for k, v in r["autograd"].items()}
    bm = {k: v["median_ms"] for k, v in r["bare_launches"].items()}
    dense_ms = 0.5 * (m["dense_a"] + m["dense_b"])
    r["dense_spread"] = abs(m["dense_a"] - m["dense_b"]) / dense_ms
    r["packed_vs_dense"] = m["packed"] / dense_ms
    r["packed_vs_engine"] = m["packed"] / m["engine"]
    r["packed_vs_torch"] = m["packed"] / m["torch_encoder"]
    r["bare_forward_packed_vs_dense"] = bm["packed_forward"] / (0.5 * (bm["dense_forward_a"] + bm["dense_forward_b"]))
    r["bare_backward_packed_vs_dense"] = bm["packed_backward"] / (0.5 * (bm["dense_backward_a"] + bm["dense_backward_b"]))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layer_packed_bench.json"))
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batches", default="256,8192")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/layer_packed_bench.py needs the GPU: libdr4sr_hip.so has no CPU path")
    assert a.calls * a.blocks >= 300, "at least 300 timed calls per path"
    dev = torch.device("cuda", 0)
    res = {"what": f"two encoder layers, forward + backward, L = {L}, F = {F}, H = {H}, p = {P_DROP}, fp32; ms per call, host-enqueued (no "
                   f"graph), device events around blocks of calls after {a.warmup} warm-up calls of every path, paths alternating block by block",
           "device": torch.cuda.get_device_name(0), "calls_per_block": a.calls, "blocks": a.blocks, "cases": []}
    for B in (int(v) for v in a.batches.split(",")):
        for D in (64, 128):
            for lengths in ("toys", "full"):
                r = measure(B, D, lengths, dev, a.calls, a.blocks, a.warmup)
                m = {k: v["median_ms"] for k, v in r["autograd"].items()}
                print(f"B={B} d={D} {lengths}: {r['plan']['tiles']} tiles, fill {r['plan']['mean_tile_fill_rows']:.1f} rows; packed "
                      f"{m['packed']:.4f} ms, dense {m['dense_a']:.4f} / {m['dense_b']:.4f}, engine {m['engine']:.4f}, torch "
                      f"{m['torch_encoder']:.4f}; packed / dense {r['packed_vs_dense']:.3f} (bare forward "
                      f"{r['bare_forward_packed_vs_dense']:.3f}, bare backward {r['bare_backward_packed_vs_dense']:.3f}), packed / engine "
                      f"{r['packed_vs_engine']:.3f}", flush=True)
                res["cases"].append(r)
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:                  # after every case: a run cut short keeps what it measured
                    json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
