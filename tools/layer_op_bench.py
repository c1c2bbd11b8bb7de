#!/usr/bin/env python3
"""Forward + backward of TWO encoder layers through torch.ops.dr4sr_hip.sasrec_layer (GPU box) at B = 256, L = 50, p = 0.5, d = 64 and
d = 128 (F = 128, H = 2), in ms per forward + backward, bracketed by device events around blocks of calls after warm-up, against
  (a) torch's own nn.TransformerEncoder (fp32, training mode, the reference's configuration and masks) on the same GPU — what a
      reference-side user replaces;
  (b) SasrecEngine.encode + encode_bwd at the same shape on toys-shaped rows — the project's packed path, which computes only the valid
      tokens (about 11 % of B * L) where the op computes every position: an expected loss for the op.
The op is timed twice: through autograd (what a user runs) and as bare op calls (forward launches and backward launches apart, which
names the larger phase).  Writes profiles/layer_op_bench.json.

Usage:  python tools/layer_op_bench.py [--out profiles/layer_op_bench.json] [--calls 100] [--blocks 3]
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

B, L, H, F, NL, P_DROP, EPS = 256, 50, 2, 128, 2, 0.5, 1e-12
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


def timed(fn, calls, blocks, warmup=50):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = [block_ms(fn, calls) for _ in range(blocks)]
    return {"ms_blocks": t, "median_ms": statistics.median(t)}


def measure(D, dev, calls, blocks):
    gen = torch.Generator().manual_seed(D)
    params = {}
    for n, s in zip(param_names(NL), param_shapes(TOYS_N_ITEMS, L, D, F, NL)):
        params[n] = (1.0 if n.endswith(("norm1.weight", "norm2.weight")) else 0.0) + 0.05 * torch.randn(s, generator=gen)
    params["item_embedding.weight"][0] = 0
    rows = make_rows(n_rows=B, n_items=TOYS_N_ITEMS, seed=5, dense=False)
    idx, sl = torch.from_numpy(rows["in_item_id"]).to(dev), torch.from_numpy(rows["seqlen"]).to(dev)
    key_pad = idx == 0
    x = torch.randn(B, L, D, generator=gen).to(dev)
    d_out = torch.randn(B, L, D, generator=gen).to(dev)
    pre = "query_encoder.transformer_layer.layers."
    w = [[params[f"{pre}{i}.{n}"].to(dev).requires_grad_(True) for n in LAYER] for i in range(NL)]
    o = torch.ops.dr4sr_hip
    xg = x.clone().requires_grad_(True)
    step = [0]

    def op_autograd():
        step[0] += 1
        y = xg
        for i in range(NL):
            y, _ = o.sasrec_layer(y, key_pad, True, *w[i], H, EPS, P_DROP, 7, step[0], i)
        torch.autograd.grad(y, [xg] + w[0] + w[1], d_out)

    wd = [[t.detach() for t in wi] for wi in w]
    kept = {}

    def op_fwd():
        ys, sv = [x], []
        for i in range(NL):
            y, s = o.sasrec_layer(ys[-1], key_pad, True, *wd[i], H, EPS, P_DROP, 7, 1, i)
            ys.append(y)
            sv.append(s)
        kept["ys"], kept["sv"] = ys, sv

    def op_bwd():
        dy = d_out
        for i in reversed(range(NL)):
            dy = o.sasrec_layer_backward(kept["ys"][i], key_pad, True, *wd[i], H, EPS, P_DROP, 7, 1, i, kept["sv"][i], dy)[0]

    # (a) torch's own encoder, configured and called as model/sasrec.py:21-34,:58,:65-68
    layer = torch.nn.TransformerEncoderLayer(d_model=D, nhead=H, dim_feedforward=F, dropout=P_DROP, activation="gelu", layer_norm_eps=EPS,
                                             batch_first=True, norm_first=False)
    enc = torch.nn.TransformerEncoder(layer, num_layers=NL).to(dev).train()
    causal = torch.triu(torch.ones(L, L, dtype=torch.bool, device=dev), 1)
    xt = x.clone().requires_grad_(True)
    tp = list(enc.parameters())

    def torch_encoder():
        y = enc(src=xt, mask=causal, src_key_padding_mask=key_pad)
        torch.autograd.grad(y, [xt] + tp, d_out)

    # (b) the engine's packed path on the same rows
    eng = SasrecEngine(TOYS_N_ITEMS, L, D, H, F, NL, EPS, P_DROP, B, dev)
    eng.load_named(params)
    plan = eng.make_plan(idx, None, sl)
    out = torch.empty(B, L, D, device=dev)

    def engine():
        eng.encode(plan, True, _lib.POOL_ORIGIN, out)
        eng.encode_bwd(plan, True, _lib.POOL_ORIGIN, d_out)

    r = {"D": D, "valid_token_fraction": float(sl.clamp(0, L).sum()) / (B * L),
         "op_autograd": timed(op_autograd, calls, blocks), "op_forward_launches": timed(op_fwd, calls, blocks),
         "op_backward_launches": timed(op_bwd, calls, blocks), "torch_encoder": timed(torch_encoder, calls, blocks),
         "engine_packed": timed(engine, calls, blocks)}
    m = {k: v["median_ms"] for k, v in r.items() if isinstance(v, dict)}
    r["op_vs_torch"] = m["op_autograd"] / m["torch_encoder"]
    r["op_vs_engine"] = m["op_autograd"] / m["engine_packed"]
    r["largest_phase"] = "backward launches" if m["op_backward_launches"] > m["op_forward_launches"] else "forward launches"
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layer_op_bench.json"))
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    assert a.calls * a.blocks >= 200, "at least 200 timed calls"
    dev = torch.device("cuda", 0)
    res = {"what": f"two encoder layers, forward + backward, B = {B}, L = {L}, F = {F}, H = {H}, p = {P_DROP}, fp32; ms per forward + backward, "
                   "host-enqueued (no graph), device events around blocks of calls after 50 warm-up calls",
           "device": torch.cuda.get_device_name(0), "calls_per_block": a.calls, "cases": []}
    for D in (64, 128):
        r = measure(D, dev, a.calls, a.blocks)
        print(f"d={D}: op {r['op_autograd']['median_ms']:.4f} ms (forward launches {r['op_forward_launches']['median_ms']:.4f}, backward "
              f"launches {r['op_backward_launches']['median_ms']:.4f}), torch encoder {r['torch_encoder']['median_ms']:.4f} ms, engine "
              f"{r['engine_packed']['median_ms']:.4f} ms; op / torch {r['op_vs_torch']:.3f}, op / engine {r['op_vs_engine']:.3f}", flush=True)
        res["cases"].append(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
