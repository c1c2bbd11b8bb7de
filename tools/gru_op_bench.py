#!/usr/bin/env python3
"""Forward + backward of TWO GRU layers (D = 64 -> H = 256 -> H = 256, no biases, L = 50) through torch.ops.dr4sr_hip.gru_layer (GPU box)
at one batch size per run (B = 256: the latency regime, B = 8192: the throughput regime), in ms per forward + backward, bracketed by
device events around blocks of calls after warm-up, variants alternating block by block (the method of tools/fmlp_op_bench.py):
  (a) the op through autograd with `seqlen` drawn from the amazon-toys length histogram (11 % of the positions valid);
  (b) the op through autograd with seqlen = None: every position computed, what the reference does;
  (c) fp32 torch.nn.GRU(64, 256, 2, bias=False, batch_first=True) on the same GPU through autograd — what a reference-side user replaces;
  (d) GruEngine.encode + encode_bwd on item ids of the same lengths — the project's plan-based path: packed valid tokens, bf16x3
      recurrences, cooperative multi-CU recurrence at small B; it ALSO does the embedding gather, the H -> D projection, the pooling and
      their backward, which (a) - (c) do not;
  and the bare launches of (a), forward and backward apart.
Then the group-size table: the bare launches of (a) and (b) with 16, 8 and 4 sequences per workgroup of the recurrence launches
(DR4SR_GRU_OP_GROUP), which is what csrc/gru_op.hip group_of chooses from.
Merges its result into profiles/gru_op_bench.json under the key "B<batch>".

Usage:  python tools/gru_op_bench.py --batch 256 [--calls 50] [--blocks 5] [--out profiles/gru_op_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dr4sr_amd.ops  # noqa: E402,F401
from dr4sr_amd import _lib  # noqa: E402
from dr4sr_amd.data.synthetic import TOYS_N_ITEMS, make_rows  # noqa: E402
from dr4sr_amd.gru_engine import GruEngine, gru_param_names, gru_param_shapes  # noqa: E402

L, D, H, NL = 50, 64, 256, 2
GROUP = "DR4SR_GRU_OP_GROUP"


def block_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def timed_alternating(fns, calls, blocks, warmup):
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


def measure(dev, B, calls, blocks, warmup):
    gen = torch.Generator().manual_seed(B)
    rows = make_rows(n_rows=B, n_items=TOYS_N_ITEMS, L=L, seed=3)
    idx, sl = torch.from_numpy(rows["in_item_id"]).to(dev), torch.from_numpy(rows["seqlen"]).to(dev)
    params = {}
    for n, s in zip(gru_param_names(NL), gru_param_shapes(TOYS_N_ITEMS, D, H, NL)):
        params[n] = 0.08 * torch.randn(s, generator=gen)
    params["item_embedding.weight"][0] = 0
    w = [[params[f"query_encoder.0.3.gru.weight_{k}_l{l}"].to(dev).requires_grad_(True) for k in ("ih", "hh")] for l in range(NL)]
    x = torch.randn(B, L, D, generator=gen).to(dev)
    d_out = torch.randn(B, L, H, generator=gen).to(dev)
    o = torch.ops.dr4sr_hip
    xg = x.clone().requires_grad_(True)

    def op_autograd(seqlen):
        def run():
            y = xg
            for l in range(NL):
                y, _ = o.gru_layer(y, *w[l], seqlen)
            torch.autograd.grad(y, [xg] + w[0] + w[1], d_out)
        return run

    wd = [[t.detach() for t in wl] for wl in w]
    kept = {}

    def op_fwd(seqlen):
        def run():
            ys, sv = [x], []
            for l in range(NL):
                y, s = o.gru_layer(ys[-1], *wd[l], seqlen)
                ys.append(y)
                sv.append(s)
            kept[seqlen is None] = (ys, sv)
        return run

    def op_bwd(seqlen):
        def run():
            ys, sv = kept[seqlen is None]
            dy = d_out
            for l in reversed(range(NL)):
                dy = o.gru_layer_backward(ys[l], *wd[l], seqlen, ys[l + 1], sv[l], dy)[0]
        return run

    # (c) torch's own GRU
    gru = torch.nn.GRU(D, H, NL, bias=False, batch_first=True).to(dev)
    with torch.no_grad():
        for l in range(NL):
            getattr(gru, f"weight_ih_l{l}").copy_(wd[l][0])
            getattr(gru, f"weight_hh_l{l}").copy_(wd[l][1])
    xt = x.clone().requires_grad_(True)

    def torch_gru():
        y, _ = gru(xt)
        torch.autograd.grad(y, [xt] + list(gru.parameters()), d_out)

    # (d) the engine (item ids in, [B, L, D] 'origin' queries out)
    eng = GruEngine(TOYS_N_ITEMS, L, D, H, NL, 0.0, B, dev)
    eng.load_named(params)
    plan = eng.make_plan(idx, None, sl)
    out = torch.empty(B, L, D, device=dev)
    d_q = torch.randn(B, L, D, generator=gen).to(dev)

    def engine():
        eng.encode(plan, True, _lib.POOL_ORIGIN, out)
        eng.encode_bwd(plan, True, _lib.POOL_ORIGIN, d_q)

    op_fwd(sl)()
    op_fwd(None)()
    r = timed_alternating({"op_autograd_seqlen": op_autograd(sl), "op_autograd_all_positions": op_autograd(None), "torch_gru_fp32": torch_gru,
                           "engine": engine, "op_seqlen_forward_launches": op_fwd(sl), "op_seqlen_backward_launches": op_bwd(sl)},
                          calls, blocks, warmup)
    eng.check_coop()
    m = {k: v["median_ms"] for k, v in r.items()}
    r["valid_positions"] = float(sl.clamp(0, L).sum()) / (B * L)
    r["default_group"] = 4 if B <= 1024 else (8 if B <= 2048 else 16)
    r["op_seqlen_vs_torch"] = m["op_autograd_seqlen"] / m["torch_gru_fp32"]
    r["op_all_positions_vs_torch"] = m["op_autograd_all_positions"] / m["torch_gru_fp32"]
    r["op_seqlen_vs_engine"] = m["op_autograd_seqlen"] / m["engine"]
    # the group-size table: bare launches, every size in turn inside each block
    table = {}
    fns = {}
    for gs in (16, 8, 4):
        for tag, seqlen in (("seqlen", sl), ("all_positions", None)):
            def both(gs=gs, seqlen=seqlen):
                _lib.set_env(GROUP, gs)
                op_fwd(seqlen)()
                op_bwd(seqlen)()
            fns[f"group{gs}_{tag}"] = both
    table = timed_alternating(fns, max(calls // 2, 2), blocks, max(warmup // 4, 2))
    _lib.set_env(GROUP, None)
    r["group_size_table_fwd_plus_bwd_launches"] = table
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru_op_bench.json"))
    ap.add_argument("--batch", type=int, required=True)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    r = measure(dev, a.batch, a.calls, a.blocks, a.warmup)
    m = {k: v["median_ms"] for k, v in r.items() if isinstance(v, dict) and "median_ms" in v}
    print(f"B = {a.batch}: " + ", ".join(f"{k} {v:.4f} ms" for k, v in m.items()), flush=True)
    print("group sizes: " + ", ".join(f"{k} {v['median_ms']:.4f} ms" for k, v in r["group_size_table_fwd_plus_bwd_launches"].items()), flush=True)
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    res["what"] = (f"two GRU layers ({D} -> {H} -> {H}, no biases), forward + backward, L = {L}, fp32; ms per forward + backward, host-enqueued "
                   "(no graph), device events around blocks of calls after warm-up, variants alternating block by block; seqlen from the "
                   "amazon-toys length histogram")
    res["device"] = torch.cuda.get_device_name(0)
    r["calls_per_block"], r["warmup_calls"] = a.calls, a.warmup
    res[f"B{a.batch}"] = r
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
