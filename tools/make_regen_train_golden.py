#!/usr/bin/env python3
"""Golden fixture of the regenerator's TRAIN-MODE gradient (tests/golden/regen_train_toys.npz + .partN.npz) by RUNNING the
reference's stage 2 classes on the CPU with model.train(), their random dropout replaced by the masks of dr4sr_amd/regen_dropout.py.

Works only where the reference checkout (USTC-StarTeam/DR4SR) exists; set-up as tools/make_regen_grad_golden.py (the same exec of
2.Pretrain_regenerator.py, the scoring fixture's checkpoint and its first pairs at the file-wide widths).  Only DATA is written.

What is patched while the reference's Generator runs:
  torch.nn.functional.dropout                        as nn.Dropout and multi_head_attention_forward look it up: call number i of a
                                                     forward multiplies by the host mirror's factors of the site the call order names
  torch.nn.functional.scaled_dot_product_attention   need_weights=False attention goes through it, dropout inside: replaced by
                                                     softmax(Q K^T / sqrt(d) + mask) -> factors of the probability site -> . V
The tool asserts that every one of the 30 sites is consumed exactly once per forward, with the expected shape.  F.gumbel_softmax is
recorded as the eval tool records it (tau = 1); the causal source mask, loss_fn + 1 * reg_loss, loss.backward().
Stored: the reference's fp32 gradient of every parameter, both loss terms (fp32 and float64), err32 per tensor = max |reference fp32 -
reference .double()|, the recorded noise and (p, seed, step).  No masks: they are regenerated.
Asserted: the reference in .double() against RegenModel.loss_and_grad(backend="torch", dtype=float64, dropout=...) to 1e-10 relative
per tensor; the fp32 restatement against the reference's fp32 within 4 x err32 per tensor.

Usage:  python tools/make_regen_train_golden.py [--out tests/golden/regen_train_toys.npz]
"""
import argparse
import json
import math
import os
import random
import sys
import tempfile
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
PART_BYTES = 1_000_000
N_BATCH = 256
P_DROP, SEED, STEP = 0.5, 20240229, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "tests", "golden", "regen_train_toys.npz"))
    a = ap.parse_args()
    from make_golden import _install_stubs
    from make_regen_golden import _run_script
    import make_regen_golden
    from make_regen_score_golden import N_ITEM, matrices
    make_regen_golden.N_ITEM = N_ITEM
    _install_stubs()
    sys.path.insert(0, REF)
    import torch
    import torch.nn.functional as F
    rng = random.Random(0)
    tmp = tempfile.mkdtemp(prefix="regen_train_golden_")
    root = os.path.join(tmp, "toy")
    os.makedirs(root)
    cwd = os.getcwd()
    os.chdir(REF)
    try:
        E = torch.load(os.path.join(REF, "dataset/amazon-toys/toy/pre-trained_embedding.ckpt"), map_location="cpu")
        torch.save({"parameters": {"item_embedding.weight": E["parameters"]["item_embedding.weight"][:N_ITEM].clone()}},
                   os.path.join(root, "pre-trained_embedding.ckpt"))
        train = []
        for _ in range(64):
            seq = [rng.randrange(1, N_ITEM) for _ in range(rng.randint(3, 12))]
            train.append([seq, [seq[p] for p in sorted(rng.sample(range(len(seq)), 2))]])
        torch.save(train, os.path.join(root, "seq-pat-pair.pth"))
        g = _run_script("2.Pretrain_regenerator.py", ["--root_path", root, "--epochs", "1"])
    finally:
        os.chdir(cwd)
    model, K = g["model"], g["K"]

    from dr4sr_amd import regen_dropout as rd
    from dr4sr_amd.regen import RegenModel, score_param_names
    z = np.load(os.path.join(os.path.dirname(HERE), "tests", "golden", "regen_score_toys.npz"))
    sd = {k: torch.from_numpy(z[f"p:{k}"].astype(np.float32)) for k in score_param_names()}
    sd["item_embedding_decoder.weight"] = sd["item_embedding.weight"].clone()
    missing = model.load_state_dict(sd, strict=True)
    model.train()
    all_pairs = json.loads(str(z["pairs_json"]))
    Ls, T = int(z["Ls"]), int(z["T"])
    src, tgt, sl, tl = matrices(torch, all_pairs)
    assert (src.shape[1], tgt.shape[1] - 1) == (Ls, T)
    pairs = all_pairs[:N_BATCH]
    src, tgt, sl, tl = src[:N_BATCH], tgt[:N_BATCH], sl[:N_BATCH], tl[:N_BATCH]
    assert all(all(v in s for v in t) for s, t in pairs)
    tied = model.item_embedding_decoder.weight is model.item_embedding.weight
    drop = rd.RegenDropout(P_DROP, SEED, STEP)
    pair_ids = list(range(N_BATCH))

    # ---- call order -> site: the order nn.Transformer's modules reach their dropout in Generator.forward
    enc = lambda st, l: [("p", rd.site(st, l, 0)), ("h", rd.site(st, l, 1), 64), ("h", rd.site(st, l, 2), 256), ("h", rd.site(st, l, 3), 64)]
    dec = lambda l: [("p", rd.site(rd.STACK_DEC, l, 0)), ("h", rd.site(rd.STACK_DEC, l, 1), 64), ("p", rd.site(rd.STACK_DEC, l, 2)),
                     ("h", rd.site(rd.STACK_DEC, l, 3), 64), ("h", rd.site(rd.STACK_DEC, l, 4), 256), ("h", rd.site(rd.STACK_DEC, l, 5), 64)]
    order = ([("h", rd.SITE_SRC_EMB, 64)] + enc(rd.STACK_SRC, 0) + enc(rd.STACK_SRC, 1) + [("h", rd.SITE_TGT_EMB, 64)]
             + enc(rd.STACK_COND, 0) + enc(rd.STACK_COND, 1) + dec(0) + dec(1))
    assert len(order) == rd.N_SITES and sorted(o[1] for o in order) == sorted(v[0] for v in rd.all_sites().values())
    calls = {"i": 0}

    def next_site(kind):
        assert calls["i"] < len(order), "more dropout calls than sites"
        o = order[calls["i"]]
        calls["i"] += 1
        assert o[0] == kind, (calls["i"] - 1, o, kind)
        return o

    def dropout(input, p=0.5, training=True, inplace=False):
        assert training and p == P_DROP and not inplace
        o = next_site("h")
        assert input.dim() == 3 and input.shape[0] == N_BATCH and input.shape[2] == o[2] and input.shape[1] in (Ls, T), (o, input.shape)
        return input * torch.from_numpy(rd.keep_rows(drop, o[1], pair_ids, input.shape[1], o[2])).to(input.dtype)

    def sdpa(query, key, value, attn_mask=None, dropout_p=0.0, is_causal=False, scale=None, **kw):
        assert dropout_p == P_DROP and not is_causal and scale is None and not kw
        o = next_site("p")
        assert query.dim() == 4 and tuple(query.shape[:2]) == (N_BATCH, 2) and query.shape[3] == 32, query.shape
        s = query @ key.transpose(-1, -2) / math.sqrt(query.shape[-1])
        if attn_mask is not None:
            assert attn_mask.dtype == query.dtype
            s = s + attn_mask
        a = torch.softmax(s, -1)
        a = a * torch.from_numpy(rd.keep_probs(drop, o[1], pair_ids, a.shape[2], a.shape[3])).to(a.dtype)
        return a @ value

    state = {"mode": "draw", "noise": None, "sample": None}

    def gumbel(logits, tau=1, hard=False, eps=1e-10, dim=-1):
        if state["mode"] == "draw":                   # the reference's own call, and the noise it drew, regenerated from the RNG state
            rs = torch.get_rng_state()
            out = F.gumbel_softmax(logits, tau=tau, hard=hard, dim=dim)
            torch.set_rng_state(rs)
            noise = -torch.empty_like(logits, memory_format=torch.legacy_contiguous_format).exponential_().log()
            assert torch.equal(((logits + noise) / tau).softmax(dim), out), "the regenerated Gumbel noise does not reproduce the sample"
            state["noise"] = noise.detach().clone()
        else:                                         # the recorded noise at another dtype
            out = ((logits + state["noise"].to(logits.dtype)) / tau).softmax(dim)
        state["sample"] = out.detach().clone()
        return out

    proxy = types.ModuleType("functional_proxy")
    proxy.__dict__.update(F.__dict__)
    proxy.gumbel_softmax = gumbel
    g["F"] = proxy

    def run(mdl, dtype):
        """train_epoch's forward and loss (2.Pretrain_regenerator.py:275-288) without the optimizer; gradients by parameter name"""
        mdl.zero_grad(set_to_none=True)
        mdl.condition_encoder.tau = 1
        assert mdl.training
        tgt_input = tgt[:, :-1]
        src_mask, tgt_mask, src_padding_mask, tgt_padding_mask = g["create_mask"](src, tgt_input)
        calls["i"] = 0
        saved = F.dropout, F.scaled_dot_product_attention
        F.dropout, F.scaled_dot_product_attention = dropout, sdpa
        try:
            logits = mdl(src, tgt_input, src_mask.to(dtype), tgt_mask.to(dtype), src_padding_mask, tgt_padding_mask, src_padding_mask, sl, tl)
        finally:
            F.dropout, F.scaled_dot_product_attention = saved
        assert calls["i"] == rd.N_SITES, f"{calls['i']} of the {rd.N_SITES} sites were consumed"
        tgt_out = tgt[:, 1:]
        loss = g["loss_fn"](logits.reshape(-1, logits.shape[-1]), tgt_out.reshape(-1))
        condition_prob = mdl.condition_encoder.condition4loss
        reg_loss = - (condition_prob * torch.log(condition_prob + 1e-12)).sum(-1).mean()
        (loss + 1 * reg_loss).backward()
        named = dict(mdl.named_parameters())
        grads = {}
        for k in score_param_names():
            gk = named[k].grad
            grads[k] = torch.zeros_like(named[k]) if gk is None else gk.detach().clone()
        if not tied:                                  # two Parameters holding one table: the table's gradient is their sum
            gd = named["item_embedding_decoder.weight"].grad
            if gd is not None:
                grads["item_embedding.weight"] = grads["item_embedding.weight"] + gd
        return grads, float(loss.detach()), float(reg_loss.detach())

    torch.manual_seed(1)
    state["mode"] = "draw"
    g32, l32, e32 = run(model, torch.float32)
    noise = state["noise"]
    model.double()
    state["mode"] = "noise"
    g64, l64, e64 = run(model, torch.float64)
    model.float()

    # ---- the restatement: float64 must BE the reference's float64; fp32 within 4 x err32 of the reference's fp32
    rm = RegenModel.from_state_dict(sd, "cpu")
    assert rm.has_condition_encoder and rm.K == K
    kw = dict(noise=noise, tau=1.0, entropy_weight=1.0, dropout=drop)
    r64 = rm.loss_and_grad(pairs, "encoder", True, (Ls, T), "torch", torch.float64, **kw)
    r32 = rm.loss_and_grad(pairs, "encoder", True, (Ls, T), "torch", torch.float32, **kw)
    err32, ratio32, agree, out = {}, {}, 0.0, {}
    for k in score_param_names():
        e = float((g32[k].double() - g64[k]).abs().max())
        err32[k] = e
        agree = max(agree, float((g64[k] - r64.grads[k]).abs().max()) / max(float(g64[k].abs().max()), 1e-300))
        d = float((r32.grads[k].double() - g32[k].double()).abs().max())
        ratio32[k] = d / e if e > 0 else (0.0 if d == 0 else float("inf"))
        assert d <= 4 * e, (k, d, e)
        out[f"g:{k}"] = g32[k].numpy().astype(np.float32)
    agree = max(agree, abs(float(r64.loss) - l64) / abs(l64), abs(float(r64.entropy) - e64) / abs(e64))
    print("float64 restatement vs the reference's modules in double, worst relative difference per tensor:", agree)
    assert agree < 1e-10, agree
    print("fp32 restatement vs the reference's fp32, worst ratio to err32:", max(ratio32.values()))
    eval_loss = float(rm.loss_and_grad(pairs, "encoder", True, (Ls, T), "torch", torch.float64, noise=noise, tau=1.0, entropy_weight=1.0).loss)
    assert abs(eval_loss - l64) > 1e-3, "the train-mode loss equals the eval-mode loss: no dropout reached the model"
    meta = dict(K=np.int32(K), n_pairs=np.int32(N_BATCH), Ls=np.int32(Ls), T=np.int32(T), noise=noise.numpy().astype(np.float32),
                err32=np.array(json.dumps(err32)), ratio32=np.array(json.dumps(ratio32)), agree64=np.float64(agree), tied_table=np.bool_(tied),
                p=np.float64(P_DROP), seed=np.uint64(SEED), step=np.uint32(STEP), loss=np.float64(l32), reg_loss=np.float64(e32),
                loss64=np.float64(l64), reg_loss64=np.float64(e64))
    parts, cur, size = [], {}, 0
    for k, v in out.items():
        if cur and size + v.nbytes > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += v.nbytes
    parts.append(cur)
    stem = a.out[:-4]
    names = []
    for i, part in enumerate(parts):
        name = f"{stem}.part{i}.npz"
        np.savez_compressed(name, **part)
        names.append(os.path.basename(name))
        print(name, os.path.getsize(name), "bytes")
        assert os.path.getsize(name) < (1 << 20)
    meta["parts"] = np.array(json.dumps(names))
    np.savez_compressed(a.out, **meta)
    print(a.out, os.path.getsize(a.out), "bytes; missing / unexpected keys on load:", missing)


if __name__ == "__main__":
    main()
