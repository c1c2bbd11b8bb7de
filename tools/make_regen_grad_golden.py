#!/usr/bin/env python3
"""Golden fixture of the gradient of the regenerator's training loss (tests/golden/regen_grad_toys.npz + .partN.npz) by RUNNING the
reference's stage 2 classes on the CPU.

Works only where the reference checkout (USTC-StarTeam/DR4SR) exists.  2.Pretrain_regenerator.py is exec'd as tools/
make_regen_score_golden.py does (one epoch on a few synthetic pairs, only to obtain its Generator, create_mask and loss_fn); the
checkpoint and the pairs come from tests/golden/regen_score_toys.npz: its parameters, and its first 256 pairs (every target inside its
source) at the file-wide widths.  Only DATA is written.

  gumbel   model.eval(), autograd on, tau = 1, the causal source mask; F.gumbel_softmax runs as it is under a saved RNG state and the
           Gumbel noise it drew is regenerated from that state (asserted to reproduce its sample bit for bit) and recorded;
           loss = loss_fn + 1 * reg_loss as train_epoch forms it (2.Pretrain_regenerator.py:283-287); loss.backward().
  const    the same with the recorded sample injected as a detached constant (a leaf that requires grad): the condition encoder
           receives no gradient, and the leaf's gradient is dw plus the gradient of reg_loss, which the reference forms from the
           same tensor (condition4loss).
Stored per mode: the reference's fp32 gradient of every parameter, loss_fn, reg_loss, and per tensor err32 = max |reference fp32 -
float64| (the reference's own modules in .double() on the same noise); for const also dw and its err32.  The tool asserts that the
reference in .double() agrees with RegenModel.loss_and_grad(backend="torch", dtype=float64) to 1e-10 relative per tensor, and checks the
fp32 restatement against the reference's fp32 within 4 x err32 per tensor (the measured ratio is stored).

A file of the repository holds at most 1 MiB and the 98 gradient tensors are 1.9 MB per mode, so the arrays go into numbered part files
of at most 1 000 000 raw bytes each beside the main file, which lists them.

Usage:  python tools/make_regen_grad_golden.py [--out tests/golden/regen_grad_toys.npz]
"""
import argparse
import json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "tests", "golden", "regen_grad_toys.npz"))
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
    tmp = tempfile.mkdtemp(prefix="regen_grad_golden_")
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

    # ---- the checkpoint and the pairs of the scoring fixture
    from dr4sr_amd.regen import RegenModel, score_param_names
    z = np.load(os.path.join(os.path.dirname(HERE), "tests", "golden", "regen_score_toys.npz"))
    sd = {k: torch.from_numpy(z[f"p:{k}"].astype(np.float32)) for k in score_param_names()}
    sd["item_embedding_decoder.weight"] = sd["item_embedding.weight"].clone()
    missing = model.load_state_dict(sd, strict=True)
    model.eval()
    all_pairs = json.loads(str(z["pairs_json"]))
    Ls, T = int(z["Ls"]), int(z["T"])
    src, tgt, sl, tl = matrices(torch, all_pairs)
    assert (src.shape[1], tgt.shape[1] - 1) == (Ls, T)
    pairs = all_pairs[:N_BATCH]
    src, tgt, sl, tl = src[:N_BATCH], tgt[:N_BATCH], sl[:N_BATCH], tl[:N_BATCH]
    assert all(all(v in s for v in t) for s, t in pairs)
    tied = model.item_embedding_decoder.weight is model.item_embedding.weight

    state = {"mode": "draw", "noise": None, "sample": None, "inject": None}

    def gumbel(logits, tau=1, hard=False, eps=1e-10, dim=-1):
        if state["mode"] == "draw":                   # the reference's own call, and the noise it drew, regenerated from the RNG state
            rs = torch.get_rng_state()
            out = F.gumbel_softmax(logits, tau=tau, hard=hard, dim=dim)
            torch.set_rng_state(rs)
            noise = -torch.empty_like(logits, memory_format=torch.legacy_contiguous_format).exponential_().log()
            assert torch.equal(((logits + noise) / tau).softmax(dim), out), "the regenerated Gumbel noise does not reproduce the sample"
            state["noise"] = noise.detach().clone()
        elif state["mode"] == "noise":                # the recorded noise at another dtype
            out = ((logits + state["noise"].to(logits.dtype)) / tau).softmax(dim)
        else:                                         # a constant
            out = state["inject"]
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
        tgt_input = tgt[:, :-1]
        src_mask, tgt_mask, src_padding_mask, tgt_padding_mask = g["create_mask"](src, tgt_input)
        logits = mdl(src, tgt_input, src_mask.to(dtype), tgt_mask.to(dtype), src_padding_mask, tgt_padding_mask, src_padding_mask, sl, tl)
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
    out, ref = {}, {}
    state["mode"] = "draw"
    ref["gumbel", 32] = run(model, torch.float32)
    noise, sample = state["noise"], state["sample"]
    state["mode"], state["inject"] = "const", sample.clone().requires_grad_(True)
    ref["const", 32] = run(model, torch.float32)
    dw32 = state["inject"].grad.detach().clone()
    model.double()
    state["mode"] = "noise"
    ref["gumbel", 64] = run(model, torch.float64)
    state["mode"], state["inject"] = "const", sample.double().requires_grad_(True)
    ref["const", 64] = run(model, torch.float64)
    dw64 = state["inject"].grad.detach().clone()
    model.float()

    # ---- the restatement: float64 must BE the reference's float64; fp32 within 4 x err32 of the reference's fp32
    rm = RegenModel.from_state_dict(sd, "cpu")
    assert rm.has_condition_encoder and rm.K == K
    calls = {"gumbel": dict(conditions="encoder", noise=noise, tau=1.0, entropy_weight=1.0), "const": dict(conditions=sample[None])}
    err32, ratio32, agree = {}, {}, 0.0
    for mode in ("gumbel", "const"):
        g32, l32, e32 = ref[mode, 32]
        g64, l64, e64 = ref[mode, 64]
        kw = dict(calls[mode])
        cond = kw.pop("conditions")
        r64 = rm.loss_and_grad(pairs, cond.double() if mode == "const" else cond, True, (Ls, T), "torch", torch.float64, **kw)
        r32 = rm.loss_and_grad(pairs, cond, True, (Ls, T), "torch", torch.float32, **kw)
        items = [(k, g32[k], g64[k], r32.grads[k], r64.grads[k]) for k in score_param_names()]
        if mode == "const":
            # the injected tensor also feeds reg_loss (condition4loss), so the reference's gradient of it is dw + d reg_loss / dw
            dreg = lambda w: -(torch.log(w + 1e-12) + w / (w + 1e-12)) / w.shape[0]
            items.append(("dw", dw32, dw64, r32.dw[0] + dreg(sample), r64.dw[0] + dreg(sample.double())))
        for k, a32, a64, b32, b64 in items:
            e = float((a32.double() - a64).abs().max())
            err32[f"{mode}:{k}"] = e
            scale = max(float(a64.abs().max()), 1e-300)
            agree = max(agree, float((a64 - b64).abs().max()) / scale)
            d = float((b32.double() - a32.double()).abs().max())
            ratio32[f"{mode}:{k}"] = d / e if e > 0 else (0.0 if d == 0 else float("inf"))
            assert d <= 4 * e, (mode, k, d, e)
        agree = max(agree, abs(float(r64.loss) - l64) / abs(l64))
        if mode == "gumbel":
            agree = max(agree, abs(float(r64.entropy) - e64) / abs(e64))
        out[f"{mode}:loss"], out[f"{mode}:reg_loss"] = np.float64(l32), np.float64(e32)
        out[f"{mode}:loss64"], out[f"{mode}:reg_loss64"] = np.float64(l64), np.float64(e64)
        for k in score_param_names():
            out[f"{mode}:g:{k}"] = g32[k].numpy().astype(np.float32)
    print("float64 restatement vs the reference's modules in double, worst relative difference per tensor:", agree)
    assert agree < 1e-10, agree
    print("fp32 restatement vs the reference's fp32, worst ratio to err32:", max(ratio32.values()))
    out["const:dw"] = dw32.numpy().astype(np.float32)
    meta = dict(K=np.int32(K), n_pairs=np.int32(N_BATCH), Ls=np.int32(Ls), T=np.int32(T), noise=noise.numpy().astype(np.float32),
                sample=sample.numpy().astype(np.float32), err32=np.array(json.dumps(err32)), ratio32=np.array(json.dumps(ratio32)),
                agree64=np.float64(agree), tied_table=np.bool_(tied))
    for k in list(out):
        if np.ndim(out[k]) == 0:
            meta[k] = out.pop(k)
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
