#!/usr/bin/env python3
"""Golden fixture of teacher-forced regenerator scoring (tests/golden/regen_score_toys.npz) by RUNNING the reference's stage 2 script.

Works only where the reference checkout (USTC-StarTeam/DR4SR) exists.  2.Pretrain_regenerator.py is exec'd unmodified apart from two
in-memory substitutions ('cuda' -> 'cpu', the item count of 'toy' -> N_ITEM); only DATA is written.

  1. The script trains its Generator for a few epochs on clean synthetic pairs (every target a subsequence of its source: one target id
     outside its source makes the reference's training loss inf).  `model` is taken from the exec'd globals, its parameters are rounded
     to fp16-representable values and loaded back.
  2. model.eval() with autograd enabled (torch's fused inference path, which zero-fills pad positions, is then not taken: checked on
     the condition encoder's output).  F.gumbel_softmax in the script's globals is replaced by a recorder / injector.  The held-out
     pairs are scored at their file-wide widths exactly as train_epoch calls the model, F.cross_entropy(ignore_index=0,
     reduction='none'): with real Gumbel samples (recorded), with each one-hot condition, with softmax(condition logits); all three
     again with an all-zero src_mask (stage 3's bidirectional encoder).  Also: the scalar loss_fn of the first 256 pairs, and the rows
     that fill the target width scored once more one column wider (their EOS is then pooled by the condition encoder).
  3. err32 per mode and quantity: max |reference fp32 - float64| over finite values, the float64 side being dr4sr_amd.regen's
     backend="torch" restatement; the reference's own modules converted with .double() must agree with it to 1e-10.

Usage:  python tools/make_regen_score_golden.py [--out tests/golden/regen_score_toys.npz] [--epochs 3]
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
N_ITEM = 200
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def held_out_pairs(rng, topics):
    """the scored pairs; the three whose target holds an id outside the source come last (after the 256-pair loss batch)"""
    pairs = []

    def sub(seq, k):
        pos = sorted(rng.sample(range(len(seq)), k))
        return [seq[p] for p in pos]

    for i in range(290):
        tp = rng.choice(topics)
        seq = [rng.choice(tp) for _ in range(rng.randint(3, 30))]
        pairs.append([seq, sub(seq, 1 + i % min(6, len(seq)))])
    for n in (18, 25, 31):                                   # targets of 18 ids fill the width: len(t) + 2 = 20 = T + 1
        seq = rng.sample(range(1, N_ITEM), n)
        pairs.append([seq, sub(seq, 18)])
    seq = rng.sample(range(1, N_ITEM), 48)                   # a source row of 50 ids
    pairs.append([seq, sub(seq, 4)])
    seq = rng.sample(range(1, N_ITEM), 9)
    seq = seq[:4] + [seq[1]] + seq[4:] + [seq[1], seq[6]]    # repeated ids in the source, and one of them twice in the target
    pairs.append([seq, [seq[1], seq[3], seq[4]]])
    assert pairs[-1][1][0] == pairs[-1][1][2]
    rng.shuffle(pairs)
    for n in (4, 9, 15):
        seq = rng.sample(range(1, N_ITEM), n)
        out = next(v for v in range(1, N_ITEM) if v not in seq)
        t = sub(seq, 2)
        pairs.append([seq, [t[0], out, t[1]]])
    return pairs


def matrices(torch, pairs, T1=None):
    """2.Pretrain_regenerator.py:49-64"""
    from torch.nn.utils.rnn import pad_sequence
    src = pad_sequence([torch.tensor([N_ITEM] + s + [N_ITEM + 1]) for s, _ in pairs], batch_first=True, padding_value=0)
    tgt = pad_sequence([torch.tensor([N_ITEM] + t + [N_ITEM + 1]) for _, t in pairs], batch_first=True, padding_value=0)
    want = max(20, tgt.shape[1]) if T1 is None else T1
    if tgt.shape[1] < want:
        tgt = torch.cat([tgt, torch.zeros(tgt.shape[0], want - tgt.shape[1], dtype=torch.long)], dim=-1)
    return src, tgt, torch.tensor([len(s) + 2 for s, _ in pairs]), torch.tensor([len(t) + 2 for _, t in pairs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "tests", "golden", "regen_score_toys.npz"))
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from make_golden import _install_stubs
    from make_regen_golden import _run_script
    import make_regen_golden
    make_regen_golden.N_ITEM = N_ITEM
    _install_stubs()
    sys.path.insert(0, REF)
    import torch
    import torch.nn.functional as F
    rng = random.Random(a.seed)
    tmp = tempfile.mkdtemp(prefix="regen_score_golden_")
    root = os.path.join(tmp, "toy")
    os.makedirs(root)
    cwd = os.getcwd()
    os.chdir(REF)
    try:
        E = torch.load(os.path.join(REF, "dataset/amazon-toys/toy/pre-trained_embedding.ckpt"), map_location="cpu")
        E = E["parameters"]["item_embedding.weight"][:N_ITEM].clone()
        torch.save({"parameters": {"item_embedding.weight": E}}, os.path.join(root, "pre-trained_embedding.ckpt"))
        topics = [rng.sample(range(1, N_ITEM), 40) for _ in range(8)]
        train = []
        for _ in range(1000):
            tp = rng.choice(topics)
            seq = [rng.choice(tp) for _ in range(rng.randint(3, 20))]
            pos = sorted(rng.sample(range(len(seq)), rng.randint(1, min(5, len(seq)))))
            train.append([seq, [seq[p] for p in pos]])
        torch.save(train, os.path.join(root, "seq-pat-pair.pth"))
        g = _run_script("2.Pretrain_regenerator.py", ["--root_path", root, "--epochs", str(a.epochs)])
    finally:
        os.chdir(cwd)
    model, K = g["model"], g["K"]
    sd = {k: (v.detach().half().float() if v.is_floating_point() else v.detach().clone()) for k, v in model.state_dict().items()}
    model.load_state_dict(sd)
    model.eval()

    # ---- the recorder / injector in place of F.gumbel_softmax (the script's classes look `F` up in the exec'd globals)
    state = {"inject": None, "logits": None, "sample": None}

    def gumbel(logits, tau=1, hard=False, eps=1e-10, dim=-1):
        state["logits"] = logits.detach().clone()
        out = F.gumbel_softmax(logits, tau=tau, hard=hard, dim=dim) if state["inject"] is None else state["inject"](logits)
        state["sample"] = out.detach().clone()
        return out

    proxy = types.ModuleType("functional_proxy")
    proxy.__dict__.update(F.__dict__)
    proxy.gumbel_softmax = gumbel
    g["F"] = proxy
    pad_out = {}
    model.condition_encoder.encoder.register_forward_hook(lambda m, i, o: pad_out.__setitem__("y", o.detach()))

    pairs = held_out_pairs(rng, topics)
    src, tgt, sl, tl = matrices(torch, pairs)
    n, Ls, T = len(pairs), src.shape[1], tgt.shape[1] - 1
    census = {"pairs": n, "Ls": Ls, "T": T, "target_lengths": sorted({len(t) for _, t in pairs}),
              "fill_width": sum(len(t) + 2 == T + 1 for _, t in pairs), "source_of_50": sum(len(s) + 2 == 50 for s, _ in pairs),
              "source_repeats": sum(len(set(s)) < len(s) for s, _ in pairs), "target_repeats": sum(len(set(t)) < len(t) for _, t in pairs),
              "target_outside_source": sum(any(v not in s for v in t) for s, t in pairs)}
    print("census:", json.dumps(census))
    assert census["fill_width"] >= 2 and census["source_of_50"] >= 1 and census["target_repeats"] >= 1 and census["source_repeats"] >= 1
    assert census["target_outside_source"] == 3 and min(census["target_lengths"]) == 1 and (Ls, T) == (50, 19)

    def run(mdl, src, tgt, sl, tl, inject, causal, dtype=torch.float32, reduce=False):
        """train_epoch's call of the model (2.Pretrain_regenerator.py:275-283) and the per-token cross entropy"""
        state["inject"] = inject
        tgt_input = tgt[:, :-1]
        src_mask, tgt_mask, src_padding_mask, tgt_padding_mask = g["create_mask"](src, tgt_input)
        if not causal:
            src_mask = torch.zeros_like(src_mask)
        logits = mdl(src, tgt_input, src_mask.to(dtype), tgt_mask.to(dtype), src_padding_mask, tgt_padding_mask, src_padding_mask, sl, tl)
        tgt_out = tgt[:, 1:]
        if reduce:
            return g["loss_fn"](logits.reshape(-1, logits.shape[-1]), tgt_out.reshape(-1)).detach()
        ce = F.cross_entropy(logits.reshape(-1, logits.shape[-1]), tgt_out.reshape(-1), ignore_index=0, reduction="none")
        return ce.detach().reshape(tgt_out.shape), state["logits"], state["sample"]

    def one_hot(k):
        return lambda lg: F.one_hot(torch.full(lg.shape[:1], k), K).to(lg.dtype)

    def evaluate(mdl, dtype, w_gumbel=None):
        out = {"nll_gumbel": [], "nll_onehot": [], "nll_softmax": [], "w_gumbel": []}
        for ci, causal in enumerate((True, False)):
            inj = None if w_gumbel is None else (lambda lg, ci=ci: w_gumbel[ci].to(lg.dtype))
            ce, lg, w = run(mdl, src, tgt, sl, tl, inj, causal, dtype)
            out["nll_gumbel"].append(ce)
            out["w_gumbel"].append(w)
            out["cond_logits"] = lg
            out["nll_onehot"].append(torch.stack([run(mdl, src, tgt, sl, tl, one_hot(k), causal, dtype)[0] for k in range(K)]))
            out["nll_softmax"].append(run(mdl, src, tgt, sl, tl, lambda lg: torch.softmax(lg, -1), causal, dtype)[0])
        return {k: (torch.stack(v) if isinstance(v, list) else v) for k, v in out.items()}

    torch.manual_seed(a.seed + 1)
    ref = evaluate(model, torch.float32)
    pad_pos = int(tl.min())                                   # a pad position of the shortest target
    assert float(pad_out["y"][int(tl.argmin()), pad_pos].abs().max()) > 0, "the fused inference path zero-filled the pad positions"
    batch = slice(0, 256)
    loss_batch = run(model, src[batch], tgt[batch], sl[batch], tl[batch], lambda lg: torch.softmax(lg, -1), True, reduce=True)
    wide = [i for i, (_, t) in enumerate(pairs) if len(t) + 2 == T + 1]
    pw = [pairs[i] for i in wide]
    srcw, tgtw, slw, tlw = matrices(torch, pw, T + 2)
    srcw = torch.cat([srcw, torch.zeros(len(pw), Ls - srcw.shape[1], dtype=torch.long)], 1)
    wide_nll = torch.stack([run(model, srcw, tgtw, slw, tlw, one_hot(k), True)[0] for k in range(K)])
    wide_cond = state["logits"]

    # ---- float64: the restatement, and the reference's own modules in double as its check
    from dr4sr_amd.regen import RegenModel, score_param_names
    rm = RegenModel.from_state_dict(sd, "cpu")
    assert rm.has_condition_encoder and rm.K == K
    ref64 = evaluate(model.double(), torch.float64, ref["w_gumbel"])
    wide64 = torch.stack([run(model, srcw, tgtw, slw, tlw, one_hot(k), True, torch.float64)[0] for k in range(K)])
    wide_cond64 = state["logits"]
    model.float()
    err32, agree = {}, 0.0

    def diff(x, y):
        fin = torch.isfinite(x) & torch.isfinite(y)
        assert torch.equal(torch.isinf(x), torch.isinf(y))
        return float((x.double() - y.double())[fin].abs().max())

    for ci, causal in enumerate((True, False)):
        tag = "causal" if causal else "bidir"
        r = rm.score(pairs, ref["w_gumbel"][ci][None], causal, (Ls, T), "torch", torch.float64)
        err32[f"nll_gumbel_{tag}"] = diff(ref["nll_gumbel"][ci], r.nll[0])
        agree = max(agree, diff(ref64["nll_gumbel"][ci], r.nll[0]), diff(ref64["cond_logits"], r.cond_logits))
        r = rm.score(pairs, "all", causal, (Ls, T), "torch", torch.float64)
        err32[f"nll_onehot_{tag}"] = diff(ref["nll_onehot"][ci], r.nll)
        agree = max(agree, diff(ref64["nll_onehot"][ci], r.nll))
        r = rm.score(pairs, "encoder", causal, (Ls, T), "torch", torch.float64)
        err32[f"nll_softmax_{tag}"] = diff(ref["nll_softmax"][ci], r.nll[0])
        agree = max(agree, diff(ref64["nll_softmax"][ci], r.nll[0]))
        err32["cond_logits"] = diff(ref["cond_logits"], r.cond_logits)
    r = rm.score(pw, "all", True, (Ls, T + 1), "torch", torch.float64)
    err32["wide_nll"] = diff(wide_nll, r.nll)
    err32["wide_cond"] = diff(wide_cond, r.cond_logits)
    agree = max(agree, diff(wide64, r.nll), diff(wide_cond64, r.cond_logits))
    r = rm.score(pairs[batch], "encoder", True, (Ls, T), "torch", torch.float64)
    err32["loss_batch"] = abs(float(loss_batch) - float(r.loss()[0]))
    print("err32:", json.dumps(err32))
    print("float64 restatement vs the reference's modules in double:", agree)
    assert agree < 1e-10, agree

    out = {f"p:{k}": sd[k].numpy().astype(np.float16) for k in score_param_names()}
    for k in score_param_names():
        assert np.array_equal(out[f"p:{k}"].astype(np.float32), sd[k].numpy()), k
    f32 = lambda t: t.numpy().astype(np.float32)
    out.update(K=np.int32(K), n_item=np.int32(N_ITEM), Ls=np.int32(Ls), T=np.int32(T), pairs_json=np.array(json.dumps(pairs)),
               census=np.array(json.dumps(census)), err32=np.array(json.dumps(err32)),
               nll_gumbel=f32(ref["nll_gumbel"]), nll_onehot=f32(ref["nll_onehot"]), nll_softmax=f32(ref["nll_softmax"]),
               w_gumbel=f32(ref["w_gumbel"]), cond_logits=f32(ref["cond_logits"]), loss_batch=np.float32(float(loss_batch)),
               loss_batch_n=np.int32(256), wide_idx=np.array(wide, np.int32), wide_nll=f32(wide_nll), wide_cond=f32(wide_cond))
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
