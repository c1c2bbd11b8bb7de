#!/usr/bin/env python3
"""The bits of teacher-forced scoring and of its gradients (csrc/regen_score.hip, csrc/regen_score_bwd.hip), for comparing two builds
of the library: a refactor of those files must not move one of them.

  regen_bits.py --out A.npz         runs the loaded library (DR4SR_LIB_PATH selects another build) on fixed seeds and writes every
                                    output below; one process per library
  regen_bits.py --compare A.npz B.npz    numpy.array_equal and the same bytes per array; exit status 1 on a difference

Cases: the committed scoring / gradient fixture (tests/golden/regen_score_toys.npz, its first 256 pairs for the gradients), 5 000
random toys-shaped pairs with K = 5 (the sizes of tests/test_gpu_regen_grad.py; the pair generator is the tests', restated here), and
1 000 with K = 3.  Per case: nll with a causal and a bidirectional source for [2, n, K] weights and for the encoder's own (n_w = 2 and
1), the condition logits, every gradient tensor, dw and the loss of loss_and_grad with [2, n, K] weights and with "encoder" + noise,
and the condition encoder's gradients (condition_grad).  These are the 42 eval-mode arrays.
A library that has the train-mode entry points adds `train:` arrays (dropout 0.5, seed 1, step 1, on the first 1 000 pairs of a case):
both NLLs, the condition logits, both gradients with dw and loss, and condition_grad.  --compare --allow-new lists the arrays only the
second file has as `new` instead of counting them as missing (an older build against a newer one).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def toys_shaped_pairs(n, n_item, seed):
    g = np.random.default_rng(seed)
    lens = np.minimum(g.geometric(1 / 9.0, n) + 1, 48)
    lens[:4] = [48, 2, 30, 18]
    pairs = []
    for i, l in enumerate(lens):
        s = g.integers(1, n_item, int(l)).tolist()
        k = 18 if (i % 97 == 3 and l >= 18) else int(g.integers(1, min(6, l) + 1))
        pos = sorted(g.choice(int(l), k, replace=False).tolist())
        pairs.append([s, [s[p] for p in pos]])
    return pairs


def outputs_of(torch, m, pairs, grad_pairs, width, seed, tag, out):
    from dr4sr_amd.regen import score_param_names
    g = torch.Generator().manual_seed(seed)
    mixed = torch.softmax(2 * torch.randn(2, len(pairs), m.K, generator=g), -1)
    noise = -torch.log(-torch.log(torch.rand(len(pairs), m.K, generator=g).clamp_min(1e-9)))
    dl = torch.randn(len(pairs), m.K, generator=g)
    ng = len(grad_pairs)
    for causal in (True, False):
        side = "causal" if causal else "bidir"
        r = m.score(pairs, mixed, causal, width, "hip")
        out[f"{tag}:nll:{side}:n_w2"] = r.nll.numpy()
        r = m.score(pairs, "encoder", causal, width, "hip")
        out[f"{tag}:nll:{side}:encoder"] = r.nll.numpy()
    out[f"{tag}:cond_logits"] = r.cond_logits.numpy()
    for name, cond, kw in (("n_w2", mixed[:, :ng], {}), ("encoder", "encoder", dict(noise=noise[:ng], tau=0.7, entropy_weight=1.0))):
        for causal in (True, False):
            side = "causal" if causal else "bidir"
            r = m.loss_and_grad(grad_pairs, cond, causal, width, "hip", **kw)
            out[f"{tag}:grad:{side}:{name}"] = torch.cat([r.grads[k].reshape(-1) for k in score_param_names()]).cpu().numpy()
            out[f"{tag}:dw:{side}:{name}"] = r.dw.cpu().numpy()
            out[f"{tag}:loss:{side}:{name}"] = np.float64(float(r.loss))
    cg = m.condition_grad(pairs, dl, width, "hip")
    out[f"{tag}:condition_grad"] = torch.cat([cg[k].reshape(-1) for k in cg]).cpu().numpy()
    if hasattr(m, "score_bwd_device") and "dropout" in m.score_bwd_device.__code__.co_varnames:
        from dr4sr_amd.regen import RegenDropout
        d = RegenDropout(0.5, 1, 1)
        tp, tg = pairs[:1000], grad_pairs[:1000]
        r = m.score(tp, mixed[:, :len(tp)], True, width, "hip", dropout=d)
        out[f"train:{tag}:nll:causal:n_w2"] = r.nll.numpy()
        r = m.score(tp, "encoder", False, width, "hip", dropout=d)
        out[f"train:{tag}:nll:bidir:encoder"] = r.nll.numpy()
        out[f"train:{tag}:cond_logits"] = r.cond_logits.numpy()
        for name, cond, causal, kw in (("causal:n_w2", mixed[:, :len(tg)], True, {}),
                                       ("bidir:encoder", "encoder", False, dict(noise=noise[:len(tg)], tau=0.7, entropy_weight=1.0))):
            r = m.loss_and_grad(tg, cond, causal, width, "hip", dropout=d, **kw)
            out[f"train:{tag}:grad:{name}"] = torch.cat([r.grads[k].reshape(-1) for k in score_param_names()]).cpu().numpy()
            out[f"train:{tag}:dw:{name}"] = r.dw.cpu().numpy()
            out[f"train:{tag}:loss:{name}"] = np.float64(float(r.loss))
        cg = m.condition_grad(tp, dl[:len(tp)], width, "hip", dropout=d)
        out[f"train:{tag}:condition_grad"] = torch.cat([cg[k].reshape(-1) for k in cg]).cpu().numpy()
    print(f"{tag}: {len(pairs)} pairs, K = {m.K}: done", flush=True)


def run(path):
    import torch
    from dr4sr_amd import _lib
    from dr4sr_amd.regen import NUM_ITEM, RegenModel, random_state_dict, score_param_names
    _lib.load()
    out = {"library": np.array(os.path.relpath(os.path.abspath(_lib.LIB_PATH), ROOT))}
    z = np.load(os.path.join(ROOT, "tests", "golden", "regen_score_toys.npz"))
    sd = {k: torch.from_numpy(z[f"p:{k}"].astype(np.float32)) for k in score_param_names()}
    sd["item_embedding_decoder.weight"] = sd["item_embedding.weight"].clone()
    pairs = json.loads(str(z["pairs_json"]))
    m = RegenModel.from_state_dict(sd, "cuda")
    outputs_of(torch, m, pairs, pairs[:256], (int(z["Ls"]), int(z["T"])), 1, "fixture", out)
    for tag, K, n, seed in (("random_K5", 5, 5000, 9), ("random_K3", 3, 1000, 11)):
        m = RegenModel.from_state_dict(random_state_dict(NUM_ITEM["toy"], K=K, seed=4, std=0.3, condition_encoder=True), "cuda")
        pairs = toys_shaped_pairs(n, m.n_item, seed)
        outputs_of(torch, m, pairs, pairs, None, seed, tag, out)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **out)
    print(f"{len(out) - 1} arrays from {out['library']} -> {path}")


def compare(a_path, b_path, allow_new=False):
    a, b = np.load(a_path), np.load(b_path)
    print(f"A: {a['library']}\nB: {b['library']}")
    keys = sorted((set(a.files) | set(b.files)) - {"library"})
    bad = 0
    for k in keys:
        if allow_new and k not in a.files:
            print(f"new       {k}")
            continue
        if k not in a.files or k not in b.files:
            print(f"MISSING   {k}")
            bad += 1
            continue
        x, y = a[k], b[k]
        same = x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y) and x.tobytes() == y.tobytes()    # the bytes: -0 is not +0
        bad += not same
        note = "" if same else f"  differing entries: {int((x != y).sum()) if x.shape == y.shape else 'shape'}"
        print(f"{'equal    ' if same else 'DIFFERENT'} {k}  {x.dtype}{list(x.shape)}  finite {int(np.isfinite(x).sum())}/{x.size}{note}")
    common = [k for k in keys if k in a.files and k in b.files]
    print(f"{len(common) - bad} of {len(common)} arrays of both files bitwise equal" if allow_new else f"{len(keys) - bad} of {len(keys)} arrays bitwise equal")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--allow-new", action="store_true", help="--compare: arrays only B has are listed as new, not as missing")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare, allow_new=a.allow_new))
    if not a.out:
        ap.error("--out or --compare")
    run(a.out)


if __name__ == "__main__":
    main()
