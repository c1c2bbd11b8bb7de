#!/usr/bin/env python3
"""Golden fixture of dataset regeneration (tests/golden/regen_toys.npz) by RUNNING the reference's stage 2 and stage 3 scripts.

Works only where the reference checkout (USTC-StarTeam/DR4SR) exists.  The scripts' text is exec'd unmodified apart from two
in-memory substitutions: 'cuda' -> 'cpu', and the item count of 'toy' in their num_item_dict -> N_ITEM, so that the fixture's item
table (and with it the committed file) stays small; the model code is untouched.  Only DATA is written.

  1. 2.Pretrain_regenerator.py --root_path <tmp>/toy --epochs E on ~1 000 synthetic sequence-pattern pairs, with the first N_ITEM
     rows of the shipped toys pre-trained_embedding.ckpt as its item table.
  2. The saved regenerator is rounded to fp16-representable fp32 values (so that it can be stored in fp16 without changing the model
     that stage 3 decodes with) and written back.
  3. 3.Hybrid_inference.py --root_path <tmp>/toy/ on a toys-format train.pth of 56 rows with seqlens 1..47 (len(src) up to 50) and a
     small patterns.pth.  translate() is wrapped to record every decoded token sequence, inference_mask / inference_mask_generative
     to record at every step the gap between the best and the second-best ALLOWED logit.
  4. Stored: the state dict (fp16, item table once), the source rows, the tokens per (condition, sequence), the per-step gaps and top
     logits, and the train.pth / patterns.pth / train_regen.pth row lists (JSON text).

Usage:  python tools/make_regen_golden.py [--out tests/golden/regen_toys.npz] [--epochs 15]
"""
import argparse
import json
import os
import random
import sys
import tempfile
import textwrap

import numpy as np

REF = "/root/reference"
N_ITEM = 1000
L = 50
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def _run_script(name, argv, wrap=None):
    text = open(os.path.join(REF, name)).read().replace("'cuda'", "'cpu'").replace("'toy': 11925", f"'toy': {N_ITEM}")
    head, body = text.split("if __name__ == '__main__':", 1)
    g = {"__name__": "regen_reference", "__file__": os.path.join(REF, name)}
    sys.argv = [name] + argv
    exec(compile(head, name, "exec"), g)
    if wrap:
        wrap(g)
    exec(compile(textwrap.dedent(body), name, "exec"), g)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "tests", "golden", "regen_toys.npz"))
    ap.add_argument("--epochs", type=int, default=15)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from make_golden import _install_stubs
    _install_stubs()
    sys.path.insert(0, REF)
    import torch
    rng = random.Random(a.seed)
    tmp = tempfile.mkdtemp(prefix="regen_golden_")
    root = os.path.join(tmp, "toy")
    os.makedirs(root)
    cwd = os.getcwd()
    os.chdir(REF)
    try:
        E = torch.load(os.path.join(REF, "dataset/amazon-toys/toy/pre-trained_embedding.ckpt"), map_location="cpu")
        E = E["parameters"]["item_embedding.weight"][:N_ITEM].clone()
        torch.save({"parameters": {"item_embedding.weight": E}}, os.path.join(root, "pre-trained_embedding.ckpt"))
        # ---- stage 2 data: sequences over a few "topics" so that patterns are learnable
        pairs = []
        topics = [rng.sample(range(1, N_ITEM), 40) for _ in range(12)]
        for _ in range(1000):
            tp = rng.choice(topics)
            seq = [rng.choice(tp) for _ in range(rng.randint(3, 20))]
            k = rng.randint(1, min(5, len(seq)))
            pos = sorted(rng.sample(range(len(seq)), k))
            pairs.append([seq, [seq[p] for p in pos]])
        torch.save(pairs, os.path.join(root, "seq-pat-pair.pth"))
        _run_script("2.Pretrain_regenerator.py", ["--root_path", root, "--epochs", str(a.epochs)])
        sd = torch.load(os.path.join(root, "regenerator.pth"), map_location="cpu")
        sd = {k: (v.half().float() if v.is_floating_point() else v) for k, v in sd.items()}
        torch.save(sd, os.path.join(root, "regenerator.pth"))
        # ---- stage 3 data: toys-format rows [user, hist[50], target[50], seqlen, label[50], domain[50]]
        seqlens = list(range(1, 48)) + [1, 2, 3, 5, 8, 13, 21, 34, 47]
        train = []
        for u, sl in enumerate(seqlens):
            tp = rng.choice(topics)
            items = [rng.choice(tp) if rng.random() < 0.8 else rng.randint(1, N_ITEM - 1) for _ in range(sl + 1)]
            hist, tgt = items[:sl], items[1:sl + 1]
            train.append([u + 1, hist + [0] * (L - sl), tgt + [0] * (L - sl), sl, [1] * L, [0] * L])
        torch.save(train, os.path.join(root, "train.pth"))
        pats = []
        for _ in range(6):
            p = rng.sample(rng.choice(topics), rng.randint(2, 5))
            sl = len(p) - 1
            pats.append([0, tuple(p[:-1] + [0] * (L - sl)), tuple(p[1:] + [0] * (L - sl)), sl, [1] * sl + [0] * (L - sl), [0] * L])
        torch.save(pats, os.path.join(root, "patterns.pth"))
        rec = {"tokens": [], "gaps": [], "top": []}
        cur = {}

        def wrap(g):
            tr, im, img = g["translate"], g["inference_mask"], g["inference_mask_generative"]

            def gap_of(logits):
                v = torch.topk(logits.reshape(-1), 2).values
                cur.setdefault("gaps", []).append(float(v[0] - v[1]))
                cur.setdefault("top", []).append(float(v[0]))
                return logits

            g["inference_mask"] = lambda lg, s, y: gap_of(im(lg, s, y))
            g["inference_mask_generative"] = lambda lg, s, y: gap_of(img(lg, s, y))

            def translate(model, src):
                cur.clear()
                out = tr(model, src)
                rec["tokens"].append(out.tolist())
                rec["gaps"].append(list(cur.get("gaps", [])))
                rec["top"].append(list(cur.get("top", [])))
                return out
            g["translate"] = translate

        g3 = _run_script("3.Hybrid_inference.py", ["--root_path", root + "/"], wrap)
        K = g3["K"]
        regen = torch.load(os.path.join(root, "train_regen.pth"))
    finally:
        os.chdir(cwd)
    sys.path.insert(0, os.path.dirname(HERE))
    from dr4sr_amd.regen import param_names
    n = len(train)
    assert len(rec["tokens"]) == K * n
    lens = [len(t) for t in rec["tokens"]]
    ends = {"eos_at_step0": sum(t == [N_ITEM, N_ITEM + 1] for t in rec["tokens"]),
            "eos_after_1_2": sum(3 <= len(t) <= 4 and t[-1] == N_ITEM + 1 for t in rec["tokens"]),
            "no_eos_24": sum(len(t) == 25 and t[-1] != N_ITEM + 1 for t in rec["tokens"])}
    print("endings:", ends, "lengths:", sorted(set(lens)))
    tok = np.full((K * n, 25), -1, np.int64)
    gaps = np.full((K * n, 24), np.nan, np.float32)
    top = np.full((K * n, 24), np.nan, np.float32)
    for i, t in enumerate(rec["tokens"]):
        tok[i, :len(t)] = t
        gaps[i, :len(rec["gaps"][i])] = rec["gaps"][i]
        top[i, :len(rec["top"][i])] = rec["top"][i]
    out = {f"p:{k}": sd[k].numpy().astype(np.float16) for k in param_names()}
    for k in param_names():
        assert np.array_equal(out[f"p:{k}"].astype(np.float32), sd[k].numpy()), k
    out.update(tokens=tok, token_len=np.array(lens, np.int32), gaps=gaps, top=top, K=np.int32(K), n_item=np.int32(N_ITEM),
               train_json=np.array(json.dumps(train)), patterns_json=np.array(json.dumps([list(map(lambda x: list(x) if isinstance(x, tuple) else x, r)) for r in pats])),
               regen_json=np.array(json.dumps([[list(x) if isinstance(x, tuple) else x for x in r] for r in regen])),
               endings=np.array(json.dumps(ends)))
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
