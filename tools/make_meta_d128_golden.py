#!/usr/bin/env python3
"""Golden fixture of DR4SR+ (MetaModel over SASRec) at embed_dim 128 by RUNNING the reference:
tests/golden/metamodel_sasrec_d128.npz (batches, noise, losses, weights, meta parameters / gradients / hyper-gradient / meta steps)
+ metamodel_sasrec_d128.part<i>.npz (sub-model parameters, inner gradients, validation gradients; each part under the size limit of a
committed file).  tests/_meta_d128.py puts them back together.

The run is tools/make_golden.py's run_meta_case unchanged; the one difference is that the reference's utils.load_config is wrapped so
that every config it returns carries model.embed_dim = 128 (the reference's YAML says 64).  Only DATA is committed.

Usage:  python tools/make_meta_d128_golden.py [--out tests/golden]
"""
import argparse
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

NAME = "metamodel_sasrec_d128"
SEQLENS = [1, 2, 3, 5, 8, 13, 21, 34, 47, 49, 50, 4, 2, 50]          # make_golden.main's list
PART_LIMIT = 900 * 1024                                               # compressed bytes per part, below the 1 MiB file limit
BIG = ("param.", "inner.grad.", "outer.grad_val.")                    # what goes to the parts


def split(arrays, out_dir, name=NAME, big_prefixes=BIG):
    """<name>.npz with the small arrays and meta.n_parts + <name>.part<i>.npz with the arrays whose key starts with one of big_prefixes"""
    small = {k: v for k, v in arrays.items() if not k.startswith(big_prefixes)}
    big = [k for k in arrays if k.startswith(big_prefixes)]
    parts, cur = [], {}

    def size_of(d):
        with tempfile.NamedTemporaryFile(suffix=".npz") as f:
            np.savez_compressed(f, **d)
            f.flush()
            return os.path.getsize(f.name)
    for k in big:                                                     # greedy, in the fixture's own key order
        trial = dict(cur)
        trial[k] = arrays[k]
        if cur and size_of(trial) > PART_LIMIT:
            parts.append(cur)
            cur = {k: arrays[k]}
        else:
            cur = trial
    if cur:
        parts.append(cur)
    small["meta.n_parts"] = np.int64(len(parts))
    files = [(name + ".npz", small)] + [(f"{name}.part{i}.npz", p) for i, p in enumerate(parts)]
    for fn, d in files:
        path = os.path.join(out_dir, fn)
        np.savez_compressed(path, **d)
        kib = os.path.getsize(path) / 1024
        assert kib < 1024, (fn, kib)
        print(f"wrote {path}: {len(d)} arrays, {kib:.0f} KiB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden"))
    args = ap.parse_args()
    out_dir = os.path.abspath(args.out)
    if not os.path.isdir(MG.REF):
        sys.exit("reference not present; golden vectors can only be regenerated in the build container")
    MG._install_stubs()
    sys.path.insert(0, MG.REF)
    import utils as rutils
    orig_load = rutils.load_config

    def load_config_d128(cfg):
        c = orig_load(cfg)
        c["model"]["embed_dim"] = 128
        return c
    rutils.load_config = load_config_d128                             # run_meta_case reads utils.load_config when it starts
    with tempfile.TemporaryDirectory(prefix="dr4sr_meta_d128_") as tmp:
        MG.run_meta_case(tmp, NAME, "SASRec", n_items=151, seqlens=SEQLENS, seed=15)
        z = np.load(os.path.join(tmp, NAME + ".npz"))
        arrays = {k: z[k] for k in z.files}
    assert arrays["meta_param.0.weight"].shape == (128, 128) and arrays["param.item_embedding.weight"].shape[1] == 128
    split(arrays, out_dir)


if __name__ == "__main__":
    main()
