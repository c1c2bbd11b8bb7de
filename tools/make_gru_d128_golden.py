#!/usr/bin/env python3
"""Golden fixture of GRU4Rec at embed_dim 128 by RUNNING the reference: tests/golden/gru4rec_d128.npz (batches, outputs, meta and the
number of parts) + gru4rec_d128.part<i>.npz (parameters, gradients, parameters after one Adam step; each part under the size limit of a
committed file).  tests/_gru_d128.py puts them back together.

The run is tools/make_golden.py's run_case unchanged: the d64 case's ten sequence lengths, hidden 128 (configs/gru4rec.yaml's 256 only
makes the fixture larger), a seed of its own.  Only DATA is committed.

Usage:  python tools/make_gru_d128_golden.py [--out tests/golden]
"""
import argparse
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402
from make_meta_d128_golden import split  # noqa: E402  (the same split into files under the size limit)

NAME = "gru4rec_d128"
SEQLENS = [1, 2, 3, 5, 8, 13, 21, 34, 47, 49]                         # make_golden.main's seqlens[:10], the gru4rec_d64 case
SEED = 33
BIG = ("param.", "grad.", "adam1.")                                   # what goes to the parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden"))
    args = ap.parse_args()
    out_dir = os.path.abspath(args.out)
    if not os.path.isdir(MG.REF):
        sys.exit("reference not present; golden vectors can only be regenerated in the build container")
    MG._install_stubs()
    sys.path.insert(0, MG.REF)
    with tempfile.TemporaryDirectory(prefix="dr4sr_gru_d128_") as tmp:
        MG.run_case(tmp, NAME, "GRU4Rec", n_items=131, seqlens=SEQLENS, embed_dim=128, seed=SEED,
                    overrides={"model": {"hidden_size": 128}})
        z = np.load(os.path.join(tmp, NAME + ".npz"))
        arrays = {k: z[k] for k in z.files}
    assert arrays["param.item_embedding.weight"].shape[1] == 128 and arrays["param.query_encoder.1.weight"].shape == (128, 128)
    split(arrays, out_dir, NAME, BIG)


if __name__ == "__main__":
    main()
