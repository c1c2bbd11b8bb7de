"""Loader of the GRU4Rec d = 128 fixture (tools/make_gru_d128_golden.py): tests/golden/gru4rec_d128.npz holds the batches, outputs, meta
values and the number of parts, gru4rec_d128.part<i>.npz the parameters, gradients and parameters after one Adam step."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAME = "gru4rec_d128"


@functools.lru_cache(maxsize=1)
def load():
    """one dict of every array of the fixture (read once per session; callers must not write into the arrays)"""
    z = np.load(os.path.join(GOLDEN, NAME + ".npz"))
    g = {k: z[k] for k in z.files}
    for i in range(int(g["meta.n_parts"])):
        p = np.load(os.path.join(GOLDEN, f"{NAME}.part{i}.npz"))
        g.update({k: p[k] for k in p.files})
    return g
