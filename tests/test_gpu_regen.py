"""Dataset regeneration on the MI355X (csrc/regen.hip through dr4sr_regen_encode / dr4sr_regen_decode): tokens against the reference's
(tests/golden/regen_toys.npz) and against the batched torch restatement, batch independence, argument errors, and the whole stage 3
-> SASRec training path."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from test_regen_cpu import load_fixture, tokens_agree

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _synthetic_sources(n, n_item, seed):
    g = np.random.default_rng(seed)
    lens = np.minimum(g.geometric(1 / 9.0, n), 47)            # toys-like: mean ~9 items, a few up to 47 (len(src) up to 50)
    lens[:3] = [1, 47, 24]
    return [[n_item] + g.integers(1, n_item, int(l) + 1).tolist() + [n_item + 1] for l in lens]


def test_hip_matches_reference_tokens():
    from dr4sr_amd.regen import RegenModel
    z, sd, train, src, ref = load_fixture()
    m = RegenModel.from_state_dict(sd, "cuda")
    got = m.decode(src, backend="hip")
    bad = [i for i in range(len(ref)) if not tokens_agree(got[i], ref[i], z["gaps"][i], z["top"][i])]
    assert not bad, [(i, got[i], ref[i]) for i in bad[:3]]
    assert [t.tolist() for t in m.translate(src[:5], 4)] == got[4 * len(src):4 * len(src) + 5]


def test_hip_matches_torch_on_toys_shaped_rows():
    from dr4sr_amd.regen import RegenModel, random_state_dict
    m = RegenModel.from_state_dict(random_state_dict(seed=3, std=0.3), "cuda")
    src = _synthetic_sources(2000, m.n_item, 7)
    hip = m.decode(src, backend="hip")
    ref, gaps, tops = m.decode_with_gaps(src)
    assert len(hip) == len(ref) == 5 * 2000
    bad = [i for i in range(len(ref)) if not tokens_agree(hip[i], ref[i], gaps[i].numpy(), tops[i].numpy())]
    assert not bad, [(i, hip[i], ref[i]) for i in bad[:3]]
    same = sum(a == b for a, b in zip(hip, ref))
    assert same >= 0.99 * len(ref), same
    assert {2, 3, 25} <= {len(t) for t in hip}                    # EOS at step 0, at step 1, and rows that never stop


def test_decode_is_independent_of_the_batch():
    from dr4sr_amd.regen import RegenModel, random_state_dict
    m = RegenModel.from_state_dict(random_state_dict(seed=5, std=0.3), "cuda")
    src = _synthetic_sources(4096, m.n_item, 11)
    big = m.decode(src, 1, 1, "hip")                              # 4 096 rows in one call
    again = m.decode(src, 1, 1, "hip")
    assert big == again
    for i in (0, 1, 2, 777, 4095):
        assert m.decode([src[i]], 1, 1, "hip")[0] == big[i], i
    allc = m.decode(src[:300], backend="hip")                     # all 5 conditions of the first 300: condition 1 is rows 300..599
    assert allc[300:600] == big[:300]


def test_argument_errors_and_workspace_size():
    from dr4sr_amd import _lib
    from dr4sr_amd.regen import RegenModel, random_state_dict
    lib = _lib.load()
    m = RegenModel.from_state_dict(random_state_dict(200, K=2, seed=0), "cuda")
    p = m.plan()
    per_row = (2 * 50 * 128 + 2 * 25 * 128 + 64) * 4 + 12
    nb = lib.dr4sr_regen_workspace_bytes(C.byref(p), 3, 2)
    assert nb == 6 * per_row
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    src = torch.full((3, 51), 1, dtype=torch.int64, device="cuda")
    ln = torch.full((3,), 5, dtype=torch.int64, device="cuda")
    tok = torch.empty(6, 25, dtype=torch.int64, device="cuda")
    n = torch.empty(6, dtype=torch.int32, device="cuda")
    st = _lib.cur_stream()
    args = (_lib.ptr(src), _lib.ptr(ln), 3)
    wsp = C.c_void_p(ws.data_ptr())
    assert lib.dr4sr_regen_encode(C.byref(p), *args, 51, 0, 2, wsp, nb, st) == -2
    assert lib.dr4sr_regen_encode(C.byref(p), *args, 50, 0, 2, wsp, nb - 1, st) == -3
    assert lib.dr4sr_regen_encode(C.byref(p), *args, 50, 1, 2, wsp, nb, st) == -1
    assert lib.dr4sr_regen_decode(C.byref(p), *args, 50, 0, 2, wsp, nb, None, _lib.ptr(n), st) == -1
    assert lib.dr4sr_regen_encode(C.byref(p), *args, 50, 0, 2, wsp, nb, st) == 0
    assert lib.dr4sr_regen_decode(C.byref(p), *args, 50, 0, 2, wsp, nb, _lib.ptr(tok), _lib.ptr(n), st) == 0
    torch.cuda.synchronize()
    assert ((n >= 2) & (n <= 25)).all() and (tok[:, 0] == 200).all()
    with pytest.raises(ValueError, match="position table"):
        m.decode([[200] + [1] * 49 + [201]], backend="hip")


def test_regenerated_dataset_trains_sasrec(tmp_path, monkeypatch):
    """stage 3 end to end: hybrid_inference writes train_regen.pth; the SeparateDataset of `train_file: '_regen'` loads it and one
    SASRec epoch trains on it"""
    from dr4sr_amd.regen import hybrid_inference, random_state_dict
    from dr4sr_amd.utils import load_config, prepare_datasets, prepare_model, seed_everything
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("DR4SR_CONFIG_DIR", os.path.join(ROOT, "configs"))
    n_item = 300
    d = tmp_path / "dataset" / "tiny" / "tinyd"
    d.mkdir(parents=True)
    rng = np.random.default_rng(2)
    pad = lambda s: list(s) + [0] * (50 - len(s))
    train, val = [], []
    for u in range(1, 201):
        sl = int(rng.integers(1, 30))
        full = rng.integers(1, n_item, sl + 2).tolist()
        train.append([u, pad(full[:sl]), pad(full[1:sl + 1]), sl, [1] * 50, [0] * 50])
        val.append([u, pad(full[:sl]), full[sl], sl, 1, [0] * 50, pad(full[:sl])])
    torch.save(train, d / "train.pth")
    torch.save(train[:20], d / "patterns.pth")
    torch.save(val, d / "val.pth")
    torch.save(val, d / "test.pth")
    with open(d / "inter.csv", "w") as f:
        f.write("user_id,item_id,rating,timestamp,domain\n")
        for i in range(1, n_item):
            f.write(f"{(i - 1) % 200 + 1},{i},1.0,{i},0\n")
    torch.save(random_state_dict(n_item, K=5, seed=9, std=0.3), d / "regenerator.pth")
    out = hybrid_inference("dataset/tiny/tinyd/")
    rows = torch.load(out)
    assert len(rows) > 220 and rows[:200] == train
    cfg = load_config({"model": "SASRec", "dataset": "amazon-toys"})
    cfg["data"].update({"dataset": "tiny", "domain_name_list": ["tinyd"], "train_file": "_regen"})
    cfg["train"].update({"batch_size": 64, "epochs": 1, "device": "cuda"})
    seed_everything(cfg["train"]["seed"])
    ds = prepare_datasets(cfg)
    assert len(ds[0]) == len(rows)
    model = prepare_model(cfg, ds)
    model._init_model(ds[0])
    model.train()
    out = model.training_epoch(0)
    loss = [float(o["loss_0"].float().mean() if torch.is_tensor(o["loss_0"]) else o["loss_0"]) for o in out[0]]
    assert len(loss) >= 1 and np.isfinite(loss).all()
