"""Dataset regeneration (dr4sr_amd.regen, DR4SR stage 3) without a GPU: the batched torch restatement against tokens the reference's
3.Hybrid_inference.py decoded (tests/golden/regen_toys.npz, tools/make_regen_golden.py), the train_regen.pth writer against the
reference's file, state-dict loading, and the C ABI's host-side checks."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "regen_toys.npz")


def load_fixture():
    from dr4sr_amd.regen import param_names, source_rows
    z = np.load(GOLD)
    sd = {k: torch.from_numpy(z[f"p:{k}"].astype(np.float32)) for k in param_names()}
    sd["item_embedding_decoder.weight"] = sd["item_embedding.weight"].clone()
    train = json.loads(str(z["train_json"]))
    n_item = int(z["n_item"])
    src = [[n_item] + s + [n_item + 1] for s in source_rows(train)]
    ref = [list(map(int, t[:n])) for t, n in zip(z["tokens"], z["token_len"])]
    return z, sd, train, src, ref


def tokens_agree(got, ref, gaps, tops, tol=1e-4):
    """the gap rule: got matches ref up to (not including) the first step whose best and second-best allowed logits were within
    tol * max(1, |best|) — a near-tie that rounding may legitimately break either way; with no such step, completely"""
    amb = None
    for s, (g, t) in enumerate(zip(gaps, tops)):
        if np.isnan(g):
            break
        if g < tol * max(1.0, abs(float(t))):
            amb = s
            break
    if amb is None:
        return list(got) == list(ref)
    return list(got[:amb + 1]) == list(ref[:amb + 1])


def test_torch_restatement_matches_reference_tokens():
    from dr4sr_amd.regen import RegenModel
    z, sd, train, src, ref = load_fixture()
    m = RegenModel.from_state_dict(sd, "cpu")
    assert m.K == int(z["K"]) and m.n_item == int(z["n_item"])
    got = m.decode(src, backend="torch")
    assert len(got) == len(ref) == m.K * len(src)
    bad = [i for i in range(len(ref)) if not tokens_agree(got[i], ref[i], z["gaps"][i], z["top"][i])]
    assert not bad, [(i, got[i], ref[i]) for i in bad[:3]]
    # the fixture covers the three endings: EOS at step 0, EOS after one or two items, 24 items without EOS
    eos = m.eos
    assert any(t == [m.sos, eos] for t in ref)
    assert any(3 <= len(t) <= 4 and t[-1] == eos for t in ref)
    assert any(len(t) == 25 and t[-1] != eos for t in ref)
    assert max(len(s) for s in src) == 50
    # translate() returns what the reference's translate returns: one int64 tensor per source
    one = m.translate(src[:3], condition=2, backend="torch")
    assert [t.tolist() for t in one] == got[2 * len(src):2 * len(src) + 3] and one[0].dtype == torch.int64


def test_writer_reproduces_reference_train_regen():
    from dr4sr_amd.regen import regen_rows
    z, sd, train, src, ref = load_fixture()
    patterns = json.loads(str(z["patterns_json"]))
    want = json.loads(str(z["regen_json"]))
    got = json.loads(json.dumps(train + patterns + regen_rows(ref)))
    assert len(got) == len(want) and got == want


def test_hybrid_inference_writes_the_reference_layout(tmp_path):
    """hybrid_inference end to end on the CPU restatement: train.pth + patterns.pth + regenerator.pth -> train_regen.pth"""
    from dr4sr_amd.regen import hybrid_inference, random_state_dict, RegenModel, regen_rows, source_rows
    root = tmp_path / "dataset" / "tiny" / "tinyd"
    root.mkdir(parents=True)
    n_item = 60
    rng = np.random.default_rng(1)
    train = []
    for u, sl in enumerate([1, 2, 5, 9, 47, 3], 1):
        it = rng.integers(1, n_item, sl + 1).tolist()
        train.append([u, it[:sl] + [0] * (50 - sl), it[1:] + [0] * (50 - sl), sl, [1] * 50, [0] * 50])
    pats = [[0, [3, 4] + [0] * 48, [4, 5] + [0] * 48, 2, [1, 1] + [0] * 48, [0] * 50]]
    torch.save(train, root / "train.pth")
    torch.save(pats, root / "patterns.pth")
    sd = random_state_dict(n_item, K=3, seed=4, std=0.3)
    torch.save(sd, root / "regenerator.pth")
    out = hybrid_inference(str(root) + "/", backend="torch", device="cpu")
    rows = torch.load(out)
    m = RegenModel.from_state_dict(sd, "cpu")
    toks = m.decode([[m.sos] + s + [m.eos] for s in source_rows(train)], backend="torch")
    assert rows == train + pats + regen_rows(toks)
    assert len(rows) > len(train) + len(pats)
    for r in rows[len(train) + len(pats):]:
        assert r[0] == 1 and len(r[1]) == len(r[2]) == 50 and 1 <= r[3] <= 50 and r[4] == [1] * 50 and r[5] == [0] * 50
    # --begin / --end keep the reference's begin*5000 : end*5000 slice
    out = hybrid_inference(str(root) + "/", backend="torch", device="cpu", begin=1, out_name="train_regen_b1.pth")
    assert torch.load(out) == train + pats


def test_state_dict_loading_and_refusals():
    from dr4sr_amd.regen import RegenModel, random_state_dict
    sd = random_state_dict(30, K=3, seed=0)
    sd["condition_encoder.condition_layer.2.weight"] = torch.zeros(3, 64)        # ignored at inference
    m = RegenModel.from_state_dict(sd, "cpu")
    assert (m.K, m.n_item, m.sos, m.eos, m.n_rows) == (3, 30, 30, 31, 32)
    assert RegenModel.from_state_dict(random_state_dict(30, K=5), "cpu").K == 5
    bad = dict(sd)
    bad["item_embedding_decoder.weight"] = sd["item_embedding.weight"] + 1
    with pytest.raises(ValueError, match="item_embedding_decoder"):
        RegenModel.from_state_dict(bad, "cpu")
    with pytest.raises(ValueError, match="dataset 'toy'"):
        RegenModel.from_state_dict(sd, "cpu", dataset="toy")
    bad = dict(sd)
    del bad["transformer.decoder.norm.weight"]
    with pytest.raises(ValueError, match="transformer.decoder.norm.weight"):
        RegenModel.from_state_dict(bad, "cpu")
    # len(src) > 50: the reference's position table has 50 rows
    with pytest.raises(ValueError, match="position table"):
        m.decode([[30] + [1] * 49 + [31]], backend="torch")
    assert len(m.decode([[30] + [1] * 48 + [31]], backend="torch")) == 3
    with pytest.raises(ValueError, match="backend"):
        m.decode([[30, 1, 31]], backend="eager")
    with pytest.raises(ValueError, match="conditions"):
        m.decode([[30, 1, 31]], cond0=2, n_cond=2, backend="torch")


def test_lib_binds_regen_entry_points():
    from dr4sr_amd import _lib
    from dr4sr_amd.regen import param_names, param_shapes
    lib = _lib.load()
    assert lib.dr4sr_regen_plan_sizeof() == C.sizeof(_lib.RegenPlan)
    off = (C.c_int64 * _lib.REGEN_TENSORS)()
    n = lib.dr4sr_regen_param_layout(11927, 5, off)
    sizes = [int(np.prod(s)) for s in param_shapes(11927, 5)]
    assert len(param_names()) == _lib.REGEN_TENSORS and n == sum(sizes)
    assert list(off) == list(np.cumsum([0] + sizes[:-1]))
    assert lib.dr4sr_regen_param_layout(2, 5, None) == -1
    p = _lib.RegenPlan()
    p.abi_version, p.n_rows, p.K, p.max_len, p.D, p.H, p.F, p.n_layer, p.ln_eps = _lib.ABI_VERSION, 11927, 5, 25, 64, 2, 256, 2, 1e-12
    p.params, p.n_params = 4096, n                                   # never dereferenced by the host-side checks
    per_row = (2 * 50 * 128 + 2 * 25 * 128 + 64) * 4 + 12
    assert lib.dr4sr_regen_workspace_bytes(C.byref(p), 100, 5) == 500 * per_row
    ws = C.c_void_p(8192)
    assert lib.dr4sr_regen_encode(C.byref(p), C.c_void_p(64), C.c_void_p(64), 4, 51, 0, 5, ws, 1 << 40, None) == -2   # len(src) > 50
    assert lib.dr4sr_regen_encode(C.byref(p), C.c_void_p(64), C.c_void_p(64), 4, 50, 3, 3, ws, 1 << 40, None) == -1   # conditions > K
    assert lib.dr4sr_regen_encode(C.byref(p), C.c_void_p(64), C.c_void_p(64), 4, 50, 0, 5, ws, 20 * per_row - 1, None) == -3
    assert lib.dr4sr_regen_decode(C.byref(p), C.c_void_p(64), C.c_void_p(64), 4, 50, 0, 5, ws, 20 * per_row, None, None, None) == -1
    for field, val in (("D", 128), ("H", 4), ("F", 128), ("n_layer", 3), ("max_len", 26)):
        q = _lib.RegenPlan.from_buffer_copy(p)
        setattr(q, field, val)
        assert lib.dr4sr_regen_workspace_bytes(C.byref(q), 10, 1) == -2, field
    q = _lib.RegenPlan.from_buffer_copy(p)
    q.abi_version = 8
    assert lib.dr4sr_regen_workspace_bytes(C.byref(q), 10, 1) == -1
    q = _lib.RegenPlan.from_buffer_copy(p)
    q.n_params = n - 1
    assert lib.dr4sr_regen_workspace_bytes(C.byref(q), 10, 1) == -1
