"""Teacher-forced scoring of the regenerator (RegenModel.score, DR4SR stage 2's forward and loss) without a GPU: the torch restatement
against per-token NLLs and condition logits that the reference's 2.Pretrain_regenerator.py computed (tests/golden/regen_score_toys.npz,
tools/make_regen_score_golden.py), the matrix-width rules, the C ABI's layout and host-side checks, state dicts without a
condition_encoder, and the --score CLI.

Tolerances: err32 (stored in the fixture per mode and quantity) is max |reference fp32 - float64| over the finite values, the
reference's own rounding noise.  A second fp32 evaluation in another summation order may sit 4 x err32 from the float64 result; a
wrong mask, a missing norm or the pooling rule moves an NLL by 1e-2 or more."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "regen_score_toys.npz")
MODES = ("gumbel", "onehot", "softmax")


def load_score_fixture():
    from dr4sr_amd.regen import score_param_names
    z = np.load(GOLD)
    sd = {k: torch.from_numpy(z[f"p:{k}"].astype(np.float32)) for k in score_param_names()}
    sd["item_embedding_decoder.weight"] = sd["item_embedding.weight"].clone()
    return z, sd, json.loads(str(z["pairs_json"])), json.loads(str(z["err32"])), (int(z["Ls"]), int(z["T"]))


def conditions_of(z, mode, ci):
    """what RegenModel.score takes as `conditions` to replay the fixture's mode under source mask ci (0 causal, 1 bidirectional)"""
    return {"gumbel": torch.from_numpy(z["w_gumbel"][ci])[None], "onehot": "all", "softmax": "encoder"}[mode]


def reference_of(z, mode, ci):
    ref = torch.from_numpy(z[f"nll_{mode}"][ci])
    return ref if mode == "onehot" else ref[None]


def check_close(got, want, bound, what, n_expected=None, unit=None):
    """every entry compared: +inf in the same places and nowhere else, the finite ones within `bound`; returns the worst difference"""
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if n_expected is not None:
        assert got.numel() == n_expected, (what, got.numel(), n_expected)
    assert not torch.isnan(got).any() and not (got == float("-inf")).any(), what
    assert torch.equal(torch.isinf(got), torch.isinf(want)), what
    fin = torch.isfinite(want)
    worst = float((got - want)[fin].abs().max())
    print(f"{what}: max |diff| {worst:.3e}, bound {bound:.3e}" + (f", {worst / unit:.2f} x err32" if unit else ""))
    assert worst <= bound, (what, worst, bound)
    return worst


def test_torch_fp32_matches_reference_in_all_six_modes():
    from dr4sr_amd.regen import RegenModel
    z, sd, pairs, err32, width = load_score_fixture()
    m = RegenModel.from_state_dict(sd, "cpu")
    assert m.has_condition_encoder and m.K == int(z["K"]) == 5
    n, T = len(pairs), width[1]
    seen = 0
    for ci, causal in enumerate((True, False)):
        tag = "causal" if causal else "bidir"
        for mode in MODES:
            cond = conditions_of(z, mode, ci)
            ref = reference_of(z, mode, ci)
            r32 = m.score(pairs, cond, causal, width, "torch")
            r64 = m.score(pairs, cond, causal, width, "torch", torch.float64)
            e = err32[f"nll_{mode}_{tag}"]
            check_close(r64.nll, ref, e * (1 + 1e-6), f"float64 vs reference {mode} {tag}", ref.numel())
            check_close(r32.nll, r64.nll, 4 * e, f"fp32 vs float64 {mode} {tag}", ref.numel())
            check_close(r32.nll, ref, 4 * e, f"fp32 vs reference {mode} {tag}", ref.numel())
            check_close(r32.cond_logits, r64.cond_logits, 4 * err32["cond_logits"], f"condition logits vs float64 {mode} {tag}", n * 5)
            check_close(r32.cond_logits, z["cond_logits"], 4 * err32["cond_logits"], f"condition logits vs reference {mode} {tag}", n * 5)
            assert int(torch.isinf(ref).sum()) == 3 * ref.shape[0]            # the three targets with an id outside their source
            assert torch.equal(r32.n_tok, torch.tensor([len(t) + 1 for _, t in pairs]))
            assert torch.equal(r32.nll == 0, torch.from_numpy(z[f"nll_{mode}"][ci] == 0).reshape(r32.nll.shape))
            seen += ref.numel()
    assert seen == 2 * (1 + 5 + 1) * n * T                                    # no stored token left out
    # loss() is the reference's CrossEntropyLoss(ignore_index=0) over the stored 256-pair batch
    nb = int(z["loss_batch_n"])
    got = m.score(pairs[:nb], "encoder", True, width, "torch").loss()
    assert got.shape == (1,) and abs(float(got[0]) - float(z["loss_batch"])) <= 4 * err32["nll_softmax_causal"]


def test_census_of_the_fixture():
    z, sd, pairs, err32, (Ls, T) = load_score_fixture()
    assert (Ls, T) == (50, 19) and 250 <= len(pairs) <= 350
    lens = {len(t) for _, t in pairs}
    assert min(lens) == 1 and sum(len(t) + 2 == T + 1 for _, t in pairs) >= 2          # rows whose EOS is cut from tgt_in
    assert any(len(s) + 2 == 50 for s, _ in pairs)
    assert any(len(set(s)) < len(s) for s, _ in pairs) and any(len(set(t)) < len(t) for _, t in pairs)
    assert sum(any(v not in s for v in t) for s, t in pairs) == 3
    assert all(0 < e < 1e-4 for k, e in err32.items()), err32                # the reference's noise: far below any structural error


def test_width_is_honoured():
    from dr4sr_amd.regen import RegenModel
    z, sd, pairs, err32, (Ls, T) = load_score_fixture()
    m = RegenModel.from_state_dict(sd, "cpu")
    full = m.score(pairs, "all", True, (Ls, T), "torch")
    e = 4 * err32["nll_onehot_causal"]
    short = next(i for i, (s, t) in enumerate(pairs) if len(t) == 2 and len(s) < 20)
    one = m.score([pairs[short]], "all", True, (Ls, T), "torch")             # a short row alone at the file's widths: its value in the file
    check_close(one.nll[:, 0], full.nll[:, short], e, "short row alone, width=(Ls, T)")
    check_close(one.cond_logits[0], full.cond_logits[short], 4 * err32["cond_logits"], "short row's condition logits, width=(Ls, T)")
    # Without width= the widths come from the given pairs.  The target side never depends on them (T only adds pad columns): the
    # condition logits are the file's.  The NLL is the file's when the source fills the file's Ls (the 50-id source here) ...
    long_src = next(i for i, (s, t) in enumerate(pairs) if len(s) + 2 == Ls)
    one = m.score([pairs[long_src]], "all", True, None, "torch")
    assert one.width == (Ls, T)
    check_close(one.nll[:, 0], full.nll[:, long_src], e, "row with a full-width source alone, no width=")
    check_close(one.cond_logits[0], full.cond_logits[long_src], 4 * err32["cond_logits"], "its condition logits")
    # ... and for a shorter source it is what the reference gives for a one-pair file: the row is then not padded, so PAD 0 is not
    # among the ids the softmax runs over (condition_mask scatters the padded row), and every NLL is smaller by log(1 - p(PAD))
    one = m.score([pairs[short]], "all", True, None, "torch")
    assert one.width == (len(pairs[short][0]) + 2, T)
    check_close(one.cond_logits[0], full.cond_logits[short], 4 * err32["cond_logits"], "short row's condition logits, no width=")
    live = full.nll[:, short] != 0
    drop = (full.nll[:, short] - one.nll[:, 0])[live]
    assert torch.equal(one.nll[:, 0] != 0, live) and float(drop.min()) > 0 and float(drop.max()) < 0.5, drop
    wide = [int(i) for i in z["wide_idx"]]
    assert len(wide) >= 2 and all(len(pairs[i][1]) + 2 == T + 1 for i in wide)
    w = m.score([pairs[i] for i in wide], "all", True, (Ls, T + 1), "torch")
    assert w.nll.shape == (5, len(wide), T + 1) and float(w.nll[:, :, T].abs().max()) == 0.0
    check_close(w.nll, z["wide_nll"], 4 * err32["wide_nll"], "rows that fill the width, one column wider: NLL vs reference")
    check_close(w.nll[:, :, :T], full.nll[:, wide], e, "rows that fill the width: NLL does not depend on the width")
    check_close(w.cond_logits, z["wide_cond"], 4 * err32["wide_cond"], "their condition logits, EOS pooled, vs reference")
    moved = (w.cond_logits - full.cond_logits[wide]).abs().max()
    assert float(moved) > 1000 * err32["cond_logits"], float(moved)              # the EOS column changes what is pooled
    with pytest.raises(ValueError, match="narrower"):
        m.score([pairs[wide[0]]], "all", True, (Ls, T - 1), "torch")
    with pytest.raises(ValueError, match="position table"):
        m.score(pairs[:2], "all", True, (51, T), "torch")


def test_layout_workspace_and_argument_errors():
    from dr4sr_amd import _lib
    from dr4sr_amd.regen import param_shapes, score_param_names, score_param_shapes
    lib = _lib.load()
    assert lib.dr4sr_abi_version() == 10 == _lib.ABI_VERSION
    assert _lib.REGEN_SCORE_TENSORS == 98 == len(score_param_names()) and _lib.REGEN_TENSORS == 70
    off = (C.c_int64 * 98)()
    old = (C.c_int64 * 70)()
    n = lib.dr4sr_regen_score_param_layout(11927, 5, off)
    n_old = lib.dr4sr_regen_param_layout(11927, 5, old)
    sizes = [int(np.prod(s)) for s in score_param_shapes(11927, 5)]
    assert n == sum(sizes) and list(off) == list(np.cumsum([0] + sizes[:-1]))
    assert list(off[:70]) == list(old) and off[70] == n_old == sum(int(np.prod(s)) for s in param_shapes(11927, 5))
    assert score_param_names()[70] == "condition_encoder.encoder.layers.0.self_attn.in_proj_weight"
    assert score_param_names()[94:] == [f"condition_encoder.condition_layer.{i}.{x}" for i in (0, 2) for x in ("weight", "bias")]
    assert lib.dr4sr_regen_score_param_layout(2, 5, None) == -1 and lib.dr4sr_regen_score_param_layout(10, 0, None) == -1
    p = _lib.RegenPlan()
    p.abi_version, p.n_rows, p.K, p.max_len, p.D, p.H, p.F, p.n_layer, p.ln_eps = 10, 11927, 5, 25, 64, 2, 256, 2, 1e-12
    p.params, p.n_params = 4096, n                                   # never dereferenced by the host-side checks
    cum = lambda n_pair: ((n_pair + 1) * 4 + 255) // 256 * 256
    ws = lambda n_pair, Ls, K=5: cum(n_pair) + n_pair * K * 2 * Ls * 128 * 4
    B = C.byref
    assert lib.dr4sr_regen_score_workspace_bytes(B(p), 100, 50, 19, 5) == ws(100, 50) == lib.dr4sr_regen_score_workspace_bytes(B(p), 100, 50, 19, 1)
    assert lib.dr4sr_regen_score_workspace_bytes(B(p), 7, 23, 49, 2) == ws(7, 23)
    assert lib.dr4sr_regen_score_workspace_bytes(B(p), 0, 1, 1, 1) == 256
    for args, rc in (((10, 51, 19, 5), -2), ((10, 50, 51, 5), -2), ((-1, 50, 19, 5), -1), ((10, 0, 19, 5), -1), ((10, 50, 0, 5), -1),
                     ((10, 50, 19, 0), -1), ((1 << 24, 50, 19, 1), -1), ((1 << 23, 50, 50, 5), -1)):
        assert lib.dr4sr_regen_score_workspace_bytes(B(p), *args) == rc, args
    q = _lib.RegenPlan.from_buffer_copy(p)
    q.n_params = n_old                                                # the decode layout's buffer is refused
    assert lib.dr4sr_regen_score_workspace_bytes(B(q), 10, 50, 19, 5) == -1
    for field, val, rc in (("D", 128, -2), ("H", 4, -2), ("F", 128, -2), ("n_layer", 3, -2), ("K", 6, -2), ("abi_version", 9, -1), ("params", 0, -1)):
        q = _lib.RegenPlan.from_buffer_copy(p)
        setattr(q, field, val)
        assert lib.dr4sr_regen_score_workspace_bytes(B(q), 10, 50, 19, 5) == rc, field
    a = C.c_void_p(64)
    wsp, big = C.c_void_p(8192), 1 << 40
    score = lambda **kw: lib.dr4sr_regen_score(B(kw.get("plan", p)), kw.get("src", a), kw.get("src_len", a), kw.get("tgt", a), kw.get("tgt_len", a),
                                               kw.get("n", 4), kw.get("Ls", 50), kw.get("T", 19), kw.get("w", a), kw.get("n_w", 5), 1,
                                               kw.get("ws", wsp), kw.get("bytes", big), kw.get("nll", a), None)
    for name in ("src", "src_len", "tgt", "tgt_len", "w", "nll"):
        assert score(**{name: None}) == -1, name
    assert score(Ls=51) == -2 and score(T=51) == -2 and score(n_w=0) == -1 and score(n=-1) == -1 and score(Ls=0) == -1 and score(T=0) == -1
    assert score(ws=None) == -3 and score(bytes=ws(4, 50) - 1) == -3 and score(plan=q) == -1
    assert score(n=0) == 0                                            # nothing to do: nothing is launched
    cond = lambda **kw: lib.dr4sr_regen_score_condition(B(kw.get("plan", p)), kw.get("tgt", a), kw.get("tgt_len", a), kw.get("n", 4), kw.get("T", 19),
                                                        kw.get("ws", wsp), kw.get("bytes", big), kw.get("out", a), None)
    for name in ("tgt", "tgt_len", "out"):
        assert cond(**{name: None}) == -1, name
    assert cond(T=51) == -2 and cond(T=0) == -1 and cond(n=-1) == -1 and cond(ws=None) == -3 and cond(bytes=cum(4) - 1) == -3
    assert cond(plan=q) == -1 and cond(n=0) == 0


def test_state_dict_without_condition_encoder():
    from dr4sr_amd.regen import RegenModel, random_state_dict
    sd = random_state_dict(40, K=3, seed=1, std=0.3)
    m = RegenModel.from_state_dict(sd, "cpu")
    assert not m.has_condition_encoder
    assert len(m.decode([[40, 3, 4, 5, 41]], backend="torch")) == 3
    pairs = [[[3, 4, 5, 6], [4, 6]], [[7, 8], [8]]]
    r = m.score(pairs, "all", backend="torch")
    assert r.nll.shape == (3, 2, 19) and r.cond_logits is None and torch.isfinite(r.nll).all() and r.n_tok.tolist() == [3, 2]
    with pytest.raises(ValueError, match="condition_encoder"):
        m.score(pairs, "encoder", backend="torch")
    with pytest.raises(ValueError, match="conditions"):
        m.score(pairs, "best", backend="torch")
    with pytest.raises(ValueError, match="backend"):
        m.score(pairs, "all", backend="eager")
    with pytest.raises(ValueError, match="condition weights"):
        m.score(pairs, torch.ones(1, 3, 3), backend="torch")
    full = RegenModel.from_state_dict(random_state_dict(40, K=3, seed=1, std=0.3, condition_encoder=True), "cpu")
    assert full.has_condition_encoder
    r2 = full.score(pairs, "all", backend="torch")
    assert torch.equal(r2.nll, r.nll) and r2.cond_logits.shape == (2, 3)         # the decoder never reads the condition encoder
    assert full.decode([[40, 3, 4, 5, 41]], backend="torch") == m.decode([[40, 3, 4, 5, 41]], backend="torch")
    enc = full.score(pairs, "encoder", backend="torch")
    w = torch.softmax(r2.cond_logits, -1)[None]
    assert torch.equal(full.score(pairs, w, backend="torch").nll, enc.nll) and enc.loss().shape == (1,)
    assert torch.allclose(enc.per_pair().sum() / 5, enc.loss()[0])


def test_random_state_dict_is_what_the_parent_returned():
    from dr4sr_amd.regen import param_names, random_state_dict, score_param_names

    def digest(sd):
        h = hashlib.sha256()
        for k in sorted(sd):
            h.update(k.encode())
            h.update(str(tuple(sd[k].shape)).encode())
            h.update(sd[k].contiguous().numpy().tobytes())
        return h.hexdigest()

    pinned = "e5e8e46a2453a2ac280a24203668221c7cd9afe8f6e28e837f31bff452d447ba"       # computed on the commit before condition_encoder=
    sd = random_state_dict(seed=3, std=0.3)
    assert set(sd) == set(param_names()) | {"item_embedding_decoder.weight"} and digest(sd) == pinned
    more = random_state_dict(seed=3, std=0.3, condition_encoder=True)
    assert set(more) == set(score_param_names()) | {"item_embedding_decoder.weight"}
    assert digest({k: v for k, v in more.items() if k in sd}) == pinned
    assert float(more["condition_encoder.encoder.layers.1.norm2.weight"].min()) == 1.0


def test_cli_score_prints_the_documented_json(tmp_path, capsys):
    from dr4sr_amd.regen import main, random_state_dict
    root = tmp_path / "dataset" / "tiny" / "tinyd"
    root.mkdir(parents=True)
    n_item = 50
    rng = np.random.default_rng(0)
    pairs = []
    for _ in range(40):
        s = rng.integers(1, n_item, int(rng.integers(2, 12))).tolist()
        pos = sorted(rng.choice(len(s), int(rng.integers(1, min(4, len(s)) + 1)), replace=False).tolist())
        pairs.append([s, [s[p] for p in pos]])
    torch.save(pairs, root / "seq-pat-pair.pth")
    torch.save(random_state_dict(n_item, K=4, seed=2, std=0.3, condition_encoder=True), root / "regenerator.pth")
    main(["--score", "--root_path", str(root) + "/", "--backend", "torch", "--device", "cpu"])
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert set(rep) == {"pairs", "tokens", "width", "causal_source", "inf_tokens", "loss_encoder", "loss_best_condition", "nll_per_condition",
                        "argmin_hist", "encoder_argmax_hist", "agreement"}
    assert rep["pairs"] == 40 and rep["tokens"] == sum(len(t) + 1 for _, t in pairs) and rep["inf_tokens"] == 0 and rep["causal_source"]
    assert len(rep["nll_per_condition"]) == 4 and sum(rep["argmin_hist"]) == 40 == sum(rep["encoder_argmax_hist"])
    assert rep["loss_best_condition"] <= min(rep["nll_per_condition"]) + 1e-12 and 0.0 <= rep["agreement"] <= 1.0
    assert np.isfinite(rep["loss_encoder"])
    main(["--score", "--root_path", str(root) + "/", "--backend", "torch", "--device", "cpu", "--bidirectional_source", "--end", "0"])
    rep2 = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rep2["pairs"] == 0 and not rep2["causal_source"]
