"""Train-mode dropout of the regenerator without a GPU: the host mirror of the kernels' masks (dr4sr_amd/regen_dropout.py), the torch
restatement that applies them (RegenModel backend="torch", dropout=RegenDropout(...)), and the reference's own train-mode gradients
(tests/golden/regen_train_toys.npz, made by tools/make_regen_train_golden.py from the reference's Generator in model.train() with its
random dropout replaced by these masks)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from test_regen_grad_cpu import small_model, small_pairs

GOLD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_train_fixture():
    """(arrays, the scoring fixture's state dict, its first pairs, err32 per tensor, widths, the RegenDropout of the recorded step)"""
    from dr4sr_amd.regen import RegenDropout
    from test_regen_score_cpu import load_score_fixture
    z = dict(np.load(os.path.join(GOLD_DIR, "regen_train_toys.npz")))
    for name in json.loads(str(z["parts"])):
        z.update(np.load(os.path.join(GOLD_DIR, name)))
    _, sd, pairs, _, width = load_score_fixture()
    assert width == (int(z["Ls"]), int(z["T"]))
    return z, sd, pairs[:int(z["n_pairs"])], json.loads(str(z["err32"])), width, RegenDropout(float(z["p"]), int(z["seed"]), int(z["step"]))


def test_torch_backend_matches_the_reference_train_mode_gradients():
    """backend="torch" with the recorded (p, seed, step) against loss.backward() of the reference's Generator in model.train() under the
    same masks (loss_fn + 1 * reg_loss, recorded Gumbel noise, tau 1, causal source mask).  The bounds are those of
    tests/test_regen_grad_cpu.py for the eval fixture: fp32 within 4 x err32_t of the reference's fp32 gradients, float64 within
    1 x err32_t + 1e-10 x max |gradient| (err32_t = max |reference fp32 - reference float64| per tensor, stored; the tool asserts the
    float64 sides agree to 1e-10 relative), the two loss terms against the recorded scalars"""
    from dr4sr_amd.regen import RegenModel, score_param_names
    z, sd, pairs, err32, width, drop = load_train_fixture()
    m = RegenModel.from_state_dict(sd, "cpu")
    assert len(pairs) == 256 and drop.p == 0.5 and float(z["agree64"]) < 1e-10 and max(json.loads(str(z["ratio32"])).values()) <= 4
    kw = dict(noise=torch.from_numpy(z["noise"]), tau=1.0, entropy_weight=1.0, dropout=drop)
    res = {32: m.loss_and_grad(pairs, "encoder", True, width, "torch", torch.float32, **kw),
           64: m.loss_and_grad(pairs, "encoder", True, width, "torch", torch.float64, **kw)}
    for bits, factor, slack in ((32, 4, 0.0), (64, 1, 1e-10)):
        bad, worst = [], 0.0
        for k in score_param_names():
            want = z[f"g:{k}"]
            d = float((res[bits].grads[k].double() - torch.from_numpy(want).double()).abs().max())
            worst = max(worst, d / err32[k]) if err32[k] > 0 else worst
            if d > factor * err32[k] + slack * float(np.abs(want).max()):
                bad.append(f"{k}: |diff| {d:.3e} > {factor} x err32 {err32[k]:.3e}")
        print(f"fp{bits} restatement vs the reference in train mode: worst |diff| / err32_t over 98 tensors: {worst:.2f}")
        assert not bad, "\n".join(bad)
    e_loss = abs(float(z["loss"]) - float(z["loss64"]))
    e_reg = abs(float(z["reg_loss"]) - float(z["reg_loss64"]))
    assert abs(float(res[64].loss) - float(z["loss64"])) <= 1e-12 and abs(float(res[64].entropy) - float(z["reg_loss64"])) <= 1e-12
    assert abs(float(res[32].loss) - float(z["loss"])) <= 4 * max(e_loss, 6e-8 * 5)
    assert abs(float(res[32].entropy) - float(z["reg_loss"])) <= 4 * max(e_reg, 6e-8 * 2)
    # the fixture is a train-mode one: the eval loss of the same pairs and noise is another number
    ev = m.loss_and_grad(pairs[:32], "encoder", True, width, "torch", torch.float64, noise=kw["noise"][:32])
    tr = m.loss_and_grad(pairs[:32], "encoder", True, width, "torch", torch.float64, noise=kw["noise"][:32], dropout=drop)
    assert abs(float(ev.loss) - float(tr.loss)) > 1e-3


def test_keep_fraction_and_factors_of_every_site_class():
    """p = 0.5: the factors are exactly 0 or 2, and the keep fraction of each of the 30 sites lies within 5 sigma of 1/2 over >= 1e5
    decisions (sigma = 1 / (2 sqrt(n)): the 5 sigma rule of the pairs tests)"""
    from dr4sr_amd import regen_dropout as rd
    d = rd.RegenDropout(0.5, seed=11, step=4)
    assert d.threshold() == 32768 and float(d.scale()) == 2.0
    pairs = np.arange(7, 7 + 32)
    sites = rd.all_sites()
    assert len(sites) == 30
    seen = {}
    for name, (sid, cls) in sites.items():
        f = (rd.keep_probs(d, sid, pairs, 50, 50) if cls == "probs" else rd.keep_rows(d, sid, pairs, 50, 256 if cls == "ffn" else 64))
        assert f.dtype == np.float32 and set(np.unique(f).tolist()) == {0.0, 2.0}, name
        n = f.size
        assert n >= 100_000 and abs(float((f != 0).mean()) - 0.5) <= 5 * 0.5 / np.sqrt(n), (name, n, float((f != 0).mean()))
        seen[name] = f
    assert not np.array_equal(seen["enc0.attn_out"], seen["enc1.attn_out"]) and not np.array_equal(seen["src_emb"], seen["tgt_emb"])
    # the structured forms are the element-index formula
    idx = ((pairs[:, None, None] * 64 + np.arange(50)[None, :, None]) * 256 + np.arange(256)[None, None, :]).astype(np.uint64)
    assert np.array_equal(rd.keep_elements(d, sites["dec1.ffn_hidden"][0], idx), seen["dec1.ffn_hidden"])
    idx = (((pairs[:, None, None, None] * 2 + np.arange(2)[None, :, None, None]) * 64 + np.arange(50)[None, None, :, None]) * 64
           + np.arange(50)[None, None, None, :]).astype(np.uint64)
    assert np.array_equal(rd.keep_elements(d, sites["dec0.cross_probs"][0], idx), seen["dec0.cross_probs"])
    # another p: quantised to 1 / 65536, scale 1 / (1 - p) in fp32
    d3 = rd.RegenDropout(0.3, 1, 2)
    f = rd.keep_rows(d3, rd.SITE_SRC_EMB, pairs, 50, 64)
    assert d3.threshold() == 19661 and set(np.unique(f).tolist()) == {0.0, float(np.float32(1) / (np.float32(1) - np.float32(0.3)))}
    assert abs(float((f != 0).mean()) - (1 - 19661 / 65536)) <= 5 * np.sqrt(0.3 * 0.7 / f.size)
    with pytest.raises(ValueError):
        rd.RegenDropout(1.0)


def test_indices_beyond_32_bits_are_their_own_streams():
    """the probability sites pass 2^32 at pair 524 288: the upper counter word takes part (a mirror that dropped it would repeat pair 0)"""
    from dr4sr_amd import regen_dropout as rd
    d = rd.RegenDropout(0.5, 3, 1)
    sid = rd.site(rd.STACK_DEC, 0, 0)
    lo, hi = rd.keep_probs(d, sid, [0, 1], 50, 50), rd.keep_probs(d, sid, [524288, 524289], 50, 50)
    assert not np.array_equal(lo, hi)
    idx = np.uint64(524288) * np.uint64(8192) + np.arange(64, dtype=np.uint64)
    assert int(idx[0]) == 1 << 32 and np.array_equal(rd.keep_elements(d, sid, idx)[:50], hi[0, 0, 0])


def test_p_zero_is_eval_mode_exactly():
    from dr4sr_amd.regen import RegenDropout
    m = small_model()
    pairs = small_pairs(12, m.n_item, 0)
    a = m.score(pairs, "encoder", True, None, "torch", torch.float32)
    b = m.score(pairs, "encoder", True, None, "torch", torch.float32, dropout=RegenDropout(0.0, 5, 6))
    assert torch.equal(a.nll, b.nll) and torch.equal(a.cond_logits, b.cond_logits)
    ga = m.loss_and_grad(pairs, "encoder", backend="torch", entropy_weight=1.0)
    gb = m.loss_and_grad(pairs, "encoder", backend="torch", entropy_weight=1.0, dropout=RegenDropout(0.0))
    assert float(ga.loss) == float(gb.loss) and all(torch.equal(ga.grads[k], gb.grads[k]) for k in ga.grads)
    with pytest.raises(TypeError):
        m.score(pairs, "encoder", True, None, "torch", dropout=0.5)


def test_chunks_and_widths_do_not_move_the_masks():
    """pairs [a:b] with pair0 = a are rows a..b-1 of the full run, and a wider matrix scores the same.  The masks are exactly the same
    (checked on the mirror); the float64 results are compared to 1e-12 because a torch batch of another shape may block its GEMMs
    differently (rounding ~1e-16 on values of order 10)"""
    from dr4sr_amd import regen_dropout as rd
    from dr4sr_amd.regen import RegenDropout
    m = small_model()
    pairs = small_pairs(20, m.n_item, 3)
    d = RegenDropout(0.5, 9, 2)
    full = m.score(pairs, "encoder", True, None, "torch", torch.float64, dropout=d)
    part = m.score(pairs[7:15], "encoder", True, full.width, "torch", torch.float64, dropout=d, pair0=7)
    assert float((part.nll - full.nll[:, 7:15]).abs().max()) <= 1e-12 and float((part.cond_logits - full.cond_logits[7:15]).abs().max()) <= 1e-12
    wrong = m.score(pairs[7:15], "encoder", True, full.width, "torch", torch.float64, dropout=d)          # pair0 = 0: other masks
    assert float((wrong.nll - full.nll[:, 7:15]).abs().max()) > 1e-3
    # a wider matrix: every source row is padded at both widths (the restricted softmax runs over PAD too when a row is padded, in
    # eval mode as well, so the narrower width is Ls + 1, not Ls)
    Ls, T = full.width
    base = m.score(pairs, "encoder", True, (Ls + 1, T), "torch", torch.float64, dropout=d)
    wide = m.score(pairs, "encoder", True, (Ls + 9, T + 6), "torch", torch.float64, dropout=d)
    assert float((wide.nll[:, :, :T] - base.nll).abs().max()) <= 1e-12 and float(wide.nll[:, :, T:].abs().max()) == 0
    assert float((wide.cond_logits - base.cond_logits).abs().max()) <= 1e-12
    g_full = m.loss_and_grad(pairs, "encoder", backend="torch", dtype=torch.float64, dropout=d, entropy_weight=1.0)
    assert float((g_full.cond_logits - full.cond_logits).abs().max()) <= 1e-12
    sid = rd.site(rd.STACK_DEC, 1, 4)
    assert np.array_equal(rd.keep_rows(d, sid, range(7, 15), T, 256), rd.keep_rows(d, sid, range(20), T + 6, 256)[7:15, :T])
    assert np.array_equal(rd.keep_probs(d, sid - 2, range(7, 15), T, Ls), rd.keep_probs(d, sid - 2, range(20), T + 6, Ls + 9)[7:15, :, :T, :Ls])


def test_step_and_seed_name_the_masks():
    from dr4sr_amd.regen import RegenDropout
    m = small_model()
    pairs = small_pairs(10, m.n_item, 5)
    w = torch.full((1, len(pairs), m.K), 1.0 / m.K)
    loss = lambda d: float(m.loss_and_grad(pairs, w, backend="torch", dtype=torch.float64, dropout=d).loss)
    base = loss(RegenDropout(0.5, 4, 7))
    assert loss(RegenDropout(0.5, 4, 7)) == base
    assert abs(loss(RegenDropout(0.5, 4, 8)) - base) > 1e-6 and abs(loss(RegenDropout(0.5, 5, 7)) - base) > 1e-6
    assert abs(loss(RegenDropout(0.5, 4 + (1 << 32), 7)) - base) > 1e-6          # the seed's upper word is part of the key
    assert abs(loss(None) - base) > 1e-6


def test_condition_encoder_and_decoder_share_the_tgt_emb_mask(monkeypatch):
    """the reference drops tgt_emb ONCE and feeds it to both: the condition logits depend on the tgt_emb site and on no decoder site"""
    from dr4sr_amd import regen_dropout as rd
    from dr4sr_amd.regen import RegenDropout
    m = small_model()
    pairs = small_pairs(10, m.n_item, 8)
    d = RegenDropout(0.5, 2, 3)
    base = m.score(pairs, "encoder", True, None, "torch", torch.float64, dropout=d)
    site0 = rd.site
    monkeypatch.setattr(rd, "site", lambda stack, layer, kind: site0(stack, layer, kind) + (0x100 if stack == rd.STACK_DEC else 0))
    moved = m.score(pairs, "encoder", True, None, "torch", torch.float64, dropout=d)
    assert torch.equal(moved.cond_logits, base.cond_logits) and float((moved.nll - base.nll).abs().max()) > 1e-3
    monkeypatch.setattr(rd, "site", site0)
    monkeypatch.setattr(rd, "SITE_TGT_EMB", rd.SITE_TGT_EMB + 0x100)
    moved = m.score(pairs, "encoder", True, None, "torch", torch.float64, dropout=d)
    assert float((moved.cond_logits - base.cond_logits).abs().max()) > 1e-3 and float((moved.nll - base.nll).abs().max()) > 1e-3


def test_argument_errors_of_the_train_entry_points():
    """the *_train forms check (p, pair0) before anything else and then what their eval forms check (the library loads without a GPU)"""
    from dr4sr_amd import _lib
    lib = _lib.load()
    assert lib.dr4sr_abi_version() == 10 == _lib.ABI_VERSION
    p = _lib.RegenPlan()
    p.abi_version, p.n_rows, p.K, p.max_len, p.D, p.H, p.F, p.n_layer, p.ln_eps = 10, 11927, 5, 25, 64, 2, 256, 2, 1e-12
    p.params, p.n_params = 4096, lib.dr4sr_regen_score_param_layout(11927, 5, None)
    B, a, ws, big = C.byref, C.c_void_p(64), C.c_void_p(8192), 1 << 40
    drop = lambda pd=0.5, pair0=0: (C.c_float(pd), C.c_uint64(1), C.c_uint32(2), C.c_int64(pair0))
    calls = {
        "score": lambda n=4, T=19, **k: lib.dr4sr_regen_score_train(B(p), a, a, a, a, n, 50, T, a, 2, 1, ws, big, a, *drop(**k), None),
        "cond": lambda n=4, T=19, **k: lib.dr4sr_regen_score_condition_train(B(p), a, a, n, T, ws, big, a, *drop(**k), None),
        "bwd": lambda n=4, T=19, **k: lib.dr4sr_regen_score_bwd_train(B(p), a, a, a, a, n, 50, T, a, 2, 1, a, ws, big, a, a, None, 1, *drop(**k), None),
        "cond_bwd": lambda n=4, T=19, **k: lib.dr4sr_regen_score_condition_bwd_train(B(p), a, a, n, T, a, ws, big, a, 1, *drop(**k), None),
    }
    for name, f in calls.items():
        assert f(n=0, pd=1.0) == -1 and f(n=0, pd=-0.1) == -1 and f(n=0, pair0=-1) == -1 and f(n=0, pair0=1 << 40) == -1, name
        assert f(n=0) == 0 and f(n=0, pd=0.0) == 0 and f(n=0, pair0=600000) == 0, name          # nothing to do: nothing is launched
        assert f(T=51) == -2 and f(n=-1) == -1 and f(T=51, pd=0.0) == -2, name
