"""Teacher-forced scoring of the regenerator on the MI355X (csrc/regen_score.hip through dr4sr_regen_score / dr4sr_regen_score_condition):
per-token NLLs and condition logits against the reference's (tests/golden/regen_score_toys.npz) and against the float64 torch
restatement, bitwise batch independence, graph capture, and stage 3's decode left as it was.

Tolerance: 16 x err32, err32 being the reference's own fp32 rounding noise against float64 on the same rows (stored in the fixture;
taken from a fp32 torch run for the synthetic rows).  The kernels sum reductions of length 64, 256 and 320 in MFMA order and use the
device's erf / exp / rsqrt through six layers; a structural error moves an NLL by 1e-2 or more.
Measured on the MI355X (worst ratio |HIP - float64| / err32 over all modes): see DESIGN.md 4i."""
import json
import os

import numpy as np
import pytest
import torch

from test_regen_cpu import load_fixture, tokens_agree
from test_regen_score_cpu import MODES, check_close, conditions_of, load_score_fixture, reference_of

pytestmark = pytest.mark.gpu


def toys_shaped_pairs(n, n_item, seed):
    """sequences of about 9 items (a few up to 48) with a pattern of 1..6 of their items in order; some patterns of 18 fill the width"""
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


def test_hip_matches_reference_in_all_six_modes():
    from dr4sr_amd.regen import RegenModel
    z, sd, pairs, err32, width = load_score_fixture()
    m = RegenModel.from_state_dict(sd, "cuda")
    cpu = RegenModel.from_state_dict(sd, "cpu")
    n, T = len(pairs), width[1]
    seen, worst = 0, 0.0
    for ci, causal in enumerate((True, False)):
        tag = "causal" if causal else "bidir"
        for mode in MODES:
            cond = conditions_of(z, mode, ci)
            ref = reference_of(z, mode, ci)
            hip = m.score(pairs, cond, causal, width, "hip")
            r64 = cpu.score(pairs, cond, causal, width, "torch", torch.float64)
            e, ec = err32[f"nll_{mode}_{tag}"], err32["cond_logits"]
            d = check_close(hip.nll, r64.nll, 16 * e, f"HIP vs float64 {mode} {tag}", ref.numel(), e)
            check_close(hip.nll, ref, 16 * e, f"HIP vs reference {mode} {tag}", ref.numel(), e)
            check_close(hip.cond_logits, r64.cond_logits, 16 * ec, f"HIP condition logits vs float64 {mode} {tag}", n * 5, ec)
            check_close(hip.cond_logits, z["cond_logits"], 16 * ec, f"HIP condition logits vs reference {mode} {tag}", n * 5, ec)
            assert int(torch.isinf(hip.nll).sum()) == 3 * ref.shape[0]
            assert torch.equal(hip.nll == 0, ref == 0)
            worst = max(worst, d / e)
            seen += ref.numel()
    assert seen == 2 * (1 + 5 + 1) * n * T
    print(f"worst |HIP - float64| / err32 over the six modes: {worst:.2f}")
    nb = int(z["loss_batch_n"])
    got = m.score(pairs[:nb], "encoder", True, width, "hip").loss()
    assert abs(float(got[0]) - float(z["loss_batch"])) <= 16 * err32["nll_softmax_causal"]
    # the width rules on the device: rows that fill the width, scored one column wider
    wide = [int(i) for i in z["wide_idx"]]
    w = m.score([pairs[i] for i in wide], "all", True, (width[0], T + 1), "hip")
    check_close(w.nll, z["wide_nll"], 16 * err32["wide_nll"], "HIP rows that fill the width, one column wider", None, err32["wide_nll"])
    check_close(w.cond_logits, z["wide_cond"], 16 * err32["wide_cond"], "HIP their condition logits", None, err32["wide_cond"])


def test_hip_matches_float64_on_toys_shaped_pairs():
    from dr4sr_amd.regen import RegenModel, random_state_dict
    m = RegenModel.from_state_dict(random_state_dict(seed=3, std=0.3, condition_encoder=True), "cuda")
    assert m.K == 5
    pairs = toys_shaped_pairs(5000, m.n_item, 7)
    g = torch.Generator().manual_seed(1)
    mixed = torch.softmax(2 * torch.randn(2, len(pairs), 5, generator=g), -1)
    worst = 0.0
    for causal in (True, False):
        for cond in ("all", "encoder", mixed):
            name = cond if isinstance(cond, str) else "weights"
            hip = m.score(pairs, cond, causal, None, "hip")
            r32 = m.score(pairs, cond, causal, None, "torch")
            r64 = m.score(pairs, cond, causal, None, "torch", torch.float64)
            fin = torch.isfinite(r64.nll)
            assert fin.all()
            e = float((r32.nll.double() - r64.nll)[fin].abs().max())
            ec = float((r32.cond_logits.double() - r64.cond_logits).abs().max())
            d = check_close(hip.nll, r64.nll, 16 * e, f"HIP vs float64, {name}, causal={causal}", None, e)
            check_close(hip.cond_logits, r64.cond_logits, 16 * ec, f"HIP condition logits, {name}, causal={causal}", None, ec)
            assert torch.equal(hip.nll == 0, r64.nll == 0) and torch.equal(hip.n_tok, r64.n_tok)
            worst = max(worst, d / e)
    print(f"worst |HIP - float64| / err32 on 5 000 toys-shaped pairs: {worst:.2f}")


def test_scores_are_bitwise_independent_of_the_batch():
    from dr4sr_amd.regen import RegenModel, random_state_dict
    m = RegenModel.from_state_dict(random_state_dict(seed=5, std=0.3, condition_encoder=True), "cuda")
    pairs = toys_shaped_pairs(4096, m.n_item, 11)
    big = m.score(pairs, "all", True, None, "hip")                 # 4 096 pairs x 5 weight vectors in one call
    again = m.score(pairs, "all", True, None, "hip")
    assert torch.equal(big.nll, again.nll) and torch.equal(big.cond_logits, again.cond_logits)
    assert big.width == (50, 19) and torch.isfinite(big.nll).all()
    for i in (0, 1, 2, 3, 777, 4095):
        one = m.score([pairs[i]], "all", True, big.width, "hip")
        assert torch.equal(one.nll[:, 0], big.nll[:, i]) and torch.equal(one.cond_logits[0], big.cond_logits[i]), i
    perm = torch.randperm(len(pairs), generator=torch.Generator().manual_seed(0))
    shuf = m.score([pairs[int(i)] for i in perm], "all", True, big.width, "hip")
    assert torch.equal(shuf.nll, big.nll[:, perm]) and torch.equal(shuf.cond_logits, big.cond_logits[perm])
    for k in (0, 3):                                                # row k of "all" is the explicit one-hot call, alone among the weights
        w = torch.zeros(1, len(pairs), 5)
        w[:, :, k] = 1
        assert torch.equal(m.score(pairs, w, True, None, "hip").nll[0], big.nll[k]), k
    enc = m.score(pairs, "encoder", True, None, "hip")
    w = torch.softmax(big.cond_logits.to("cuda"), -1).cpu()[None]
    assert torch.equal(m.score(pairs, w, True, None, "hip").nll, enc.nll)
    part = m.score(pairs[100:300], "encoder", False, big.width, "hip")
    assert torch.equal(part.nll, m.score(pairs, "encoder", False, None, "hip").nll[:, 100:300])


def test_graph_capture_replays_the_same_bits():
    from dr4sr_amd.regen import RegenModel, random_state_dict
    m = RegenModel.from_state_dict(random_state_dict(300, seed=6, std=0.3, condition_encoder=True), "cuda")
    pairs = toys_shaped_pairs(600, m.n_item, 13)
    src, src_len, tgt, tgt_len, Ls, T = m._pack_pairs(pairs, None)
    dev = [t.cuda().contiguous() for t in (src, src_len, tgt, tgt_len)]
    w = torch.softmax(torch.randn(3, len(pairs), 5, generator=torch.Generator().manual_seed(2)), -1).cuda().contiguous()
    eager = m.score_device(*dev, w, True).clone()
    eager_c = m.condition_device(dev[2], dev[3]).clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.score_device(*dev, w, True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m.score_device(*dev, w, True)
        out_c = m.condition_device(dev[2], dev[3])
    for _ in range(2):
        out.fill_(-1.0)
        out_c.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(out_c, eager_c)


def test_decode_is_unchanged_after_a_score():
    """stage 3's tokens for the existing fixture, decoded by a model that has just scored (shared parameters, reused allocations)"""
    from dr4sr_amd.regen import RegenModel
    z, sd, train, src, ref = load_fixture()
    m = RegenModel.from_state_dict(sd, "cuda")
    assert not m.has_condition_encoder
    before = m.decode(src, backend="hip")
    pairs = [[s[1:-1], s[1:-1][::2][:6] or s[1:2]] for s in src]
    r = m.score(pairs, "all", True, None, "hip")
    assert r.cond_logits is None and torch.isfinite(r.nll).all()
    cpu = RegenModel.from_state_dict(sd, "cpu")
    r64 = cpu.score(pairs, "all", True, None, "torch", torch.float64)
    e = float((cpu.score(pairs, "all", True, None, "torch").nll.double() - r64.nll).abs().max())
    check_close(r.nll, r64.nll, 16 * e, "HIP vs float64 on the decode fixture's sources", None, e)
    with pytest.raises(ValueError, match="condition_encoder"):
        m.score(pairs, "encoder")
    got = m.decode(src, backend="hip")
    assert got == before
    bad = [i for i in range(len(ref)) if not tokens_agree(got[i], ref[i], z["gaps"][i], z["top"][i])]
    assert not bad, [(i, got[i], ref[i]) for i in bad[:3]]
