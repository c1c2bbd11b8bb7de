"""Pre-training of the regenerator on the MI355X (dr4sr_amd/regen_train.py, csrc/regen_head.hip): the condition head against float64
autograd of the same formula, one training step against RegenModel.loss_and_grad and torch.optim.Adam, a 24-step trajectory against the
same loop in torch, the bit-level promises, and the command line end to end.

Tolerance unit, as the other regenerator tests: err32 = max |fp32 torch - float64 torch| of the same quantity under the same masks and
noise, computed here; bound |HIP - float64| <= 16 x err32.

The torch sides take their dropout masks from the device hook dr4sr_dropout_mask instead of the numpy mirror (HookDrop below):
tests/test_gpu_regen_dropout.py proves the two equal bit for bit, one check here repeats it, and a 24-step loop in two precisions spends
seconds instead of a minute on generating masks."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_gpu_regen_score import toys_shaped_pairs
from test_regen_score_cpu import check_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ITEM, K, SEED, WIDTH = 300, 5, 2024, (50, 19)
FREE_ID, TAKEN_ID = 7, 8
_cache = {}


def pool():
    """the 512 toys-shaped pairs, with id 7 written as id 8 everywhere: an id no pair holds (its table row must never move)"""
    if "pool" not in _cache:
        sub = lambda seq: [TAKEN_ID if v == FREE_ID else v for v in seq]
        _cache["pool"] = [[sub(s), sub(t)] for s, t in toys_shaped_pairs(512, N_ITEM, 11)]
    return _cache["pool"]


def fresh_model(device="cuda", K=K):
    from dr4sr_amd.regen import RegenModel, random_state_dict
    return RegenModel.from_state_dict(random_state_dict(N_ITEM, K=K, seed=5, std=0.1, condition_encoder=True), device)


def make_trainer(**kw):
    from dr4sr_amd.regen_train import RegenTrainer
    kw.setdefault("seed", SEED)
    return RegenTrainer(fresh_model(), kw.pop("pairs", pool()), **kw)


def mirror_noise(step, n, seed=SEED):
    from dr4sr_amd import regen_dropout as rd
    return torch.from_numpy(rd.gumbel_noise(seed, step, np.arange(n), K))


class HookDrop:
    """regen_torch's TorchDrop with the masks from the device hook: the whole (seed, step, site) stream from element 0 up to the last
    pair, cut to the pairs and the shape asked for"""

    def __init__(self, d, pair0, n, dtype, device):
        self.d, self.pair0, self.n, self.dtype, self.device, self.cache = d, int(pair0), int(n), dtype, device, {}
        assert self.pair0 + self.n <= 4096, "the hook materialises the stream from element 0"

    def _stream(self, s, per_pair):
        from dr4sr_amd import _lib, regen_dropout as rd
        sid = {"src_emb": rd.SITE_SRC_EMB, "tgt_emb": rd.SITE_TGT_EMB}[s] if isinstance(s, str) else rd.site(*s)
        if (sid, per_pair) not in self.cache:
            cnt = (self.pair0 + self.n) * per_pair
            out = torch.empty(cnt, dtype=torch.float32, device="cuda")
            _lib.check(_lib.load().dr4sr_dropout_mask(_lib.ptr(out), cnt, self.d.p, self.d.seed, self.d.step, sid, _lib.cur_stream()), "dr4sr_dropout_mask")
            self.cache[(sid, per_pair)] = (out[self.pair0 * per_pair:] * float(self.d.scale())).to(device=self.device, dtype=self.dtype)
        return self.cache[(sid, per_pair)]

    def rows(self, s, x):
        n_pos, n_col = x.shape[1:]
        return self._stream(s, 64 * n_col).view(self.n, 64, n_col)[:, :n_pos]

    def probs(self, s, a):
        n_q, n_k = a.shape[2:]
        return self._stream(s, 2 * 64 * 64).view(self.n, 2, 64, 64)[:, :, :n_q, :n_k]


@pytest.fixture
def hook_masks(monkeypatch):
    """loss_and_grad(backend="torch") with HookDrop masks"""
    from dr4sr_amd import regen_dropout, regen_torch

    def of(dropout, pair0, n, dtype, device):
        return None if regen_dropout.eval_mode(dropout) else HookDrop(dropout, pair0, n, dtype, device)

    monkeypatch.setattr(regen_torch.TorchDrop, "of", staticmethod(of))


def test_hook_masks_are_the_mirror_masks():
    from dr4sr_amd.regen import RegenDropout
    from dr4sr_amd.regen_torch import TorchDrop
    d = RegenDropout(0.5, SEED, 3)
    a, b = HookDrop(d, 2, 9, torch.float64, "cuda"), TorchDrop(d, 2, 9, torch.float64, "cuda")
    for s, x in (("tgt_emb", torch.empty(9, 19, 64)), ((2, 1, 4), torch.empty(9, 19, 256)), ((0, 0, 3), torch.empty(9, 50, 64))):
        assert torch.equal(a.rows(s, x), b.rows(s, x)), s
    for s, x in (((2, 0, 2), torch.empty(9, 2, 19, 50)), ((1, 1, 0), torch.empty(9, 2, 19, 19))):
        assert torch.equal(a.probs(s, x), b.probs(s, x)), s


# ---------------------------------------------------------------------------------------------------- 1. the head
def head_ref(logits, noise, dw, tau, ew, n_batch, dt):
    c = logits.to(dt).requires_grad_(True)
    w = torch.softmax((c + noise.to(dt)) / tau, -1)
    ent = -(w * torch.log(w + 1e-12)).sum(-1)
    (dl,) = torch.autograd.grad((w * dw.to(dt)).sum() + ew * ent.sum() / n_batch, c)
    return w.detach(), ent.detach(), dl


def ulps_apart(a, b):
    """distance in representable fp32 values"""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


@pytest.mark.parametrize("k", [1, 3, 5])
def test_head_forward_and_backward_match_float64(k):
    from dr4sr_amd.regen_train import head_bwd_device, head_fwd_device
    T, worst = 19, 0.0
    for n in (1, 63, 257):
        g = torch.Generator().manual_seed(100 * n + k)
        logits, dw = 2 * torch.randn(n, k, generator=g), torch.randn(n, k, generator=g)
        noise = -torch.log(-torch.log(torch.rand(n, k, generator=g).clamp_min(1e-9)))
        nll = torch.rand(1, n, T, generator=g)
        n_tok = 3 * n + 1
        for tau in (1.0, 0.37, 0.1):
            for ew in (0.0, 1.0):
                w, ent, dnll, used = head_fwd_device(logits.cuda(), T, tau, n_tok, noise=noise.cuda(), want_noise=True)
                loss_log, ent_log = torch.zeros(3, device="cuda"), torch.zeros(3, device="cuda")
                dl = head_bwd_device(dw.cuda()[None].contiguous(), w, ent, nll.cuda(), tau, ew, n, n_tok, loss_log, ent_log, 1)
                assert torch.equal(used.cpu(), noise) and tuple(w.shape) == (1, n, k)
                assert torch.equal(dnll.cpu(), torch.full((1, n, T), 1.0 / n_tok, dtype=torch.float32))
                r32, r64 = head_ref(logits, noise, dw, tau, ew, n, torch.float32), head_ref(logits, noise, dw, tau, ew, n, torch.float64)
                for name, got, a32, a64 in zip(("w", "entropy", "dlogits"), (w[0], ent, dl), r32, r64):
                    e = float((a32.double() - a64).abs().max())
                    dd = check_close(got.cpu(), a64, 16 * e, f"head {name}: n={n} K={k} tau={tau} entropy weight {ew}", None, e or None)
                    worst = max(worst, dd / e) if e > 0 else worst
                # the step's log: this call's sums land in the slot, the neighbours stay
                assert float(loss_log[0]) == 0.0 and float(loss_log[2]) == 0.0 and float(ent_log[0]) == 0.0 and float(ent_log[2]) == 0.0
                want_loss, want_ent = float(nll.double().sum()) / n_tok, float(ent.double().sum()) / n
                assert abs(float(loss_log[1]) - want_loss) <= n * T * 2.0 ** -24 * want_loss
                assert abs(float(ent_log[1]) - want_ent) <= n * 2.0 ** -24 * abs(want_ent) + 1e-12
    print(f"K={k}: worst |HIP - float64| / err32 over w, entropy and dlogits: {worst:.2f}")


def test_head_generated_noise_is_the_mirror_and_bits_do_not_depend_on_chunking():
    from dr4sr_amd import regen_dropout as rd
    from dr4sr_amd.regen_train import head_bwd_device, head_fwd_device
    n, T, tau, n_tok = 257, 19, 0.37, 1000
    g = torch.Generator().manual_seed(5)
    logits, dw = (2 * torch.randn(n, K, generator=g)).cuda(), torch.randn(1, n, K, generator=g).cuda()
    nll = torch.rand(1, n, T, generator=g).cuda()
    for base in (0, (1 << 33) + 5):
        kw = dict(seed=SEED, step=3)
        w, ent, dnll, used = head_fwd_device(logits, T, tau, n_tok, pair0=base, want_noise=True, **kw)
        want = rd.gumbel_noise(SEED, 3, base + np.arange(n, dtype=np.uint64), K)
        apart = ulps_apart(used.cpu().numpy(), want)
        print(f"pair0 = {base}: generated noise vs the float64 mirror: {int((apart != 0).sum())} of {apart.size} differ, at most {int(apart.max())} ulp")
        assert int(apart.max()) <= 2
        # the same call twice: the same bits; the recorded form of the device's own noise: the same weights
        again = head_fwd_device(logits, T, tau, n_tok, pair0=base, want_noise=True, **kw)
        assert all(torch.equal(a, b) for a, b in zip((w, ent, dnll, used), again))
        rec = head_fwd_device(logits, T, tau, n_tok, noise=used)
        assert torch.equal(rec[0], w) and torch.equal(rec[1], ent)
        dl = head_bwd_device(dw, w, ent, nll, tau, 1.0, n, n_tok)
        assert torch.equal(dl, head_bwd_device(dw, w, ent, nll, tau, 1.0, n, n_tok))
        # 100 + 157 with pair0 set accordingly: the bits of the whole
        parts, log = [], torch.zeros(1, device="cuda")
        for a, b in ((0, 100), (100, 257)):
            wp, ep, dp, up = head_fwd_device(logits[a:b], T, tau, n_tok, pair0=base + a, want_noise=True, **kw)
            dlp = head_bwd_device(dw[:, a:b].contiguous(), wp, ep, nll[:, a:b].contiguous(), tau, 1.0, n, n_tok, log, None, 0)
            parts.append((wp, ep, dp, up, dlp))
        for i, whole in enumerate((w, ent, dnll, used)):
            assert torch.equal(torch.cat([p[i] for p in parts], 1 if whole.dim() == 3 else 0), whole), i
        assert torch.equal(torch.cat([p[4] for p in parts]), dl)
        assert abs(float(log[0]) - float(nll.double().sum()) / n_tok) <= n * T * 2.0 ** -24 * float(nll.double().sum()) / n_tok
    other = head_fwd_device(logits, T, tau, n_tok, pair0=5, want_noise=True, seed=SEED, step=3)[3]
    assert not torch.equal(other, used), "pair0 = 2^33 + 5 must not draw what pair0 = 5 draws"
    for kw in (dict(seed=SEED + 1, step=3), dict(seed=SEED, step=4)):
        assert not torch.equal(head_fwd_device(logits, T, tau, n_tok, pair0=5, want_noise=True, **kw)[3], other)


# ---------------------------------------------------------------------------------------------------- 2, 3. one step
def settle_batch(m, pairs, nb, d):
    """tests/test_gpu_regen_dropout.py's selection for a batch whose masks follow the OFFSET in the batch: start from pairs 0 .. nb - 1;
    a slot whose pair has an input of either ReLU within 16 x the fp32 noise of that activation (decided from the float64 and fp32 torch
    runs alone, under the slot's masks) takes the next unused pair, four times over.  A slot can be near whatever pair sits in it (a
    source's position 0 sees only SOS and the slot's own masks): such slots stay in the batch, which has no gaps, and are returned as
    `bad`; the comparison leaves their pairs' terms out of the compared scalar on all three sides.  At most half of the slots may change
    or be left out, the share tests/test_gpu_regen_dropout.py allows"""
    from test_gpu_regen_dropout import relu_inputs
    dev = m.device
    chosen, spare, changed, noise = list(range(nb)), list(range(nb, len(pairs))), 0, None
    slots = list(range(nb))
    for rnd in range(5):
        src, src_len, tgt, tgt_len, Ls, T = m._pack_pairs([pairs[chosen[j]] for j in slots], WIDTH)
        src, src_len, tgt, tgt_len = (t.to(dev) for t in (src, src_len, tgt, tgt_len))
        w = torch.full((1, len(slots), m.K), 1.0 / m.K, device=dev)
        pre = {}
        for dt in (torch.float32, torch.float64):
            td = HookDrop(d, 0, nb, dt, dev)
            if len(slots) != nb:                     # the changed slots alone, each under its own offset's masks
                full, sel = td, torch.tensor(slots, device=dev)
                td = type("Rows", (), {"rows": lambda self, s, x: full.rows(s, torch.empty(nb, *x.shape[1:]))[sel],
                                       "probs": lambda self, s, a: full.probs(s, torch.empty(nb, 2, *a.shape[2:]))[sel]})()
            pre[dt] = relu_inputs(m, src, tgt, tgt_len, w, dt, td, True)
        live = (torch.arange(Ls, device=dev)[None, :] < src_len[:, None])[:, :, None].expand_as(pre[torch.float64][0])
        if noise is None:                            # the unit: the fp32 noise over the whole first batch
            noise = (float((pre[torch.float32][0].double() - pre[torch.float64][0])[live].abs().max()),
                     float((pre[torch.float32][1].double() - pre[torch.float64][1]).abs().max()))
        near = ((pre[torch.float64][0].abs() <= 16 * noise[0]) & live).flatten(1).any(1) | (pre[torch.float64][1].abs() <= 16 * noise[1]).any(1)
        slots = [slots[j] for j in near.nonzero().flatten().tolist()]
        if not slots or rnd == 4:
            break
        for j in slots:
            chosen[j] = spare.pop(0)
            changed += 1
    print(f"fp32 noise of the ReLU inputs {noise[0]:.2e} / {noise[1]:.2e}; {changed} of {nb} slots changed their pair, "
          f"{len(slots)} stay near with every pair tried: {slots}")
    assert changed + len(slots) <= nb // 2, "the selection may change or leave out at most half of the slots"
    return chosen, slots


def torch_side(m, batch, good, n_tok, noise, tau, d, dt):
    """what loss_and_grad(backend="torch") differentiates, written out so that the scalar can leave pairs out: the gradient of
    sum over the GOOD pairs of (their token NLLs / n_tok + their entropy term / n_batch), n_tok and n_batch of the whole batch; with every
    pair good this is loss_and_grad's CE + 1 x entropy.  Returns (grads by name, CE of the whole batch, mean entropy of the whole batch)"""
    from dr4sr_amd import regen_torch
    dev, nb = m.device, len(batch)
    src, src_len, tgt, tgt_len, Ls, T = m._pack_pairs(batch, WIDTH)
    src, tgt, tgt_len = src.to(dev), tgt.to(dev), tgt_len.to(dev)
    leaves = {k: v.to(dt).clone().requires_grad_(True) for k, v in m.p.items()}
    td = HookDrop(d, 0, nb, dt, dev)
    _, c = regen_torch.score_forward(m, src, tgt, tgt_len, None, True, True, dt, leaves, td)
    w0 = torch.softmax((c + noise.to(dev, dt)) / tau, -1)
    ent = -(w0 * torch.log(w0 + 1e-12)).sum(-1)
    nll, _ = regen_torch.score_forward(m, src, tgt, tgt_len, w0[None], False, True, dt, leaves, td)
    g = good.to(dev, dt)
    ((nll[0].sum(-1) * g).sum() / n_tok + (ent * g).sum() / nb).backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    return grads, float(nll.detach().double().sum()) / n_tok, float(ent.detach().double().mean())


def one_step(nb, hook_masks):
    """steps 0, 1, 2 as they come, then step s = 3 on a settled batch of nb pairs: everything tests 2 and 3 compare, computed once"""
    if ("step", nb) in _cache:
        return _cache[("step", nb)]
    from dr4sr_amd.regen import RegenDropout
    from dr4sr_amd.regen_train import tau_at
    tr = make_trainer(batch_size=nb)
    for _ in range(3):
        tr.step()
    before = {k: getattr(tr, k).clone() for k in ("params", "adam_m", "adam_v")}
    m = fresh_model()                                # a model of its own with the parameters from before the step
    m.load_params(tr.state_dict())
    d = RegenDropout(0.5, SEED, 3)
    chosen, left_out = settle_batch(m, pool(), nb, d)
    assert tr.step(batch=chosen) == 3 and tr.tau == tau_at(4)
    out = {"trainer": tr, "before": before, "chosen": chosen, "left_out": left_out, "grad": tr.grad_view().clone(),
           "after": {k: getattr(tr, k).clone() for k in ("params", "adam_m", "adam_v", "grads")}}
    batch = [pool()[i] for i in chosen]
    toks = [len(t) + 1 for _, t in batch]
    n_tok, noise, tau = sum(toks), mirror_noise(3, nb), tau_at(3)
    good = torch.ones(nb)
    good[left_out] = 0
    for side, dt in (("r32", torch.float32), ("r64", torch.float64)):
        out[side] = torch_side(m, batch, good, n_tok, noise, tau, d, dt)
    # the trainer's gradient is the whole batch's: the left-out pairs' terms are taken off it, each from the HIP backward of that pair
    # alone under its slot's masks (pair0 = slot), brought to the batch's normalisation: its scalar there is
    # (n_tok_j / n_tok) x [CE_j + (n_tok / (n_tok_j n_batch)) x entropy_j]
    hip = {k: v.double().clone() for k, v in m.grads_from_flat(out["grad"]).items()}
    for j in left_out:
        r = m.loss_and_grad([batch[j]], "encoder", True, WIDTH, "hip", noise=noise[j:j + 1], tau=tau, entropy_weight=n_tok / (toks[j] * nb),
                            dropout=d, pair0=j)
        for k in hip:
            hip[k] -= r.grads[k].double() * (toks[j] / n_tok)
    out["hip"] = hip
    if not left_out:                                 # nothing left out: the written-out scalar is loss_and_grad's own
        r = m.loss_and_grad(batch, "encoder", True, WIDTH, "torch", torch.float64, noise=noise, tau=tau, entropy_weight=1.0, dropout=d)
        assert all(torch.equal(r.grads[k], out["r64"][0][k]) or float((r.grads[k] - out["r64"][0][k]).abs().max()) < 1e-12 for k in hip)
    _cache[("step", nb)] = out
    return out


@pytest.mark.parametrize("nb", [200, 300])
def test_one_step_has_the_gradient_loss_and_grad_describes(nb, hook_masks):
    """all 98 tensors of trainer.grad_view() after the backward of step 3 against float64 torch autograd of loss_and_grad's scalar on the
    same batch under the step's masks, noise and temperature; 300 pairs are two chunks (256 + 44).  Slots that sit near a ReLU step with
    every pair (settle_batch) are left out of the compared scalar on all three sides; the batch's loss and entropy are the whole batch's"""
    o = one_step(nb, hook_masks)
    tr = o["trainer"]
    hip = o["hip"]
    assert len(hip) == 98
    bad, worst, worst_k = [], 0.0, None
    for k, h in hip.items():
        r32, r64 = o["r32"][0][k].double(), o["r64"][0][k]
        e, dd = float((r32 - r64).abs().max()), float((h - r64).abs().max())
        ratio = dd / e if e > 0 else (0.0 if dd == 0 else float("inf"))
        if ratio > worst:
            worst, worst_k = ratio, k
        if dd > 16 * e:
            bad.append(f"{k}: |HIP - float64| {dd:.3e}, err32 {e:.3e}, ratio {ratio:.1f}")
    print(f"step 3, {nb} pairs ({len(o['left_out'])} left out): worst |HIP - float64| / err32_t over 98 tensors: {worst:.2f} ({worst_k})")
    assert not bad, "\n".join(bad)
    l64, ent64 = o["r64"][1], o["r64"][2]
    e = max(abs(o["r32"][1] - l64), 6e-8 * abs(l64))
    assert abs(float(tr.loss_log[3]) - l64) <= 16 * e, (float(tr.loss_log[3]), l64, e)
    e = max(abs(o["r32"][2] - ent64), 6e-8 * ent64)
    assert abs(float(tr.ent_log[3]) - ent64) <= 16 * e


@pytest.mark.parametrize("nb", [200, 300])
def test_adam_wiring_matches_torch_adam(nb, hook_masks):
    """the step's parameter update against torch.optim.Adam(lr_3, betas (0.9, 0.98), eps 1e-9) in fp32, applied to the parameters from
    before the step with the trainer's own gradient and moments: only the optimizer differs.  Bound: tests/test_gpu_api.py
    test_optimizer_choices_match_torch_optim's 3e-6 at lr 1e-2, scaled to this lr, plus one fp32 rounding of the parameter"""
    o = one_step(nb, hook_masks)
    tr, n = o["trainer"], o["trainer"].n_params
    lr3 = tr.lr_at(3)
    assert abs(lr3 - 1e-3 * (1 + np.cos(np.pi * 3 / 40)) / 2) < 1e-15
    p = torch.nn.Parameter(o["before"]["params"][:n].cpu().clone())
    opt = torch.optim.Adam([p], lr=lr3, betas=(0.9, 0.98), eps=1e-9, foreach=False)
    opt.state[p] = {"step": torch.tensor(3.0), "exp_avg": o["before"]["adam_m"][:n].cpu().clone(), "exp_avg_sq": o["before"]["adam_v"][:n].cpu().clone()}
    p.grad = o["grad"].cpu().clone()
    opt.step()
    got = o["after"]["params"][:n].cpu()
    diff = (got - p.detach()).abs()
    bound = 3e-4 * lr3 + 2.0 ** -23 * p.detach().abs()
    print(f"step 3, {nb} pairs: max |trainer - torch Adam| {float(diff.max()):.3e} (3e-4 lr = {3e-4 * lr3:.3e}); "
          f"max |update| {float((got - o['before']['params'][:n].cpu()).abs().max()):.3e}")
    assert bool((diff <= bound).all())
    assert float((o["after"]["adam_m"][:n].cpu() - opt.state[p]["exp_avg"]).abs().max()) <= 1e-6 * float(opt.state[p]["exp_avg"].abs().max())
    assert int(tr.state[0]) == 4 and not torch.equal(got, o["before"]["params"][:n].cpu())
    # the padding of all four buffers stays zero, the gradient's tail {1, 0, 0, 0}
    print(f"{n} parameters, padded to {tr.n_pad}")
    assert tr.n_pad % 4 == 0 and 0 <= tr.n_pad - n < 4
    for k in ("params", "adam_m", "adam_v", "grads"):
        assert not o["after"][k][n:tr.n_pad].any(), k
    assert o["after"]["grads"][tr.n_pad:].tolist() == [1.0, 0.0, 0.0, 0.0]
    # an id no pair holds: no gradient in four steps, so its row has not moved by a bit; its neighbour has
    E0 = fresh_model("cpu").p["item_embedding.weight"]
    sd = tr.state_dict()
    assert sd["item_embedding_decoder.weight"] is sd["item_embedding.weight"] and len(sd) == 99
    assert torch.equal(sd["item_embedding.weight"][FREE_ID].cpu(), E0[FREE_ID])
    assert not torch.equal(sd["item_embedding.weight"][TAKEN_ID].cpu(), E0[TAKEN_ID])
    assert not tr.model.grads_from_flat(o["grad"])["item_embedding.weight"][FREE_ID].any()
    # the model reads the master buffer, and sync() brings its named tensors to it
    assert tr.model.score_flat().data_ptr() == tr.params.data_ptr()
    tr.sync()
    assert torch.equal(tr.model.p["condition_linear.2.bias"], sd["condition_linear.2.bias"])
    assert torch.equal(tr.model.flat()[:N_ITEM * 64], sd["item_embedding.weight"].reshape(-1)[:N_ITEM * 64])


def test_a_step_at_learning_rate_zero_moves_the_moments_only():
    """CosineAnnealingLR(T_max = epochs) stepped per batch is exactly 0 at s = epochs"""
    tr = make_trainer(pairs=pool()[:256], batch_size=128, epochs=2)
    assert tr.lr_at(2) == 0.0 and tr.lr_at(0) == 1e-3
    tr.step()
    tr.step()
    before = {k: getattr(tr, k).clone() for k in ("params", "adam_m", "adam_v")}
    assert tr.step() == 2
    assert torch.equal(tr.params, before["params"])
    assert not torch.equal(tr.adam_m, before["adam_m"]) and not torch.equal(tr.adam_v, before["adam_v"])
    assert int(tr.state[0]) == 3
    tr.step()
    assert not torch.equal(tr.params, before["params"])
    with pytest.raises(RuntimeError):
        tr.step()


# ---------------------------------------------------------------------------------------------------- 4. trajectory
def torch_trajectory(dt, steps, batches, hook_masks):
    """the trainer's loop with loss_and_grad(backend="torch") and torch.optim.Adam in `dt`: the per-step CE values"""
    from dr4sr_amd.regen import RegenDropout
    from dr4sr_amd.regen_train import lr_at, tau_at
    m = fresh_model()
    m.p = {k: v.to(dt) for k, v in m.p.items()}                      # the master parameters in dt (loss_and_grad clones its leaves from them)
    params = [torch.nn.Parameter(v) for v in m.p.values()]
    opt = torch.optim.Adam(params, lr=1e-3, betas=(0.9, 0.98), eps=1e-9)
    losses = []
    for s in range(steps):
        batch = [pool()[i] for i in batches[s]]
        r = m.loss_and_grad(batch, "encoder", True, WIDTH, "torch", dt, noise=mirror_noise(s, len(batch)), tau=tau_at(s), entropy_weight=1.0,
                            dropout=RegenDropout(0.5, SEED, s))
        losses.append(float(r.loss))
        for g in opt.param_groups:
            g["lr"] = lr_at(s, 1e-3, 40)
        for p, k in zip(params, m.p):
            p.grad = r.grads[k].to(dt)
        opt.step()
        m._cast.clear()
    return losses


def test_trajectory_of_24_steps(hook_masks):
    """24 steps at batch 128 over the 512 pairs, epochs = 40, against the same loop in torch float64 and fp32 under the trainer's
    permutation, masks and noise.  Per step |HIP loss - float64 loss| <= 16 x |fp32 loss - float64 loss|, the unit floored at its mean
    over the 24 steps; and the loss falls (the torch backend alone gave 2.71 -> 2.37 on this model and these pairs)"""
    steps = 24
    tr = make_trainer(batch_size=128, epochs=40)
    batches = []
    for s in range(steps):
        batches.append(tr.next_batch_indices().tolist())
        assert tr.step(noise=mirror_noise(s, len(batches[-1]))) == s
    assert tr.epoch == 6 and tr.pos == 0 and sorted(sum(batches[:4], [])) == list(range(512)), "four batches are one epoch's shuffle"
    hip = tr.loss_log[:steps].double().cpu().tolist()
    l64 = torch_trajectory(torch.float64, steps, batches, hook_masks)
    l32 = torch_trajectory(torch.float32, steps, batches, hook_masks)
    unit = [abs(a - b) for a, b in zip(l32, l64)]
    floor = sum(unit) / steps
    bad = []
    for s in range(steps):
        e, dd = max(unit[s], floor), abs(hip[s] - l64[s])
        print(f"step {s:2d}: float64 {l64[s]:.6f}  HIP {hip[s]:.6f}  |HIP - float64| {dd:.2e}  |fp32 - float64| {unit[s]:.2e}  ratio {dd / e:.2f}")
        if dd > 16 * e:
            bad.append(s)
    first, last = sum(hip[:4]) / 4, sum(hip[-4:]) / 4
    print(f"mean loss of the first 4 steps {first:.4f}, of the last 4 {last:.4f}; unit floor {floor:.2e}")
    assert not bad, bad
    assert last < first


# ---------------------------------------------------------------------------------------------------- 5. bits
def bits_of(tr):
    return {k: getattr(tr, k).clone() for k in ("params", "adam_m", "adam_v", "loss_log", "ent_log")}


def test_same_seed_same_bits_and_resume_is_bit_exact():
    a, b = make_trainer(batch_size=128), make_trainer(batch_size=128)
    for _ in range(6):
        a.step()
        b.step()
    A, B = bits_of(a), bits_of(b)
    assert all(torch.equal(A[k], B[k]) for k in A)
    assert float(A["loss_log"][:6].min()) > 0 and not A["loss_log"][6:].any()
    c = make_trainer(batch_size=128)
    for _ in range(3):
        c.step()
    st = c.trainer_state()
    assert st["step"] == 3 and st["pos"] == 384 and st["epoch"] == 0
    r = make_trainer(batch_size=128)
    r.load_trainer_state(st)
    assert torch.equal(r.model.p["position_embedding.weight"], c.named_params()["position_embedding.weight"]), "the model holds the loaded values"
    for _ in range(3):
        r.step()
    R = bits_of(r)
    assert all(torch.equal(A[k], R[k]) for k in A), [k for k in A if not torch.equal(A[k], R[k])]
    assert (r.s, r.tau, r.epoch, r.pos) == (a.s, a.tau, a.epoch, a.pos) and int(r.state[0]) == 6
    other = make_trainer(batch_size=128, seed=SEED + 1)
    other.step()
    assert not torch.equal(other.loss_log[:1], A["loss_log"][:1])
    with pytest.raises(ValueError):
        make_trainer(batch_size=64).load_trainer_state(st)


def test_epoch_with_a_partial_last_batch():
    """512 pairs at batch 200: three steps of 200, 200 and 112 pairs; the epoch loss is the mean of the three batch values.  At lr = 0
    the parameters stand still, so each batch's log entries are what loss_and_grad(backend="hip") gives for that batch at that step:
    the partial batch is normalised by its own token and pair counts.  Bound: an fp32 sum of n terms in any order is within
    n 2^-24 of its value (n <= 3 800 token NLLs, <= 200 entropy terms); the two sides' noise differs in the last bit at most"""
    from dr4sr_amd.regen import RegenDropout
    from dr4sr_amd.regen_train import tau_at
    tr = make_trainer(batch_size=200, lr=0.0)
    assert tr.steps_per_epoch == 3
    batches = [tr.permutation(0)[a:a + 200].tolist() for a in (0, 200, 400)]
    assert [len(b) for b in batches] == [200, 200, 112]
    loss = tr.run_epoch()
    assert (tr.s, tr.epoch, tr.pos) == (3, 1, 0) and tr.epoch_losses == [loss]
    logs = tr.loss_log[:3].double().cpu()
    assert abs(loss - float(logs.sum()) / 3) <= 1e-12 and float(logs.min()) > 0
    m = fresh_model()
    for s, idx in enumerate(batches):
        r = m.loss_and_grad([pool()[i] for i in idx], "encoder", True, WIDTH, "hip", noise=mirror_noise(s, len(idx)), tau=tau_at(s),
                            entropy_weight=1.0, dropout=RegenDropout(0.5, SEED, s))
        print(f"batch {s} ({len(idx)} pairs): loss {float(logs[s]):.6f} / {float(r.loss):.6f}, entropy {float(tr.ent_log[s]):.6f} / {float(r.entropy):.6f}")
        assert abs(float(logs[s]) - float(r.loss)) <= 3800 * 2.0 ** -24 * float(r.loss)
        assert abs(float(tr.ent_log[s]) - float(r.entropy)) <= 200 * 2.0 ** -24 * float(r.entropy) + 1e-6
    assert torch.equal(tr.params[:tr.n_params], m.score_flat())


def test_dropout_zero_trains_in_eval_mode():
    """dropout = 0 goes through the same code to the eval entry points: step 0's loss is loss_and_grad's eval-mode loss"""
    tr = make_trainer(batch_size=128, dropout=0.0)
    idx = tr.next_batch_indices().tolist()
    tr.step()
    r = fresh_model().loss_and_grad([pool()[i] for i in idx], "encoder", True, WIDTH, "hip", noise=mirror_noise(0, 128), tau=1.0, entropy_weight=1.0)
    assert abs(float(tr.loss_log[0]) - float(r.loss)) <= 128 * 19 * 2.0 ** -24 * float(r.loss)
    dr = make_trainer(batch_size=128)
    dr.step()
    assert abs(float(dr.loss_log[0]) - float(tr.loss_log[0])) > 1e-3


# ---------------------------------------------------------------------------------------------------- 6. end to end
def test_command_line_end_to_end(tmp_path):
    from dr4sr_amd.regen import RegenModel
    from dr4sr_amd.regen_train import pretrain
    root = str(tmp_path)
    torch.save(pool(), os.path.join(root, "seq-pat-pair.pth"))
    E = 0.1 * torch.randn(N_ITEM, 64, generator=torch.Generator().manual_seed(2))
    torch.save({"parameters": {"item_embedding.weight": E}}, os.path.join(root, "pre-trained_embedding.ckpt"))
    cmd = [sys.executable, "-m", "dr4sr_amd.regen_train", "--root_path", root, "--epochs", "2", "--batch_size", "128", "--K", "5", "--seed", "3",
           "--state_out", os.path.join(root, "state.pth")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)        # a fresh child process, with a time limit
    assert out.returncode == 0, "rc=%s\n%s\n%s" % (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    lines = out.stdout.strip().splitlines()
    assert lines[0].startswith("Epoch: 1, Train loss: ") and lines[1].startswith("Epoch: 2, Train loss: ") and "Epoch time = " in lines[0]
    assert lines[-1] == os.path.join(root, "regenerator.pth")
    sd = torch.load(lines[-1], map_location="cpu")
    assert sd["item_embedding_decoder.weight"].data_ptr() == sd["item_embedding.weight"].data_ptr(), "the tables are saved tied"
    assert tuple(sd["item_embedding.weight"].shape) == (N_ITEM + 2, 64) and not torch.equal(sd["item_embedding.weight"][:N_ITEM], E), "trained rows"
    m = RegenModel.from_state_dict(sd, "cuda")
    assert m.has_condition_encoder and m.K == 5 and m.n_item == N_ITEM
    # the same run in this process: the child's file scores as the trainer's own model, bit for bit
    path, tr = pretrain(root, "again.pth", 5, 2, 3, 128, 0.5, "cuda", verbose=False)
    assert tr.s == 8 and len(tr.epoch_losses) == 2
    some = pool()[:64]
    a, b = m.score(some, "encoder", True, WIDTH), tr.model.score(some, "encoder", True, WIDTH)
    assert torch.equal(a.nll, b.nll) and torch.equal(a.cond_logits, b.cond_logits) and torch.isfinite(a.nll).all()
    st = torch.load(os.path.join(root, "state.pth"), map_location="cpu")
    assert st["step"] == 8 and torch.equal(st["params"], tr.params.cpu())
    toks = m.decode([[m.sos] + s + [m.eos] for s, _ in some[:8]])
    assert len(toks) == 8 * 5 and all(t[0] == m.sos and 2 <= len(t) <= 25 for t in toks)
