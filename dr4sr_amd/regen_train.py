"""Pre-training of the regenerator — stage 2 of DR4SR (the reference's 2.Pretrain_regenerator.py:257-307) on the GPU.

    model = RegenModel.from_state_dict(init_state_dict(pretrained_item_embedding, K=5, seed=2024), "cuda")
    trainer = RegenTrainer(model, pairs, epochs=40)         # pairs: what `python -m dr4sr_amd.pairs` wrote (seq-pat-pair.pth)
    trainer.fit()                                           # the reference's line per epoch
    torch.save(trainer.state_dict(), "regenerator.pth")     # what `python -m dr4sr_amd.regen` and the reference's stage 3 load

    python -m dr4sr_amd.regen_train --root_path dataset/amazon-toys/toy/ --K 5 --epochs 40

One step is: the batch's rows gathered on the device; per chunk of at most SCORE_BWD_PAIRS_PER_CALL pairs the condition encoder
(dr4sr_regen_score_condition[_train]), the condition head (csrc/regen_head.hip: Gumbel-softmax weights, entropy, dnll), the
teacher-forced forward and backward (dr4sr_regen_score_bwd[_train]), the head's backward and the condition encoder's backward; then
dr4sr_adam_flat over the flat parameter buffer.  Nothing inside a step waits for the device: the token count comes from the host copy
of the lengths, the loss and entropy go to device logs that are read once per epoch.

What is restated and what is the project's own: the loss, the optimizer, tau_s = max(0.995^s, 0.1), the learning rate
lr (1 + cos(pi s / epochs)) / 2 stepped PER BATCH (CosineAnnealingLR(T_max = epochs) as the reference steps it: period 2 epochs
batches, exactly 0 at odd multiples of `epochs`) and the batching (256, shuffled, the last batch partial) are the reference's.  The random
streams are the project's: the shuffle is a seeded CPU torch.Generator permutation per epoch, the dropout masks and the Gumbel noise
are the Philox streams of regen_dropout.py — not torch's CUDA generator, so a run does not reproduce the reference's numbers sample for
sample, only its distribution.
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
import os
import time

import torch

from . import _lib
from .regen import (D, FF, N_LAYER, N_POS, SCORE_BWD_PAIRS_PER_CALL, RegenDropout, RegenModel, param_names, score_param_names,
                    score_param_shapes)

HEAD_KMAX = 8
TAU_DECAY, TAU_MIN = 0.995, 0.1


def lr_at(s: int, lr: float, epochs: int) -> float:
    """the learning rate of global step s: CosineAnnealingLR(T_max = epochs, eta_min = 0) stepped once per batch, in closed form"""
    return lr * (1.0 + math.cos(math.pi * s / epochs)) / 2.0


def tau_at(s: int) -> float:
    """the Gumbel-softmax temperature of global step s: 1 at s = 0, multiplied by 0.995 after each forward, floor 0.1 (Python doubles)"""
    tau = 1.0
    for _ in range(s):
        tau = max(tau * TAU_DECAY, TAU_MIN)
    return tau


def head_fwd_device(cond_logits, T: int, tau: float, n_tok: int, *, noise=None, seed: int = 0, step: int = 0, pair0: int = 0,
                    want_noise: bool = False):
    """csrc/regen_head.hip forward on device tensors: cond_logits [n, K] -> (w [1, n, K], ent [n], dnll [1, n, T], the noise used or None).
    Only enqueues on the current stream"""
    n, K = cond_logits.shape
    dev = cond_logits.device
    w = torch.empty(1, n, K, dtype=torch.float32, device=dev)
    ent = torch.empty(n, dtype=torch.float32, device=dev)
    dnll = torch.empty(1, n, T, dtype=torch.float32, device=dev)
    used = torch.empty(n, K, dtype=torch.float32, device=dev) if want_noise else None
    if noise is not None and (tuple(noise.shape) != (n, K) or noise.dtype != torch.float32):
        raise ValueError(f"noise of shape {tuple(noise.shape)} / {noise.dtype}, expected ({n}, {K}) fp32")
    _lib.check(_lib.load().dr4sr_regen_head_fwd(_lib.ptr(cond_logits), _lib.ptr(noise), n, K, T, float(tau), int(n_tok),
                                                C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_uint32(int(step) & 0xFFFFFFFF), int(pair0),
                                                _lib.ptr(w), _lib.ptr(ent), _lib.ptr(dnll), _lib.ptr(used), _lib.cur_stream()),
               "dr4sr_regen_head_fwd")
    return w, ent, dnll, used


def head_bwd_device(dw, w, ent, nll, tau: float, entropy_weight: float, n_batch: int, n_tok: int, loss_log=None, ent_log=None, slot: int = 0):
    """csrc/regen_head.hip backward on device tensors: dw [1, n, K], the forward's w and ent -> dlogits [n, K]; adds this call's share of
    the step's loss and entropy to loss_log[slot] / ent_log[slot] when given.  Only enqueues on the current stream"""
    n, K = w.shape[-2:]
    T = nll.shape[-1] if nll is not None else 1
    for log in (loss_log, ent_log):
        if log is not None and not (0 <= slot < log.numel()):
            raise IndexError(f"log slot {slot} outside [0, {log.numel()})")
    dlogits = torch.empty(n, K, dtype=torch.float32, device=w.device)
    _lib.check(_lib.load().dr4sr_regen_head_bwd(_lib.ptr(dw), _lib.ptr(w), _lib.ptr(ent), _lib.ptr(nll), n, K, T, float(tau),
                                                float(entropy_weight), int(n_batch), int(n_tok), _lib.ptr(dlogits), _lib.ptr(loss_log),
                                                _lib.ptr(ent_log), int(slot), _lib.cur_stream()), "dr4sr_regen_head_bwd")
    return dlogits


def init_state_dict(pretrained_item_embedding, K: int = 5, seed: int = 2024):
    """an initial regenerator state dict in the reference's names, drawn from the DISTRIBUTIONS of the reference's initial state (not
    its RNG stream): nn.Linear weights, the attention out_proj's included, N(0, 0.02^2) with zero biases (normal_initialization);
    LayerNorm 1 / 0; position_embedding N(0, 0.02^2); the MHA in_proj_weight's are bare parameters normal_initialization never visits:
    torch's xavier-uniform, bound sqrt(6 / (64 + 192)), in_proj_bias 0; the table is the pretrained rows followed by two N(0, 0.02^2)
    rows for SOS and EOS (2.Pretrain_regenerator.py:159-178)"""
    E = torch.as_tensor(pretrained_item_embedding).detach().to("cpu", torch.float32)
    if E.dim() != 2 or E.shape[1] != D or E.shape[0] < 1:
        raise ValueError(f"pretrained item embedding of shape {tuple(E.shape)}, expected [n_item, {D}]")
    if not (1 <= int(K) <= HEAD_KMAX):
        raise ValueError(f"K must be in 1..{HEAD_KMAX}, not {K!r}")
    g = torch.Generator().manual_seed(int(seed))
    n_rows = E.shape[0] + 2
    bound = math.sqrt(6.0 / (D + 3 * D))
    sd = {}
    for name, shape in zip(score_param_names(), score_param_shapes(n_rows, int(K))):
        leaf = name.rsplit(".", 1)[-1]
        if name == "item_embedding.weight":
            sd[name] = torch.cat([E, 0.02 * torch.randn(2, D, generator=g)])
        elif "norm" in name.split(".")[-2]:
            sd[name] = torch.ones(shape) if leaf == "weight" else torch.zeros(shape)
        elif leaf == "in_proj_weight":
            sd[name] = (2.0 * torch.rand(shape, generator=g) - 1.0) * bound
        elif leaf in ("bias", "in_proj_bias"):
            sd[name] = torch.zeros(shape)
        else:
            sd[name] = 0.02 * torch.randn(shape, generator=g)
    sd["item_embedding_decoder.weight"] = sd["item_embedding.weight"]
    return sd


class RegenTrainer:
    """the reference's pre-training loop over a RegenModel's flat parameter buffer (module docstring)"""

    def __init__(self, model: RegenModel, pairs, *, epochs: int = 40, batch_size: int = 256, lr: float = 1e-3, betas=(0.9, 0.98),
                 eps: float = 1e-9, dropout: float = 0.5, entropy_weight: float = 1.0, seed: int = 2024, causal_source: bool = True,
                 width=None):
        if not isinstance(model, RegenModel) or not model.has_condition_encoder:
            raise ValueError("pre-training needs condition_encoder.* and this model has none")
        if model.K > HEAD_KMAX:
            raise ValueError(f"K = {model.K}: the condition head is built for K <= {HEAD_KMAX}")
        if int(epochs) < 1 or int(batch_size) < 1 or len(pairs) < 1:
            raise ValueError("epochs, batch_size and the number of pairs must be positive")
        RegenDropout(dropout)                                        # its range check
        self.model, self.device = model, model.device
        self.epochs, self.batch_size, self.lr = int(epochs), int(batch_size), float(lr)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.dropout, self.entropy_weight, self.seed, self.causal_source = float(dropout), float(entropy_weight), int(seed), bool(causal_source)
        # ---- data: packed once at the file-wide widths, validated once, on the device once
        src, src_len, tgt, tgt_len, self.Ls, self.T = model._pack_pairs(pairs, width)
        self.n = len(pairs)
        _validate_targets(src, tgt, tgt_len)
        self.n_tok = (tgt[:, 1:] != 0).sum(1)                        # host copy: a batch's token count never comes from the device
        dev = self.device
        self.src, self.src_len, self.tgt, self.tgt_len = (t.to(dev).contiguous() for t in (src, src_len, tgt, tgt_len))
        self.steps_per_epoch = (self.n + self.batch_size - 1) // self.batch_size
        # ---- buffers: dr4sr_adam_flat takes n % 4 == 0 and reads a 4-float tail behind the gradient; the 98-tensor layout ends in a
        # [K] bias, so all four buffers are padded to a multiple of 4 and the model's score_flat() becomes a view of the padded master
        flat = model.score_flat()
        self.n_params = flat.numel()
        self.n_pad = (self.n_params + 3) // 4 * 4
        self.params = torch.zeros(self.n_pad, dtype=torch.float32, device=dev)
        self.params[:self.n_params] = flat
        model.adopt_score_flat(self.params[:self.n_params])
        self.grads = torch.zeros(self.n_pad + _lib.GRAD_TAIL, dtype=torch.float32, device=dev)
        self.grads[self.n_pad] = 1.0                                 # the tail {normaliser 1 (the gradient is already the mean's), 0, poison 0, 0}
        self.adam_m = torch.zeros(self.n_pad, dtype=torch.float32, device=dev)
        self.adam_v = torch.zeros(self.n_pad, dtype=torch.float32, device=dev)
        self.state = torch.zeros(_lib.STATE_WORDS, dtype=torch.int32, device=dev)
        self.loss_log = torch.zeros(self.epochs * self.steps_per_epoch, dtype=torch.float32, device=dev)
        self.ent_log = torch.zeros_like(self.loss_log)
        lib = _lib.load()
        plan = model.score_plan()
        nc = min(self.batch_size, SCORE_BWD_PAIRS_PER_CALL, self.n)
        sizes = (lib.dr4sr_regen_score_bwd_workspace_bytes(C.byref(plan), nc, self.Ls, self.T, 1),
                 max(lib.dr4sr_regen_score_condition_bwd_workspace_bytes(C.byref(plan), nc, self.T),
                     lib.dr4sr_regen_score_workspace_bytes(C.byref(plan), nc, 1, self.T, 1)))
        for nb in sizes:
            if nb < 0:
                _lib.check(int(nb), "the regenerator's workspace queries")
        self._ws = torch.empty(int(sizes[0]), dtype=torch.uint8, device=dev)
        self._ws_cond = torch.empty(int(sizes[1]), dtype=torch.uint8, device=dev)
        self.s, self.tau, self.epoch, self.pos = 0, 1.0, 0, 0        # global step, its temperature, the epoch and the position inside it
        self._perm_epoch, self._perm, self._perm_dev = -1, None, None
        self.epoch_losses = []

    # ------------------------------------------------------------------------------------------------ the schedules and the shuffle
    def lr_at(self, s: int) -> float:
        return lr_at(s, self.lr, self.epochs)

    def permutation(self, epoch: int):
        """the epoch's shuffle: a CPU torch.Generator permutation seeded by (seed, epoch) — the project's own stream"""
        g = torch.Generator().manual_seed((self.seed * 1000003 + int(epoch)) & 0x7FFFFFFFFFFFFFFF)
        return torch.randperm(self.n, generator=g)

    def next_batch_indices(self):
        """the pair indices (CPU int64) the next step() takes"""
        if self._perm_epoch != self.epoch:
            self._perm = self.permutation(self.epoch)
            self._perm_dev = self._perm.to(self.device)
            self._perm_epoch = self.epoch
        return self._perm[self.pos:self.pos + self.batch_size]

    def grad_view(self):
        """the flat gradient of the last step's backward (98-tensor score layout; model.grads_from_flat names it)"""
        return self.grads[:self.n_params]

    # ------------------------------------------------------------------------------------------------ one batch
    def step(self, noise=None, batch=None):
        """one batch: forward, backward and Adam, enqueued on the current stream; nothing is read back.  `noise` (recorded [n_batch, K]
        fp32) replaces the generated Gumbel noise and `batch` (pair indices) the shuffle's batch: both are for tests.  Returns the
        global step index s the batch ran as (its loss is loss_log[s])"""
        m, dev, s = self.model, self.device, self.s
        if s >= self.loss_log.numel():
            raise RuntimeError(f"all {self.epochs} epochs have run")
        idx = self.next_batch_indices()
        idx_dev = self._perm_dev[self.pos:self.pos + self.batch_size]
        if batch is not None:
            idx = torch.as_tensor(batch, dtype=torch.int64).reshape(-1).cpu()
            if idx.numel() < 1 or int(idx.min()) < 0 or int(idx.max()) >= self.n:
                raise IndexError(f"batch indices outside [0, {self.n})")
            idx_dev = idx.to(dev)
        nb = idx.numel()
        n_tok = max(int(self.n_tok[idx].sum()), 1)
        if noise is not None:
            noise = torch.as_tensor(noise)
            if tuple(noise.shape) != (nb, m.K):
                raise ValueError(f"noise of shape {tuple(noise.shape)}, expected ({nb}, {m.K})")
            noise = noise.to(dev, torch.float32).contiguous()
        src, src_len, tgt, tgt_len = (t.index_select(0, idx_dev) for t in (self.src, self.src_len, self.tgt, self.tgt_len))
        self.loss_log[s:s + 1].zero_()
        self.ent_log[s:s + 1].zero_()
        drop = RegenDropout(self.dropout, self.seed, s)
        grad = self.grad_view()
        for a in range(0, nb, SCORE_BWD_PAIRS_PER_CALL):
            b = min(nb, a + SCORE_BWD_PAIRS_PER_CALL)
            s_c, sl_c, t_c, tl_c = (t[a:b] for t in (src, src_len, tgt, tgt_len))          # row slices of contiguous matrices
            c = m.condition_device(t_c, tl_c, self._ws_cond, drop, a)
            w, ent, dnll, _ = head_fwd_device(c, self.T, self.tau, n_tok, noise=None if noise is None else noise[a:b], seed=self.seed,
                                              step=s, pair0=a)
            _, dw, nll = m.score_bwd_device(s_c, sl_c, t_c, tl_c, w, dnll, self.causal_source, grad, a > 0, self._ws, drop, a)
            dlog = head_bwd_device(dw, w, ent, nll, self.tau, self.entropy_weight, nb, n_tok, self.loss_log, self.ent_log, s)
            m.condition_bwd_device(t_c, tl_c, dlog, grad, True, self._ws_cond, drop, a)
        _lib.check(_lib.load().dr4sr_adam_flat(_lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(self.adam_m), _lib.ptr(self.adam_v),
                                               self.n_pad, _lib.ptr(self.state), self.lr_at(s), self.betas[0], self.betas[1], self.eps, 0.0,
                                               _lib.cur_stream()), "dr4sr_adam_flat")
        self.s = s + 1
        self.tau = max(self.tau * TAU_DECAY, TAU_MIN)
        if batch is None:
            self.pos += nb
            if self.pos >= self.n:
                self.epoch, self.pos = self.epoch + 1, 0
        return s

    # ------------------------------------------------------------------------------------------------ the epoch loop
    def run_epoch(self):
        """the current epoch (what is left of it after a resume); returns the mean of ALL its per-batch CE values, the reference's
        epoch loss: one read of the device log"""
        if self.epoch >= self.epochs:
            raise RuntimeError(f"all {self.epochs} epochs have run")
        s0, epoch = self.s - (self.pos + self.batch_size - 1) // self.batch_size, self.epoch
        while self.epoch == epoch:
            self.step()
        loss = float(self.loss_log[s0:self.s].double().mean())
        self.epoch_losses.append(loss)
        return loss

    def fit(self, verbose: bool = True):
        """the epochs that are left; prints the reference's line per epoch and returns the list of all epoch losses"""
        while self.epoch < self.epochs:
            t0 = time.perf_counter()
            loss = self.run_epoch()
            if verbose:
                print(f"Epoch: {self.epoch}, Train loss: {loss:.3f}, Epoch time = {time.perf_counter() - t0:.3f}s", flush=True)
        self.sync()
        return list(self.epoch_losses)

    # ------------------------------------------------------------------------------------------------ parameters out and in
    def named_params(self):
        """state-dict name -> a view of the master buffer"""
        return self.model.grads_from_flat(self.params[:self.n_params])

    @torch.no_grad()
    def sync(self):
        """bring trainer.model (self.p, the dtype casts and the decode layout's flat buffer) to the trained values"""
        self.model.load_params({k: v.clone() for k, v in self.named_params().items()})
        return self.model

    def state_dict(self):
        """the trained parameters under the reference's names (fp32 clones); item_embedding_decoder.weight IS item_embedding.weight"""
        sd = {k: v.clone() for k, v in self.named_params().items()}
        sd["item_embedding_decoder.weight"] = sd["item_embedding.weight"]
        return sd

    def trainer_state(self):
        """everything a fresh trainer over the same model shape, pairs and settings needs to continue bit-exactly (CPU tensors)"""
        return {"params": self.params.cpu(), "adam_m": self.adam_m.cpu(), "adam_v": self.adam_v.cpu(), "loss_log": self.loss_log.cpu(),
                "ent_log": self.ent_log.cpu(), "step": self.s, "tau": self.tau, "epoch": self.epoch, "pos": self.pos,
                "epoch_losses": list(self.epoch_losses), "seed": self.seed, "n_pairs": self.n, "batch_size": self.batch_size,
                "epochs": self.epochs}

    @torch.no_grad()
    def load_trainer_state(self, st: dict):
        for k in ("seed", "n_pairs", "batch_size", "epochs"):
            if st[k] != {"seed": self.seed, "n_pairs": self.n, "batch_size": self.batch_size, "epochs": self.epochs}[k]:
                raise ValueError(f"the saved state was made with {k} = {st[k]}")
        if st["params"].numel() != self.n_pad:
            raise ValueError(f"the saved state holds {st['params'].numel()} parameters, this model {self.n_pad}")
        for name in ("params", "adam_m", "adam_v", "loss_log", "ent_log"):
            getattr(self, name).copy_(st[name])
        self.s, self.tau, self.epoch, self.pos = int(st["step"]), float(st["tau"]), int(st["epoch"]), int(st["pos"])
        self.epoch_losses = list(st["epoch_losses"])
        self.state.zero_()
        self.state[_lib.STATE_STEP] = self.s                         # Adam's t = state[STEP] + 1
        self.sync()


def _validate_targets(src, tgt, tgt_len):
    """a target id that is not in its source row makes the reference's loss inf: ValueError, as RegenModel.loss_and_grad"""
    T1 = tgt.shape[1]
    live = (torch.arange(T1)[None, :] < tgt_len[:, None]) & (torch.arange(T1)[None, :] >= 1)
    for a in range(0, src.shape[0], 4096):
        hit = (tgt[a:a + 4096, :, None] == src[a:a + 4096, None, :]).any(-1)
        bad = (live[a:a + 4096] & ~hit).any(1).nonzero()
        if bad.numel():
            raise ValueError(f"pair {a + int(bad[0])}: a target id is not in its source (the reference's loss is inf there)")


def pretrain(root_path: str, output_name: str | None = None, K: int = 5, epochs: int = 40, seed: int = 2024, batch_size: int = 256,
             dropout: float = 0.5, device="cuda", state_in: str | None = None, state_out: str | None = None, verbose: bool = True):
    """2.Pretrain_regenerator.py's __main__: reads seq-pat-pair.pth and pre-trained_embedding.ckpt under root_path, trains, writes the
    state dict; returns (output path, trainer)"""
    pairs = torch.load(os.path.join(root_path, "seq-pat-pair.pth"))
    saved = torch.load(os.path.join(root_path, "pre-trained_embedding.ckpt"), map_location="cpu")
    model = RegenModel.from_state_dict(init_state_dict(saved["parameters"]["item_embedding.weight"], K, seed), device)
    trainer = RegenTrainer(model, pairs, epochs=epochs, batch_size=batch_size, dropout=dropout, seed=seed)
    if state_in:
        trainer.load_trainer_state(torch.load(state_in, map_location="cpu"))
    trainer.fit(verbose)
    out_path = os.path.join(root_path, output_name or "regenerator.pth")
    sd = {k: v.cpu() for k, v in trainer.state_dict().items() if k != "item_embedding_decoder.weight"}
    sd["item_embedding_decoder.weight"] = sd["item_embedding.weight"]          # saved tied, as the reference's state dict holds them
    torch.save(sd, out_path)
    if state_out:
        torch.save(trainer.trainer_state(), state_out)
    return out_path, trainer


def main(argv=None):
    ap = argparse.ArgumentParser(description="DR4SR stage 2: pre-train the regenerator on seq-pat-pair.pth and write regenerator.pth")
    ap.add_argument("--root_path", type=str, default="./dataset/amazon-toys/toy/", help="The path to the training dataset.")
    ap.add_argument("--output_name", type=str, default=None, help="The name of the pre-trained regenerator.")
    ap.add_argument("--K", type=int, default=5, help="The diversity factor for the diversity promoter.")
    ap.add_argument("--epochs", type=int, default=40, help="Training epochs of the regenerator.")
    ap.add_argument("--gpu_id", type=int, default=0)
    ap.add_argument("--seed", type=int, default=2024, help="Random seed.")
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--dropout", type=float, default=0.5, help="0 trains in eval mode")
    ap.add_argument("--state_in", type=str, default=None, help="continue from a trainer state written by --state_out")
    ap.add_argument("--state_out", type=str, default=None, help="also write the trainer state (parameters, moments, position)")
    a = ap.parse_args(argv)
    torch.cuda.set_device(a.gpu_id)
    path, _ = pretrain(a.root_path, a.output_name, a.K, a.epochs, a.seed, a.batch_size, a.dropout, torch.device("cuda", a.gpu_id),
                       a.state_in, a.state_out)
    print(path)


if __name__ == "__main__":
    main()
