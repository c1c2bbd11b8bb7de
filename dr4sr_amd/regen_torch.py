"""The regenerator in eager torch: a batched restatement of the math of csrc/regen.hip (greedy decode) and csrc/regen_score*.hip
(teacher-forced scoring and, through autograd, its gradients).

It runs on CPU or GPU in fp32 or fp64 and is the cross-check of the kernels and the float64 side of every test, not a fall-back:
RegenModel reaches it only where the caller says backend="torch".  Functions over a RegenModel, or over a name -> tensor dict `p`
where the caller passes leaves; the module keeps no state.

One set of layer blocks (mha, ln, ffn, enc_layer, dec_layer) serves both paths.  `drop` is None (eval mode: every dropout site is the
identity, which is all that decoding uses) or a TorchDrop (train mode: the kernels' own masks at nn.Transformer's 30 dropout sites).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from . import regen_dropout
from .regen import D, H, LN_EPS, MAX_LEN, N_LAYER, ROWS_PER_TORCH, GradResult, _chunks
from .regen_dropout import STACK_COND, STACK_DEC, STACK_SRC, eval_mode


class TorchDrop:
    """the keep factors of one torch batch (global pairs pair0 .. pair0 + n - 1) as tensors, from the host mirror of the kernels'
    masks (regen_dropout.py); a site is "src_emb", "tgt_emb" or (stack, layer, kind)"""

    def __init__(self, dropout, pair0, n, dtype, device):
        self.d, self.pairs, self.dtype, self.device, self.cache = dropout, range(pair0, pair0 + n), dtype, device, {}

    @staticmethod
    def of(dropout, pair0, n, dtype, device):
        return None if eval_mode(dropout) else TorchDrop(dropout, pair0, n, dtype, device)

    def _get(self, fn, s, shape):
        sid = {"src_emb": regen_dropout.SITE_SRC_EMB, "tgt_emb": regen_dropout.SITE_TGT_EMB}[s] if isinstance(s, str) else regen_dropout.site(*s)
        key = (sid, shape)
        if key not in self.cache:
            self.cache[key] = torch.from_numpy(fn(self.d, sid, list(self.pairs), *shape)).to(device=self.device, dtype=self.dtype)
        return self.cache[key]

    def rows(self, s, x):
        return self._get(regen_dropout.keep_rows, s, tuple(x.shape[1:]))

    def probs(self, s, a):
        return self._get(regen_dropout.keep_probs, s, tuple(a.shape[2:]))


# ---------------------------------------------------------------------------------------------------- the layer blocks
def _rows(drop, x, s):
    return x if drop is None else x * drop.rows(s, x)


def _probs(drop, a, s):
    return a if drop is None else a * drop.probs(s, a)


def mha(p, pre, xq, xkv, bias, drop=None, st=None, l=None, kind=0):
    """nn.MultiheadAttention `pre` with the additive `bias` on the scores; dropout sites (st, l, kind) on the probabilities and
    (st, l, kind + 1) on the output"""
    W, b = p[pre + ".in_proj_weight"], p[pre + ".in_proj_bias"]
    B, Lq, _ = xq.shape
    Lk = xkv.shape[1]
    q = F.linear(xq, W[:D], b[:D]).view(B, Lq, H, D // H).transpose(1, 2)
    k = F.linear(xkv, W[D:2 * D], b[D:2 * D]).view(B, Lk, H, D // H).transpose(1, 2)
    v = F.linear(xkv, W[2 * D:], b[2 * D:]).view(B, Lk, H, D // H).transpose(1, 2)
    a = _probs(drop, torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(D // H) + bias, -1), (st, l, kind))
    o = (a @ v).transpose(1, 2).reshape(B, Lq, D)
    return _rows(drop, F.linear(o, p[pre + ".out_proj.weight"], p[pre + ".out_proj.bias"]), (st, l, kind + 1))


def ln(p, x, pre):
    return F.layer_norm(x, (D,), p[pre + ".weight"], p[pre + ".bias"], LN_EPS)


def ffn(p, x, pre, drop=None, st=None, l=None, kind=0):
    """linear2(gelu(linear1(x))); dropout sites (st, l, kind) on the hidden and (st, l, kind + 1) on the output"""
    hid = _rows(drop, F.gelu(F.linear(x, p[pre + ".linear1.weight"], p[pre + ".linear1.bias"])), (st, l, kind))
    return _rows(drop, F.linear(hid, p[pre + ".linear2.weight"], p[pre + ".linear2.bias"]), (st, l, kind + 1))


def enc_layer(p, pre, x, bias, drop=None, st=None, l=None):
    """one post-norm nn.TransformerEncoderLayer"""
    x = ln(p, x + mha(p, pre + ".self_attn", x, x, bias, drop, st, l, 0), pre + ".norm1")
    return ln(p, x + ffn(p, x, pre, drop, st, l, 2), pre + ".norm2")


def enc_layers(p, stem, x, bias, drop=None, st=None):
    for i in range(N_LAYER):
        x = enc_layer(p, f"{stem}.layers.{i}", x, bias, drop, st, i)
    return x


def dec_layer(p, pre, x, self_bias, mem, mem_bias, drop=None, l=None):
    """one post-norm nn.TransformerDecoderLayer: self attention, cross attention over `mem`, FFN"""
    x = ln(p, x + mha(p, pre + ".self_attn", x, x, self_bias, drop, STACK_DEC, l, 0), pre + ".norm1")
    x = ln(p, x + mha(p, pre + ".multihead_attn", x, mem, mem_bias, drop, STACK_DEC, l, 2), pre + ".norm2")
    return ln(p, x + ffn(p, x, pre, drop, STACK_DEC, l, 4), pre + ".norm3")


def dec_layers(p, x, self_bias, mem, mem_bias, drop=None):
    for i in range(N_LAYER):
        x = dec_layer(p, f"transformer.decoder.layers.{i}", x, self_bias, mem, mem_bias, drop, i)
    return x


# ---------------------------------------------------------------------------------------------------- greedy decode (fp32, eval mode)
def encode(model, src, lens):
    """encoder (no attention mask in the reference; key padding here only hides the batch's padding) + encoder.norm"""
    p = model.p
    Ls = src.shape[1]
    x = p["item_embedding.weight"][src] + p["position_embedding.weight"][:Ls]
    pad = torch.arange(Ls, device=src.device)[None, :] >= lens[:, None]
    kb = torch.zeros(pad.shape, device=src.device).masked_fill(pad, float("-inf"))[:, None, None, :]
    return ln(p, enc_layers(p, "transformer.encoder", x, kb), "transformer.encoder.norm"), kb


def greedy(model, src, mem, kb, gaps=None):
    """greedy_decode (3.Hybrid_inference.py:185-208) over a batch of rows, recomputing the whole prefix at each step.  `gaps`: a pair
    of [R, MAX_LEN - 1] tensors that receive, per step, best - second-best allowed logit and the best (the cross-checks' tie rule)"""
    p, dev = model.p, model.device
    E, P = p["item_embedding.weight"], p["position_embedding.weight"]
    R = src.shape[0]
    ys = torch.full((R, 1), model.sos, dtype=torch.int64, device=dev)
    alive = torch.ones(R, dtype=torch.bool, device=dev)
    n = torch.ones(R, dtype=torch.int32, device=dev)
    for i in range(MAX_LEN - 1):
        idx = alive.nonzero().squeeze(1)
        if idx.numel() == 0:
            break
        y = ys[idx]
        T = y.shape[1]
        causal = torch.full((T, T), float("-inf"), device=dev).triu(1)
        x = dec_layers(p, E[y] + P[:T], causal, mem[idx], kb[idx])
        logits = ln(p, x[:, -1], "transformer.decoder.norm") @ E.T
        if i <= 1:      # inference_mask: ids of src (the padding repeats SOS, which is in ys) and not in ys
            allowed = torch.zeros_like(logits, dtype=torch.bool).scatter(-1, src[idx], True)
        else:           # inference_mask_generative
            allowed = torch.ones_like(logits, dtype=torch.bool)
        allowed = allowed.scatter(-1, y, False)
        masked = logits.masked_fill(~allowed, float("-inf"))
        nxt = masked.argmax(-1)
        if gaps is not None:
            v = torch.topk(masked, 2, dim=-1).values
            gaps[0][idx, i] = v[:, 0] - v[:, 1]
            gaps[1][idx, i] = v[:, 0]
        col = torch.zeros(R, dtype=torch.int64, device=dev)
        col[idx] = nxt
        ys = torch.cat([ys, col[:, None]], 1)
        n[idx] += 1
        alive[idx] = nxt != model.eos
    out = torch.zeros(R, MAX_LEN, dtype=torch.int64, device=dev)
    out[:, :ys.shape[1]] = ys
    out[torch.arange(MAX_LEN, device=dev)[None, :] >= n[:, None].long()] = 0
    return out, n


def decode(model, src, lens, cond0, n_cond, rows_per_batch=ROWS_PER_TORCH, record=()):
    """tokens [n_cond * S, MAX_LEN] int64 and len [n_cond * S] int32 (condition-major), on the host: what RegenModel._decode_hip
    returns.  `record`: two host tensors [n_cond, S, MAX_LEN - 1] that receive greedy's `gaps` (NaN after the row ended), or none"""
    dev, p = model.device, model.p
    src, lens = src.to(dev), lens.to(dev)
    S = src.shape[0]
    mem0, kb0 = encode(model, src, lens)
    c1 = torch.relu(F.linear(mem0, p["condition_linear.0.weight"], p["condition_linear.0.bias"]))
    W2, b2 = p["condition_linear.2.weight"], p["condition_linear.2.bias"]
    toks, lns = [], []
    for c in range(n_cond):
        k = cond0 + c
        mem = F.linear(c1, W2[k * D:(k + 1) * D], b2[k * D:(k + 1) * D])       # features k*64:(k+1)*64 (3.Hybrid_inference.py:146)
        for a, b in _chunks(S, rows_per_batch):
            gaps = tuple(torch.full((b - a, MAX_LEN - 1), float("nan"), device=dev) for _ in record) if record else None
            t, n = greedy(model, src[a:b], mem[a:b], kb0[a:b], gaps)
            toks.append(t)
            lns.append(n)
            for r, g in zip(record, gaps or ()):
                r[c, a:b] = g.cpu()
    return torch.cat(toks).cpu(), torch.cat(lns).cpu()


# ---------------------------------------------------------------------------------------------------- teacher-forced scoring
def score_forward(model, src, tgt, tgt_len, w, want_cond, causal_source, dtype, params=None, drop=None):
    """Generator.forward + cross_entropy(reduction='none') of 2.Pretrain_regenerator.py, batched, from the named parameters:
    (nll [n_w, n, T] or None when w is None, condition logits [n, K] or None).  `params` (name -> tensor of `dtype` on src's
    device) replaces the model's own: loss_and_grad passes leaves that require grad.  drop=None is eval mode; a TorchDrop is
    train mode"""
    dev = src.device
    p = model._params_as(dtype, dev) if params is None else params
    E, P = p["item_embedding.weight"], p["position_embedding.weight"]
    n, Ls = src.shape
    T = tgt.shape[1] - 1
    tgt_in, tgt_out = tgt[:, :-1], tgt[:, 1:]
    ninf = float("-inf")

    def key_bias(ids):
        return torch.zeros(ids.shape, dtype=dtype, device=dev).masked_fill(ids == 0, ninf)[:, None, None, :]

    def causal(L):
        return torch.full((L, L), ninf, dtype=dtype, device=dev).triu(1)

    tgt_kb = key_bias(tgt_in)
    x_t = _rows(drop, E[tgt_in] + P[:T], "tgt_emb")
    cond = None
    if want_cond:
        y = enc_layers(p, "condition_encoder.encoder", x_t, causal(T) + tgt_kb, drop, STACK_COND)
        keep = torch.arange(T, device=dev)[None, :] < tgt_len[:, None]
        pooled = (y * keep[:, :, None].to(dtype)).sum(1) / tgt_len[:, None].to(dtype)
        hid = torch.relu(F.linear(pooled, p["condition_encoder.condition_layer.0.weight"], p["condition_encoder.condition_layer.0.bias"]))
        cond = F.linear(hid, p["condition_encoder.condition_layer.2.weight"], p["condition_encoder.condition_layer.2.bias"])
    if w is None:
        return None, cond
    src_kb = key_bias(src)
    x = enc_layers(p, "transformer.encoder", _rows(drop, E[src] + P[:Ls], "src_emb"), (causal(Ls) if causal_source else 0) + src_kb,
                   drop, STACK_SRC)
    mem = ln(p, x, "transformer.encoder.norm")
    c1 = torch.relu(F.linear(mem, p["condition_linear.0.weight"], p["condition_linear.0.bias"]))
    mem = F.linear(c1, p["condition_linear.2.weight"], p["condition_linear.2.bias"]).view(n, Ls, model.K, D)
    dup = ((src[:, :, None] == src[:, None, :]) & torch.ones(Ls, Ls, dtype=torch.bool, device=dev).tril(-1)).any(-1)   # id seen earlier
    Es = E[src]                                                           # the only table rows the masked logits keep
    hit = (tgt_out[:, :, None] == src[:, None, :]) & ~dup[:, None, :]     # [n, T, Ls]: the slot of the target id, if any
    dec_bias = causal(T) + tgt_kb
    out = []
    for wi in w.to(device=dev, dtype=dtype):
        h = ln(p, dec_layers(p, x_t, dec_bias, (mem * wi[:, None, :, None]).sum(-2), src_kb, drop), "transformer.decoder.norm")
        lg = (h @ Es.transpose(1, 2)).masked_fill(dup[:, None, :], ninf)
        lse = torch.logsumexp(lg, -1)
        tl = torch.where(hit, lg, torch.zeros((), dtype=dtype, device=dev)).sum(-1)
        nll = torch.where(hit.any(-1), lse - tl, torch.full((), float("inf"), dtype=dtype, device=dev))
        out.append(nll.masked_fill(tgt_out == 0, 0.0))
    return torch.stack(out), cond


def score(model, src, tgt, tgt_len, w, causal_source, dtype, dropout, pair0):
    """the backend="torch" half of RegenModel.score on packed pairs: the lists of per-chunk nll [n_w, rows, T] and condition
    logits [rows, K], on the host (w=None: the condition encoder's own softmax weighs the memories)"""
    dev = model.device
    nll, cond = [], []
    for a, b in _chunks(src.shape[0], ROWS_PER_TORCH):
        s_d, t_d, tl_d = src[a:b].to(dev).contiguous(), tgt[a:b].to(dev).contiguous(), tgt_len[a:b].to(dev).contiguous()
        wc = None if w is None else w[:, a:b]
        c = None
        td = TorchDrop.of(dropout, pair0 + a, b - a, dtype, dev)
        if wc is None:
            _, c = score_forward(model, s_d, t_d, tl_d, None, True, causal_source, dtype, None, td)
            wc = torch.softmax(c, -1)[None]
        x, c2 = score_forward(model, s_d, t_d, tl_d, wc, model.has_condition_encoder and c is None, causal_source, dtype, None, td)
        c = c2 if c is None else c
        nll.append(x.cpu())
        if c is not None:
            cond.append(c.cpu())
    return nll, cond


def loss_and_grad(model, src, tgt, tgt_len, conditions, causal_source, dtype, noise, tau, entropy_weight, dropout, pair0):
    """the backend="torch" half of RegenModel.loss_and_grad on packed, validated pairs: autograd through score_forward"""
    dev = model.device
    n = src.shape[0]
    encoder = isinstance(conditions, str)
    n_tok = max(int((tgt[:, 1:] != 0).sum()), 1)
    leaves = {k: v.to(device=dev, dtype=dtype).clone().requires_grad_(True) for k, v in model.p.items()}
    loss = torch.zeros((), dtype=torch.float64)
    entropy = torch.zeros((), dtype=torch.float64)
    dws, conds = [], []
    for a, b in _chunks(n, ROWS_PER_TORCH):
        s_d, t_d, tl_d = src[a:b].to(dev), tgt[a:b].to(dev), tgt_len[a:b].to(dev)
        ent = None
        td = TorchDrop.of(dropout, pair0 + a, b - a, dtype, dev)
        if encoder:
            _, c = score_forward(model, s_d, t_d, tl_d, None, True, causal_source, dtype, leaves, td)
            z = c if noise is None else c + torch.as_tensor(noise)[a:b].to(dev, dtype)
            w0 = torch.softmax(z / tau, -1)
            ent = -(w0 * torch.log(w0 + 1e-12)).sum(-1).sum() / n
            w = w0[None]                                          # its .grad is the cross entropy's alone: what the kernels call dw
        else:
            c = None
            w = conditions[:, a:b].to(dev, dtype).clone().requires_grad_(True)
        w.retain_grad()
        nll, c2 = score_forward(model, s_d, t_d, tl_d, w, model.has_condition_encoder and c is None, causal_source, dtype, leaves, td)
        ce = nll.sum() / n_tok
        (ce if ent is None else ce + entropy_weight * ent).backward()
        loss += float(ce.detach())
        if ent is not None:
            entropy += float(ent.detach())
        dws.append(w.grad.detach())
        c = c2 if c is None else c
        if c is not None:
            conds.append(c.detach())
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    n_w = 1 if encoder else conditions.shape[0]
    return GradResult(loss, entropy if encoder else None, grads,
                      torch.cat(dws, 1) if dws else torch.zeros(n_w, 0, model.K, dtype=dtype, device=dev),
                      torch.cat(conds) if conds else None)


def condition_grad(model, tgt, tgt_len, dlogits, names, dtype, dropout, pair0):
    """the backend="torch" half of RegenModel.condition_grad on packed targets: autograd of sum(cond_logits * dlogits)"""
    dev = model.device
    leaves = {k: v.to(device=dev, dtype=dtype).clone().requires_grad_(k in names) for k, v in model.p.items()}
    for a, b in _chunks(tgt.shape[0], ROWS_PER_TORCH):
        _, c = score_forward(model, tgt[a:b, :1].to(dev), tgt[a:b].to(dev), tgt_len[a:b].to(dev), None, True, True, dtype, leaves,
                             TorchDrop.of(dropout, pair0 + a, b - a, dtype, dev))
        (c * dlogits[a:b].to(dev, dtype)).sum().backward()
    return {k: (leaves[k].grad if leaves[k].grad is not None else torch.zeros_like(leaves[k])) for k in names}
