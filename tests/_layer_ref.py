"""CPU torch yardstick of torch.ops.dr4sr_hip.sasrec_layer: oracle.sasrec_oracle.sasrec_layer restated with a general mask.

`layer(x, key_pad, p, pre, H, eps, causal, ...)` is the oracle's function line for line; only the mask line differs (causal is a flag,
key_pad may be None), and a query row that admits no key gets a zero attention context, the op's rule (include/dr4sr_hip.h), where the
oracle's softmax would yield NaN.  With causal=True and every row admitting a key the two are the same arithmetic on the same operands:
tests/test_layer_op_cpu.py holds them equal bit for bit, and the oracle itself is pinned to the reference's recorded numbers
(tests/test_oracle_golden.py).  nn.TransformerEncoderLayer in eval mode is NOT a yardstick: its fast path zero-fills padded rows."""
import math

import torch
import torch.nn.functional as F

from oracle import sasrec_oracle as O

LAYER_TENSORS = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
                 "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")


def layer(x, key_pad, p, pre, H, eps, causal=True, masks=None, layer=0, pdrop=0.0):
    B, L, D = x.shape
    dh = D // H
    qkv = x @ p[pre + "self_attn.in_proj_weight"].T + p[pre + "self_attn.in_proj_bias"]
    q, k, v = qkv.split(D, dim=-1)
    q = q.view(B, L, H, dh).transpose(1, 2)
    k = k.view(B, L, H, dh).transpose(1, 2)
    v = v.view(B, L, H, dh).transpose(1, 2)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
    bias = torch.triu(torch.ones(L, L, dtype=torch.bool), 1) if causal else torch.zeros(L, L, dtype=torch.bool)
    bias = bias.view(1, 1, L, L)
    if key_pad is not None:
        bias = bias | key_pad.view(B, 1, 1, L)
    bias = bias.expand(B, 1, L, L)
    dead = bias.all(-1, keepdim=True)                       # no admissible key: a zero context instead of softmax's NaN
    s = s.masked_fill(bias & ~dead, float("-inf"))
    a = torch.softmax(s, dim=-1)
    a = a.masked_fill(dead, 0.0)
    a = O._drop(a, masks, O.site(O.SITE_ATTN, layer), pdrop)
    ctx = (a @ v).transpose(1, 2).reshape(B, L, D)
    o = ctx @ p[pre + "self_attn.out_proj.weight"].T + p[pre + "self_attn.out_proj.bias"]
    o = O._drop(o, masks, O.site(O.SITE_PROJ, layer), pdrop)
    y = F.layer_norm(x + o, (D,), p[pre + "norm1.weight"], p[pre + "norm1.bias"], eps)
    h = F.gelu(y @ p[pre + "linear1.weight"].T + p[pre + "linear1.bias"])
    h = O._drop(h, masks, O.site(O.SITE_ACT, layer), pdrop)
    f = h @ p[pre + "linear2.weight"].T + p[pre + "linear2.bias"]
    f = O._drop(f, masks, O.site(O.SITE_FFN, layer), pdrop)
    return F.layer_norm(y + f, (D,), p[pre + "norm2.weight"], p[pre + "norm2.bias"], eps)


def pool(x, seqlen, pooling):
    """tests/_inw_ref.py's pooling formulas; a row with seqlen 0 pools to zeros"""
    B, L, D = x.shape
    keep = (torch.arange(L).view(1, L) < seqlen.view(B, 1)).unsqueeze(-1)
    if pooling == "origin":
        return torch.where(keep, x, torch.zeros((), dtype=x.dtype))
    if pooling == "last":
        out = x[torch.arange(B), (seqlen - 1).clamp(min=0)]
        return torch.where(seqlen.view(B, 1) > 0, out, torch.zeros((), dtype=x.dtype))
    if pooling == "mean":
        out = torch.where(keep, x, torch.zeros((), dtype=x.dtype)).sum(1) / seqlen.clamp(min=1).view(B, 1).to(x.dtype)
        return out
    raise ValueError(pooling)


def layer_params(D, Fh, n_layer, seed):
    """{`layers.i.` + name: tensor} for n_layer layers, scaled like tests/test_gpu_input_weight.py's random_params"""
    gen = torch.Generator().manual_seed(seed)
    shapes = {"self_attn.in_proj_weight": (3 * D, D), "self_attn.in_proj_bias": (3 * D,), "self_attn.out_proj.weight": (D, D),
              "self_attn.out_proj.bias": (D,), "linear1.weight": (Fh, D), "linear1.bias": (Fh,), "linear2.weight": (D, Fh),
              "linear2.bias": (D,), "norm1.weight": (D,), "norm1.bias": (D,), "norm2.weight": (D,), "norm2.bias": (D,)}
    p = {}
    for i in range(n_layer):
        for n in LAYER_TENSORS:
            if n in ("norm1.weight", "norm2.weight"):
                t = 1.0 + 0.1 * torch.randn(shapes[n], generator=gen)
            elif n == "self_attn.in_proj_weight":
                t = 0.15 * torch.randn(shapes[n], generator=gen)
            else:
                t = 0.05 * torch.randn(shapes[n], generator=gen)
            p[f"layers.{i}.{n}"] = t
    return p


def layer_grads(x, key_pad, p, H, eps, causal, d_out, n_layer=1, masks=None, pdrop=0.0):
    """-> (y, dx, {name: gradient}) of n_layer layers (prefixes `layers.i.`) under <y, d_out>"""
    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    xl = x.detach().clone().requires_grad_(True)
    y = xl
    for i in range(n_layer):
        y = layer(y, key_pad, leaf, f"layers.{i}.", H, eps, causal, masks, i, pdrop)
    names = list(leaf)
    gs = torch.autograd.grad(y, [xl] + [leaf[k] for k in names], d_out)
    return y.detach(), gs[0].detach(), {k: g.detach() for k, g in zip(names, gs[1:])}
