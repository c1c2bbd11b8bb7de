"""The float64 yardstick of the FMLP op tests (CPU, plain torch; test infrastructure, not product code).

One FMLP `Layer` in the reference's own rfft / irfft form (module/layers.py:740-791) with explicit keep masks, and the embedding LayerNorm
of model/fmlp.py:18-27, both with autograd.  tests/test_fmlp_op_cpu.py pins the helper, chained over the layers, to
oracle.fmlp_oracle.fmlp_encode(..., use_fft=True) at every even L from 2 to 64.

Parameters are keyed as an FMLP checkpoint keys them (`item_encoder.layer.{i}.filterlayer.complex_weight`, ...); masks as the oracle keys
them (oracle.fmlp_oracle.site)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import fmlp_oracle as FO

EPS = 1e-12
D, FF = 64, 256
LAYER_TENSORS = ("filterlayer.complex_weight", "filterlayer.LayerNorm.weight", "filterlayer.LayerNorm.bias", "intermediate.dense_1.weight",
                 "intermediate.dense_1.bias", "intermediate.dense_2.weight", "intermediate.dense_2.bias", "intermediate.LayerNorm.weight",
                 "intermediate.LayerNorm.bias")


def prefix(i):
    return f"item_encoder.layer.{i}."


def layer_shapes(L):
    return ((1, L // 2 + 1, D, 2), (D,), (D,), (FF, D), (FF,), (D, FF), (D,), (D,), (D,))


def layer_params(n_layer, L, seed):
    """0.05 randn weights, 1 + 0.05 randn LayerNorm weights (as tests/_fmlp_ref.make_case builds them)"""
    g = torch.Generator().manual_seed(seed)
    p = {}
    for i in range(n_layer):
        for n, s in zip(LAYER_TENSORS, layer_shapes(L)):
            p[prefix(i) + n] = (1.0 if n.endswith("LayerNorm.weight") else 0.0) + 0.05 * torch.randn(s, generator=g)
    return p


def make_x(B, L, seed):
    """[B, L, 64] randn with one all-zero row (when the batch has a second position to hold it)"""
    x = torch.randn(B, L, D, generator=torch.Generator().manual_seed(seed))
    if B > 0 and L > 1:
        x[0, 1] = 0
    return x


def _drop(x, masks, s, p):
    if masks is None or p == 0.0:
        return x
    return x * masks[s].to(x.dtype) / (1.0 - p)


def layer(x, p, pre, eps=EPS, masks=None, i=0, pdrop=0.0, return_filter=False):
    """FilterLayer then Intermediate on x [B, L, D]; masks {site: keep [B, L, D]}"""
    L = x.shape[1]
    cw = p[pre + "filterlayer.complex_weight"]
    f = torch.fft.irfft(torch.fft.rfft(x, dim=1, norm="ortho") * torch.view_as_complex(cw.contiguous()), n=L, dim=1, norm="ortho")
    f = _drop(f, masks, FO.site(FO.SITE_FILT, i), pdrop)
    xf = F.layer_norm(f + x, (x.shape[2],), p[pre + "filterlayer.LayerNorm.weight"], p[pre + "filterlayer.LayerNorm.bias"], eps)
    h = F.gelu(xf @ p[pre + "intermediate.dense_1.weight"].T + p[pre + "intermediate.dense_1.bias"])
    o = h @ p[pre + "intermediate.dense_2.weight"].T + p[pre + "intermediate.dense_2.bias"]
    o = _drop(o, masks, FO.site(FO.SITE_FFN, i), pdrop)
    y = F.layer_norm(o + xf, (x.shape[2],), p[pre + "intermediate.LayerNorm.weight"], p[pre + "intermediate.LayerNorm.bias"], eps)
    return (y, xf) if return_filter else y


def embed_ln(p, idx, eps=EPS, masks=None, pdrop=0.0):
    """model/fmlp.py:18-27: LayerNorm(item + position) and the embedding dropout"""
    E, P = p["item_embedding.weight"], p["position_embeddings.weight"]
    x = F.embedding(idx, E, padding_idx=0) + P[:idx.shape[1]].unsqueeze(0)
    x = F.layer_norm(x, (E.shape[1],), p["LayerNorm.weight"], p["LayerNorm.bias"], eps)
    return _drop(x, masks, FO.SITE_EMB, pdrop)


def _f64(t):
    return t.detach().cpu().to(torch.float64).clone().requires_grad_(True)


def layer_grads(x, p, d_out, n_layer=1, eps=EPS, masks=None, pdrop=0.0):
    """-> (y, dx, {name: gradient}) of n_layer chained layers under d_out, everything in float64"""
    xo = _f64(x)
    leaf = {k: _f64(v) for k, v in p.items()}
    y = xo
    for i in range(n_layer):
        y = layer(y, leaf, prefix(i), eps, masks, i, pdrop)
    y.backward(d_out.detach().cpu().to(torch.float64))
    return y.detach(), xo.grad, {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items()}


def layer_norm_grads(x, w, b, d_out, eps=EPS):
    """-> (y, dx, dw, db) of F.layer_norm over the last dimension, in float64"""
    xo, wo, bo = _f64(x), _f64(w), _f64(b)
    y = F.layer_norm(xo, (xo.shape[-1],), wo, bo, eps)
    y.backward(d_out.detach().cpu().to(torch.float64))
    return y.detach(), xo.grad, wo.grad, bo.grad
