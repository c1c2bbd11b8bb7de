"""The float64 yardstick of the FMLP GPU tests (CPU, plain torch; test infrastructure, not product code).

oracle/fmlp_oracle.py in its rfft / irfft form (`use_fft=True`: the reference's own formula, module/layers.py:740-757) on float64 leaves: no
[B, L, L, D] tensor, so B = 1700 at L = 50 takes under a second.  tests/test_fmlp_oracle.py pins it, at every even L, to the oracle's
circular-convolution form in float64 (the form the HIP kernels implement) and to the fp32 oracle.
"""
from __future__ import annotations

import torch

from oracle import fmlp_oracle as FO

EPS = 1e-12
TABLE = "item_embedding.weight"


def _leaves(params):
    return {k: v.detach().to(torch.float64).clone().requires_grad_(True) for k, v in params.items()}


def _grads(leaf):
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items()}


def step_grads(params, batch, n_layer, masks=None, pdrop=0.0):
    """-> (loss, query, {name: gradient}) of FO.training_step(..., use_fft=True), everything in float64"""
    leaf = _leaves(params)
    loss, q, _, _ = FO.training_step(leaf, batch, n_layer, EPS, masks, pdrop, use_fft=True)
    loss.backward()
    return loss.detach(), q.detach(), _grads(leaf)


def encode_grads(params, idx, d_out, n_layer, masks=None, pdrop=0.0):
    """-> (out, {name: gradient}): FO.fmlp_encode(..., use_fft=True) and its autograd under d_out, in float64"""
    leaf = _leaves(params)
    out = FO.fmlp_encode(leaf, idx, n_layer, EPS, masks, pdrop, use_fft=True)
    out.backward(d_out.detach().cpu().to(torch.float64))
    return out.detach(), _grads(leaf)


def make_case(B, L, NL, N, seed):
    """-> (params, in_item_id [B, L], item_id [B], neg_item [B, 1]) built as tests/test_gpu_fmlp.py::_fmlp_case builds them (left-padded
    prefixes, LayerNorm weights 1 + 0.05 randn, the rest 0.05 randn, table row 0 zero), with these rows planted whenever B (and L) allow:
      row 0 full length | row 1 a single item | row 2 all PAD | row 3 a PAD id inside its valid range (L >= 4) | row 4 a PAD target |
      row 5 one id twice | rows 0 and 5 the same target"""
    from dr4sr_amd.fmlp_engine import fmlp_param_names, fmlp_param_shapes
    gen = torch.Generator().manual_seed(seed)
    idx = torch.zeros(B, L, dtype=torch.long)
    for i in range(B):
        n = int(torch.randint(1, L + 1, (1,), generator=gen))
        idx[i, L - n:] = torch.randint(1, N, (n,), generator=gen)
    tgt = torch.randint(1, N, (B,), generator=gen)
    neg = torch.randint(1, N, (B, 1), generator=gen)
    idx[0] = torch.randint(1, N, (L,), generator=gen)
    if B > 1:
        idx[1] = 0
        idx[1, L - 1] = int(torch.randint(1, N, (1,), generator=gen))
    if B > 2:
        idx[2] = 0
    if B > 3 and L >= 4:
        n = max(3, L // 2)
        idx[3] = 0
        idx[3, L - n:] = torch.randint(1, N, (n,), generator=gen)
        idx[3, L - 2] = 0
    if B > 4:
        tgt[4] = 0
    if B > 5:
        idx[5, L - 2:] = int(torch.randint(1, N, (1,), generator=gen))
        tgt[5] = tgt[0]
    params = {}
    for nme, shp in zip(fmlp_param_names(NL), fmlp_param_shapes(N, L, 64, 256, NL)):
        params[nme] = (1.0 if nme.endswith("LayerNorm.weight") else 0.0) + 0.05 * torch.randn(shp, generator=gen)
    params[TABLE][0] = 0
    return params, idx, tgt, neg
