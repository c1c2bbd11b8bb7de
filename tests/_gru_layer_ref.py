"""Float64 restatement of ONE GRU layer as torch.ops.dr4sr_hip.gru_layer states it (include/dr4sr_hip.h): torch.nn.GRU(bias=False,
batch_first=True) with h_0 = 0, gates r | z | n, plus the op's `seqlen` rule — the steps at and behind seqlen[b] (clamped to [0, L]) are
skipped, y and dx are zero there and dy there is ignored.  Gradients come from torch autograd in float64.

tests/test_gru_op_cpu.py pins this file to torch.nn.GRU and to oracle.gru4rec_oracle.gru_layer; tests/test_gpu_gru_op.py holds the HIP op
against it.

Inputs (make_case): weights uniform in +-WEIGHT_FACTOR / sqrt(H) and x from N(0, 1).  torch's own initialisation is the factor 1; at
N(0, 0.02) weights r and z stay within 0.5 +- 0.01, where a wrong gate derivative hides in the linear regime.  With the factor below the
float64 gates of every case reach below 0.2 and above 0.8 (asserted by the CPU test)."""
import math

import torch

WEIGHT_FACTOR = 3.0
SHAPES = [(1, 1, 64, 128), (5, 12, 64, 128), (17, 12, 128, 256), (5, 50, 256, 256), (3, 70, 64, 128)]     # (B, L, I, H) of the GPU tests
WIDTHS = [(i, h) for i in (64, 128, 256) for h in (128, 256)]


def clamp_len(seqlen, L):
    return seqlen.to(torch.int64).clamp(0, L)


def gru_layer(x, w_ih, w_hh, seqlen=None, gates=None):
    """-> y [B, L, H] in x's dtype; `gates`, a list, receives (r, z, valid [B] bool) per step"""
    B, L, _ = x.shape
    H = w_hh.shape[1]
    n = clamp_len(seqlen, L) if seqlen is not None else torch.full((B,), L, dtype=torch.int64)
    gi = x @ w_ih.T
    h = torch.zeros(B, H, dtype=x.dtype)
    out = []
    for t in range(L):
        gh = h @ w_hh.T
        r = torch.sigmoid(gi[:, t, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, t, H:2 * H] + gh[:, H:2 * H])
        c = torch.tanh(gi[:, t, 2 * H:] + r * gh[:, 2 * H:])
        valid = (t < n).unsqueeze(1)
        h = torch.where(valid, (1 - z) * c + z * h, h)
        out.append(torch.where(valid, h, torch.zeros_like(h)))
        if gates is not None:
            gates.append((r.detach(), z.detach(), valid.squeeze(1)))
    return torch.stack(out, 1)


def layer_grads(x, w_ih, w_hh, d_out, seqlen=None):
    """float64 -> (y, dx, dw_ih, dw_hh); d_out behind seqlen does not count (non-finite values there are dropped first)"""
    x, w_ih, w_hh = (t.detach().double().requires_grad_(True) for t in (x, w_ih, w_hh))
    y = gru_layer(x, w_ih, w_hh, seqlen)
    d = d_out.double()
    if seqlen is not None:
        L = x.shape[1]
        behind = torch.arange(L).unsqueeze(0) >= clamp_len(seqlen, L).unsqueeze(1)
        d = d.masked_fill(behind.unsqueeze(2), 0.0)
    dx, dw_ih, dw_hh = torch.autograd.grad(y, [x, w_ih, w_hh], d)
    return y.detach(), dx, dw_ih, dw_hh


def lengths(B, L):
    """lengths that include 0, 1, L - 1 and L where B and L have room for them, the others spread over [0, L]"""
    edge = [v for v in (L, 0, 1, L - 1) if 0 <= v <= L]
    edge = list(dict.fromkeys(edge))
    g = torch.Generator().manual_seed(900 + 7 * B + L)
    rest = torch.randint(0, L + 1, (max(B - len(edge), 0),), generator=g).tolist()
    return torch.tensor((edge + rest)[:B], dtype=torch.int64)


def make_case(B, L, I, H, seed=None, factor=WEIGHT_FACTOR):
    """-> (x, w_ih, w_hh, d_out) in float32"""
    g = torch.Generator().manual_seed(1000 + 31 * B + 7 * L + I + H if seed is None else seed)
    k = factor / math.sqrt(H)
    w_ih = (torch.rand(3 * H, I, generator=g) * 2 - 1) * k
    w_hh = (torch.rand(3 * H, H, generator=g) * 2 - 1) * k
    x = torch.randn(B, L, I, generator=g)
    d_out = torch.randn(B, L, H, generator=g)
    return x, w_ih, w_hh, d_out
