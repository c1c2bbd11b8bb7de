"""What torch.ops.dr4sr_hip.gru_layer promises, checked without a GPU: the float64 helper of the GPU tests (tests/_gru_layer_ref.py) is
torch.nn.GRU(bias=False, batch_first=True) and the oracle's gru_layer; its seqlen rule is nn.GRU on each row's prefix and zeros behind it;
the GPU tests' inputs leave the gates' linear regime; fake kernels, shape refusals of the size entry points, the modules' state-dict keys
and constructor refusals."""
import numpy as np
import pytest
import torch

import dr4sr_amd.ops as ops
import _gru_layer_ref as GR
from oracle import gru4rec_oracle as GO


def torch_gru(x, w_ih, w_hh):
    """torch.nn.GRU(bias=False, batch_first=True) in float64 with the given weights"""
    m = torch.nn.GRU(x.shape[2], w_hh.shape[1], 1, bias=False, batch_first=True).double()
    with torch.no_grad():
        m.weight_ih_l0.copy_(w_ih)
        m.weight_hh_l0.copy_(w_hh)
    return m


def close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("I,H", GR.WIDTHS)
@pytest.mark.parametrize("L", [1, 2, 7])
def test_helper_is_torch_gru_and_the_oracle(I, H, L):
    x, w_ih, w_hh, d_out = (t.double() for t in GR.make_case(3, L, I, H))
    y, dx, dwi, dwh = GR.layer_grads(x, w_ih, w_hh, d_out)
    m = torch_gru(x, w_ih, w_hh)
    xr = x.clone().requires_grad_(True)
    y_t, h_t = m(xr)
    g = torch.autograd.grad(y_t, [xr, m.weight_ih_l0, m.weight_hh_l0], d_out)
    assert close(y, y_t.detach()) and close(dx, g[0]) and close(dwi, g[1]) and close(dwh, g[2])
    assert close(y[:, -1], h_t[0].detach())
    assert close(y, GO.gru_layer(x, w_ih, w_hh))


@pytest.mark.parametrize("I,H", [(64, 128), (256, 256)])
def test_seqlen_is_the_gru_of_each_prefix_and_zero_behind_it(I, H):
    B, L = 6, 7
    x, w_ih, w_hh, d_out = (t.double() for t in GR.make_case(B, L, I, H))
    seqlen = torch.tensor([7, 0, 1, 6, 3, 9])                # 9 is clamped to L
    dirty = d_out.clone()
    for b in range(B):
        dirty[b, min(int(seqlen[b]), L):] = float("nan")    # what lies behind a length is ignored
    y, dx, dwi, dwh = GR.layer_grads(x, w_ih, w_hh, dirty, seqlen)
    m = torch_gru(x, w_ih, w_hh)
    dx_t, dwi_t, dwh_t = torch.zeros_like(x), torch.zeros_like(w_ih), torch.zeros_like(w_hh)
    for b in range(B):
        n = min(int(seqlen[b]), L)
        assert float(y[b, n:].abs().max() if n < L else 0.0) == 0.0 and float(dx[b, n:].abs().max() if n < L else 0.0) == 0.0
        if n == 0:
            continue
        xb = x[b:b + 1, :n].clone().requires_grad_(True)
        yb, _ = m(xb)
        g = torch.autograd.grad(yb, [xb, m.weight_ih_l0, m.weight_hh_l0], d_out[b:b + 1, :n])
        assert close(y[b, :n], yb[0].detach())
        dx_t[b, :n] = g[0][0]
        dwi_t += g[1]
        dwh_t += g[2]
    assert close(dx, dx_t) and close(dwi, dwi_t) and close(dwh, dwh_t)
    # no seqlen: all L steps
    assert close(GR.gru_layer(x, w_ih, w_hh, torch.full((B,), L)), GR.gru_layer(x, w_ih, w_hh))


@pytest.mark.parametrize("shape", GR.SHAPES)
def test_gpu_test_inputs_leave_the_linear_regime_of_the_gates(shape):
    """every GPU case, with and without its lengths: r and z of the float64 helper go below 0.2 and above 0.8 at computed steps"""
    B, L, I, H = shape
    x, w_ih, w_hh, _ = (t.double() for t in GR.make_case(B, L, I, H))
    for seqlen in (None, GR.lengths(B, L)):
        if seqlen is not None and int(seqlen.max()) == 0:
            continue
        gates = []
        GR.gru_layer(x, w_ih, w_hh, seqlen, gates)
        r = torch.cat([r[v].flatten() for r, _, v in gates])
        z = torch.cat([z[v].flatten() for _, z, v in gates])
        for name, t in (("r", r), ("z", z)):
            assert float(t.min()) < 0.2 and float(t.max()) > 0.8, (shape, name, float(t.min()), float(t.max()))
    sl = GR.lengths(B, L)
    want = {v for v in (0, 1, L - 1, L)} if B >= 4 else {L}
    assert want <= set(sl.tolist()) and sl.shape == (B,)


def test_ops_are_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    for n in ("gru_layer", "gru_layer_backward"):
        assert n in ops.OPS and hasattr(torch.ops.dr4sr_hip, n), n
    o = torch.ops.dr4sr_hip
    with FakeTensorMode():
        x, wi, wh = torch.empty(5, 12, 64), torch.empty(384, 64), torch.empty(384, 128)
        for sl in (None, torch.empty(5, dtype=torch.int64)):
            y, saved = o.gru_layer(x, wi, wh, sl)
            assert y.shape == (5, 12, 128) and y.dtype == torch.float32 and saved.shape == (5 * 12 * 4 * 128,) and saved.dtype == torch.float32
            dx, dwi, dwh = o.gru_layer_backward(x, wi, wh, sl, y, saved, torch.empty(5, 12, 128))
            assert dx.shape == x.shape and dwi.shape == wi.shape and dwh.shape == wh.shape
            assert dx.dtype == dwi.dtype == dwh.dtype == torch.float32
    with pytest.raises(Exception):
        o.gru_layer(torch.zeros(5, 12, 64), torch.zeros(384, 64), torch.zeros(384, 128), None)      # no CPU kernel


def test_size_entry_points_refuse_unsupported_shapes():
    from dr4sr_amd import _lib
    lib = _lib.load()
    E_SHAPE = -2
    assert lib.dr4sr_gru_layer_saved_floats(5, 12, 64, 128) == 5 * 12 * 4 * 128
    for I, H in GR.WIDTHS:
        for L in (1, 1024):
            assert lib.dr4sr_gru_layer_saved_floats(3, L, I, H) == 3 * L * 4 * H
            for backward in (0, 1):
                assert lib.dr4sr_gru_layer_workspace_bytes(3, L, I, H, backward) >= 3 * L * 3 * H * 4
    assert lib.dr4sr_gru_layer_saved_floats(0, 12, 64, 128) == 0
    assert lib.dr4sr_gru_layer_workspace_bytes(0, 12, 64, 128, 0) == 0 and lib.dr4sr_gru_layer_workspace_bytes(0, 12, 64, 128, 1) == 0
    assert lib.dr4sr_gru_layer_bwd(8, 8, 8, None, 0, 12, 64, 128, None, None, None, None, None, 8, None, 0, None) == -1      # dw_ih is null
    for B, L, I, H in ((5, 12, 32, 128), (5, 12, 64, 64), (5, 12, 64, 192), (5, 0, 64, 128), (5, 1025, 64, 128)):
        assert lib.dr4sr_gru_layer_saved_floats(B, L, I, H) == E_SHAPE, (B, L, I, H)
        for backward in (0, 1):
            assert lib.dr4sr_gru_layer_workspace_bytes(B, L, I, H, backward) == E_SHAPE, (B, L, I, H)
        # ... and the calls, before anything is read or launched (the pointers are never dereferenced)
        assert lib.dr4sr_gru_layer_fwd(8, 8, 8, None, B, L, I, H, 8, None, 8, 1 << 40, None) == E_SHAPE
        assert lib.dr4sr_gru_layer_bwd(8, 8, 8, None, B, L, I, H, 8, 8, 8, 8, 8, 8, 8, 1 << 40, None) == E_SHAPE
    assert lib.dr4sr_gru_layer_saved_floats(-1, 12, 64, 128) == -1
    # B * L * 3H passes 2^31 well inside the supported range: the sizes are 64-bit
    assert lib.dr4sr_gru_layer_saved_floats(8192, 1024, 256, 256) == 8192 * 1024 * 4 * 256


def test_module_state_dict_is_the_reference_checkpoint(golden_dir):
    from dr4sr_amd.module.layers import GRU4RecQueryEncoderOps
    z = np.load(golden_dir + "/gru4rec_d64.npz")
    want = {k[len("param.query_encoder."):]: z[k].shape for k in z.files if k.startswith("param.query_encoder.")}
    N, D, H, NL = int(z["meta.num_items"]), int(z["meta.embed_dim"]), int(z["meta.hidden_size"]), int(z["meta.layer_num"])
    table = torch.nn.Embedding(N, D, padding_idx=0)
    m = GRU4RecQueryEncoderOps("item_id", table, H, NL, 0.2, 50)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == want and len(want) == 3 + 2 * NL
    m.load_state_dict({k: torch.from_numpy(z["param.query_encoder." + k]) for k in want}, strict=True)
    assert torch.equal(table.weight.detach(), torch.from_numpy(z["param.item_embedding.weight"]))     # 0.1 is the caller's table
    # torch's own GRU initialisation: uniform within +- 1 / sqrt(hidden)
    fresh = GRU4RecQueryEncoderOps("item_id", table, H, NL, 0.2, 50)
    for k, v in fresh.state_dict().items():
        if ".gru." in k:
            assert float(v.abs().max()) <= H ** -0.5 and float(v.std()) > 0.4 * H ** -0.5, k


def test_refused_constructor_arguments_raise():
    from dr4sr_amd.module.layers import GRULayerOps
    GRULayerOps(64, 128, 2, return_hidden=True)
    for kw in ({"bias": True}, {"batch_first": False}, {"bidirectional": True}):
        with pytest.raises(NotImplementedError, match="bias=False, batch_first=True"):
            GRULayerOps(64, 128, **kw)
