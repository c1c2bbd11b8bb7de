"""CPU checks of the FMLP ops (no GPU): the float64 yardstick helper against the oracle at every even L, the dispatcher registration with
fake kernels, the shape refusals of the size entry points, and the state-dict names of FMLPOps / FMLPEncoderOps."""
import pytest
import torch

import _fmlp_layer_ref as LR
import _fmlp_ref as FR
from oracle import fmlp_oracle as FO

E_ARG, E_SHAPE, E_WS = -1, -2, -3


@pytest.mark.parametrize("L", list(range(2, 65, 2)))
def test_helper_chained_over_the_layers_equals_the_oracle_in_float64(L):
    """x0, filter{i}, layer{i} and the query of oracle.fmlp_oracle.fmlp_encode(use_fft=True, return_all=True), with and without masks"""
    B, NL, N = 4, 2, 40
    params, idx, _, _ = FR.make_case(B, L, NL, N, seed=300 + L)
    p = {k: v.double() for k, v in params.items()}
    g = torch.Generator().manual_seed(L)
    masks = {s: (torch.rand(B, L, 64, generator=g) > 0.5).double() for s in range(1 + 2 * NL)}
    for m, pd in ((None, 0.0), (masks, 0.5)):
        q, acts = FO.fmlp_encode(p, idx, NL, LR.EPS, m, pd, use_fft=True, return_all=True)
        x = LR.embed_ln(p, idx, LR.EPS, m, pd)
        assert x.dtype == torch.float64 and torch.equal(x, acts["x0"])
        for i in range(NL):
            x, xf = LR.layer(x, p, LR.prefix(i), LR.EPS, m, i, pd, return_filter=True)
            assert torch.equal(xf, acts[f"filter{i}"]), (L, i)
            assert torch.equal(x, acts[f"layer{i}"]), (L, i)
        assert torch.equal(x[:, -1], q) and bool(torch.isfinite(q).all())


def test_fmlp_ops_are_registered_with_fake_kernels_and_refuse_cpu_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import dr4sr_amd.ops as ops
    from dr4sr_amd._lib import Dr4srError
    for n in ("fmlp_layer", "fmlp_layer_backward", "layer_norm", "layer_norm_backward"):
        assert n in ops.OPS and hasattr(torch.ops.dr4sr_hip, n), n
    o = torch.ops.dr4sr_hip
    B, L = 8, 50
    shapes = list(LR.layer_shapes(L))
    with FakeTensorMode():
        x = torch.empty(B, L, 64)
        w = [torch.empty(s) for s in shapes]
        y, saved = o.fmlp_layer(x, *w, 1e-12, 0.5, 7, 1, 0)
        assert y.shape == (B, L, 64) and y.dtype == torch.float32 and saved.dim() == 1 and saved.dtype == torch.float32
        assert saved.numel() == B * L * (2 * 64 + 256)
        gs = o.fmlp_layer_backward(x, *w, 1e-12, 0.5, 7, 1, 0, saved, torch.empty(B, L, 64))
        assert [tuple(g.shape) for g in gs] == [(B, L, 64)] + [tuple(s) for s in shapes]
        assert all(g.dtype == torch.float32 for g in gs)
        yn = o.layer_norm(x, w[1], w[2], 1e-12)
        assert yn.shape == (B, L, 64) and yn.dtype == torch.float32
        dx, dw, db = o.layer_norm_backward(x, w[1], 1e-12, torch.empty(B, L, 64))
        assert dx.shape == (B, L, 64) and dw.shape == (64,) and db.shape == (64,)
    w = [torch.zeros(s) for s in shapes]
    with pytest.raises(Dr4srError):
        o.fmlp_layer(torch.zeros(2, L, 64), *w, 1e-12, 0.0, 7, 1, 0)
    with pytest.raises(Dr4srError):
        o.fmlp_layer_backward(torch.zeros(2, L, 64), *w, 1e-12, 0.0, 7, 1, 0, torch.zeros(8), torch.zeros(2, L, 64))
    with pytest.raises(Dr4srError):
        o.layer_norm(torch.zeros(2, L, 64), w[1], w[2], 1e-12)
    with pytest.raises(Dr4srError):
        o.layer_norm_backward(torch.zeros(2, L, 64), w[1], 1e-12, torch.zeros(2, L, 64))


def test_size_entry_points_refuse_unsupported_shapes():
    from dr4sr_amd import _lib
    lib = _lib.load()
    for fn in (lib.dr4sr_fmlp_layer_saved_floats, lambda *a: lib.dr4sr_fmlp_layer_workspace_bytes(*a, 0),
               lambda *a: lib.dr4sr_fmlp_layer_workspace_bytes(*a, 1)):
        for L in range(2, 65, 2):
            assert fn(4, L, 64, 256) > 0, L
        assert fn(4, 49, 64, 256) == E_SHAPE and fn(4, 1, 64, 256) == E_SHAPE            # odd L
        assert fn(4, 66, 64, 256) == E_SHAPE and fn(4, 0, 64, 256) == E_SHAPE
        assert fn(4, 50, 128, 256) == E_SHAPE and fn(4, 50, 128, 512) == E_SHAPE         # D = 128
        assert fn(4, 50, 64, 128) == E_SHAPE                                              # F != 4 D
        assert fn(-1, 50, 64, 256) == E_ARG
    assert lib.dr4sr_fmlp_layer_saved_floats(3, 10, 64, 256) == 3 * 10 * (2 * 64 + 256)
    assert lib.dr4sr_fmlp_layer_saved_floats(0, 10, 64, 256) == 0
    small, big = lib.dr4sr_fmlp_layer_workspace_bytes(300, 50, 64, 256, 0), lib.dr4sr_fmlp_layer_workspace_bytes(300, 50, 64, 256, 1)
    assert 0 < small < big and big == lib.dr4sr_fmlp_layer_workspace_bytes(256, 50, 64, 256, 1)      # 256 gradient slots at most
    assert lib.dr4sr_layer_norm_workspace_bytes(7, 64) > 0
    assert lib.dr4sr_layer_norm_workspace_bytes(7, 66) == E_SHAPE and lib.dr4sr_layer_norm_workspace_bytes(7, 2048) == E_SHAPE
    assert lib.dr4sr_layer_norm_workspace_bytes(-1, 64) == E_ARG
    # the entry points answer before any launch: null pointers and bad shapes need no GPU
    assert lib.dr4sr_fmlp_layer_fwd(None, None, 1, 50, 64, 256, 1e-12, 0.0, 0, 0, 0, None, None, None, 0, None) == E_ARG
    assert lib.dr4sr_fmlp_layer_bwd(None, None, 1, 50, 64, 256, 1e-12, 0.0, 0, 0, 0, None, None, None, None, None, 0, None) == E_ARG
    assert lib.dr4sr_layer_norm_fwd(None, None, None, 1, 64, 1e-12, None, None) == E_ARG
    assert lib.dr4sr_layer_norm_bwd(None, None, 1, 64, 1e-12, None, None, None, None, None, 0, None) == E_ARG


def test_module_state_dict_carries_the_reference_names_and_loads_an_engine_checkpoint():
    from dr4sr_amd.fmlp_engine import fmlp_param_names, fmlp_param_shapes
    from dr4sr_amd.module.layers import FMLPEncoderOps, FMLPOps
    N, L, D, F, NL = 30, 50, 64, 256, 3
    want = dict(zip(fmlp_param_names(NL), fmlp_param_shapes(N, L, D, F, NL)))
    table = torch.nn.Embedding(N, D, padding_idx=0)
    m = FMLPOps(table, NL)
    sd = m.state_dict()
    assert set(sd) == set(want)
    for k, s in want.items():
        assert tuple(sd[k].shape) == tuple(s), k
    # a parameter dict in an FMLP checkpoint's layout loads with strict=True; the table is the one the module was handed
    g = torch.Generator().manual_seed(1)
    ckpt = {k: torch.randn(s, generator=g) for k, s in want.items()}
    m.load_state_dict(ckpt, strict=True)
    assert m.item_embedding is table and torch.equal(table.weight.detach(), ckpt["item_embedding.weight"])
    k = "item_encoder.layer.2.filterlayer.complex_weight"
    assert torch.equal(m.state_dict()[k], ckpt[k])
    rest = {k: v for k, v in ckpt.items() if k != "item_embedding.weight"}
    missing = m.load_state_dict(rest, strict=False)
    assert missing.missing_keys == ["item_embedding.weight"] and not missing.unexpected_keys
    assert m.step == 0 and m.seed == 2023 and m.p_drop == 0.5 and m.eps == 1e-12
    # the encoder alone: the reference's names under FMLPEncoder, and one initialisation copied into every layer (layers.py:796-798)
    enc = FMLPEncoderOps(num_hidden_layers=NL)
    pre = "item_encoder."
    assert set(enc.state_dict()) == {k[len(pre):] for k in want if k.startswith(pre)}
    cw = [l.filterlayer.complex_weight for l in enc.layer]
    assert cw[0].shape == (1, 26, 64, 2) and 0.015 < float(cw[0].detach().std()) < 0.025
    for l in enc.layer[1:]:
        for a, b in zip(enc.layer[0].tensors(), l.tensors()):
            assert torch.equal(a, b) and a is not b
    assert float(enc.layer[0].intermediate.LayerNorm.weight.detach().min()) == 1.0
