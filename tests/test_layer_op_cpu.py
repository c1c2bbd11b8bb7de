"""CPU checks of the encoder-layer ops (no GPU): the yardstick helper against the oracle, the dispatcher registration with fake kernels,
the state-dict names of SASRecQueryEncoderOps, and the shape refusals of the size entry points."""
import pytest
import torch

import _layer_ref as LR
from oracle import sasrec_oracle as O

H, EPS = 2, 1e-12


@pytest.mark.parametrize("D,F", [(64, 128), (128, 128)])
def test_helper_equals_the_oracle_bit_for_bit_when_causal(D, F):
    B, L = 4, 12
    g = torch.Generator().manual_seed(D)
    p = LR.layer_params(D, F, 1, seed=3)
    x = torch.randn(B, L, D, generator=g)
    key_pad = torch.zeros(B, L, dtype=torch.bool)
    key_pad[1, 5:] = True                                    # post-padded
    key_pad[2, 6] = True                                     # a padded key inside a valid range
    masks = {O.site(s, 0): (torch.rand(shape, generator=g) > 0.5).float()
             for s, shape in ((O.SITE_ATTN, (B, H, L, L)), (O.SITE_PROJ, (B, L, D)), (O.SITE_ACT, (B, L, F)), (O.SITE_FFN, (B, L, D)))}
    for m, pd in ((None, 0.0), (masks, 0.5)):
        ref = O.sasrec_layer(x, key_pad, p, "layers.0.", H, EPS, m, 0, pd)
        got = LR.layer(x, key_pad, p, "layers.0.", H, EPS, True, m, 0, pd)
        assert not torch.isnan(ref).any() and torch.equal(got, ref)
    # a row that admits no key: the oracle yields NaN there, the helper a finite row; every other row is untouched
    key_pad[3, :] = True
    ref = O.sasrec_layer(x, key_pad, p, "layers.0.", H, EPS)
    got = LR.layer(x, key_pad, p, "layers.0.", H, EPS, True)
    assert torch.isnan(ref[3]).all() and torch.isfinite(got).all() and torch.equal(got[:3], ref[:3])
    # bidirectional and mask-free forms differ from the causal one
    assert not torch.equal(LR.layer(x, None, p, "layers.0.", H, EPS, False), LR.layer(x, None, p, "layers.0.", H, EPS, True))


def test_new_ops_are_registered_with_fake_kernels_and_refuse_cpu_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import dr4sr_amd.ops as ops
    from dr4sr_amd._lib import Dr4srError, POOL_LAST, POOL_MEAN, POOL_ORIGIN
    new = ("sasrec_layer", "sasrec_layer_backward", "seq_pool", "seq_pool_backward", "dropout", "embed_gather_posadd_backward")
    for n in new:
        assert n in ops.OPS and hasattr(torch.ops.dr4sr_hip, n), n
    o = torch.ops.dr4sr_hip
    B, L, D, F = 8, 50, 64, 256
    shapes = [(3 * D, D), (3 * D,), (D, D), (D,), (F, D), (F,), (D, F), (D,), (D,), (D,), (D,), (D,)]
    with FakeTensorMode():
        x = torch.empty(B, L, D)
        w = [torch.empty(s) for s in shapes]
        y, saved = o.sasrec_layer(x, torch.empty(B, L, dtype=torch.bool), True, *w, 2, 1e-12, 0.5, 7, 1, 0)
        assert y.shape == (B, L, D) and y.dtype == torch.float32 and saved.dim() == 1 and saved.dtype == torch.float32
        assert saved.numel() == B * (L * (6 * D + F) + 2 * L * L)
        y2, _ = o.sasrec_layer(x, None, False, *w, 2, 1e-12, 0.0, 7, 1, 1)
        assert y2.shape == (B, L, D)
        gs = o.sasrec_layer_backward(x, None, False, *w, 2, 1e-12, 0.0, 7, 1, 1, saved, torch.empty(B, L, D))
        assert [tuple(g.shape) for g in gs] == [(B, L, D)] + shapes
        sl = torch.empty(B, dtype=torch.int64)
        assert o.seq_pool(x, sl, POOL_ORIGIN).shape == (B, L, D)
        assert o.seq_pool(x, sl, POOL_LAST).shape == (B, D) and o.seq_pool(x, sl, POOL_MEAN).shape == (B, D)
        assert o.seq_pool_backward(torch.empty(B, D), sl, POOL_LAST, L).shape == (B, L, D)
        assert o.dropout(x, 0.5, 7, 1, 0).shape == (B, L, D)
        dE, dP = o.embed_gather_posadd_backward(x, torch.empty(B, L, dtype=torch.int64), 100, 50)
        assert dE.shape == (100, D) and dP.shape == (50, D)
    w = [torch.zeros(s) for s in shapes]
    with pytest.raises(Dr4srError):
        o.sasrec_layer(torch.zeros(2, 12, D), None, True, *w, 2, 1e-12, 0.0, 7, 1, 0)
    with pytest.raises(Dr4srError):
        o.seq_pool(torch.zeros(2, 12, D), torch.ones(2, dtype=torch.int64), POOL_LAST)
    with pytest.raises(Dr4srError):
        o.dropout(torch.zeros(2, 12, D), 0.5, 7, 1, 0)


def test_module_state_dict_carries_the_reference_names():
    """torch.nn.TransformerEncoder's parameter names under SASRecQueryEncoder (model/sasrec.py:10-37) = the engine's parameter names
    with the `query_encoder.` prefix stripped, plus the tied item table"""
    from dr4sr_amd.engine import param_names, param_shapes
    from dr4sr_amd.module.layers import SASRecQueryEncoderOps
    N, L, D, F, NL = 30, 12, 64, 128, 2
    table = torch.nn.Embedding(N, D, padding_idx=0)
    m = SASRecQueryEncoderOps("item_id", D, L, 2, F, 0.5, "gelu", 1e-12, NL, table, bidirectional=True)
    pre = "query_encoder."
    want = {n[len(pre):]: s for n, s in zip(param_names(NL), param_shapes(N, L, D, F, NL)) if n.startswith(pre)}
    want["item_encoder.weight"] = (N, D)
    sd = m.state_dict()
    assert set(sd) == set(want)
    for k, s in want.items():
        assert tuple(sd[k].shape) == tuple(s), k
    # the names torch's own layer gives them (what the reference's checkpoint holds)
    t = torch.nn.TransformerEncoder(torch.nn.TransformerEncoderLayer(D, 2, F, 0.5, "gelu", 1e-12, batch_first=True, norm_first=False), NL)
    assert {"transformer_layer." + k for k in t.state_dict()} == {k for k in sd if k.startswith("transformer_layer.")}
    assert m.bidirectional and m.step == 0
    with pytest.raises(NotImplementedError):
        SASRecQueryEncoderOps("item_id", D, L, 2, F, 0.5, "relu", 1e-12, NL, table)


def test_size_entry_points_refuse_unsupported_shapes():
    from dr4sr_amd import _lib
    lib = _lib.load()
    E_SHAPE = -2
    for fn in (lib.dr4sr_sasrec_layer_saved_floats, lib.dr4sr_sasrec_layer_workspace_bytes):
        assert fn(4, 50, 64, 2, 128) > 0 and fn(4, 64, 64, 2, 256) > 0 and fn(4, 64, 128, 2, 128) > 0
        assert fn(4, 65, 64, 2, 128) == E_SHAPE             # L = 65
        assert fn(4, 50, 96, 2, 128) == E_SHAPE             # D = 96
        assert fn(4, 50, 64, 4, 128) == E_SHAPE             # head_dim 16
        assert fn(4, 50, 128, 2, 256) == E_SHAPE and fn(4, 50, 128, 4, 128) == E_SHAPE
        assert fn(-1, 50, 64, 2, 128) == -1
    assert lib.dr4sr_sasrec_layer_saved_floats(3, 5, 64, 2, 128) == 3 * ((5 * (6 * 64 + 128) + 2 * 25 + 3) // 4 * 4)
    # the entry points answer before any launch: null pointers and bad shapes need no GPU
    assert lib.dr4sr_sasrec_layer_fwd(None, None, 1, None, 1, 12, 64, 2, 128, 1e-12, 0.0, 0, 0, 0, None, None, None) == -1
    assert lib.dr4sr_seq_pool_fwd(None, None, 1, 1, 12, 64, None, None) == -1
