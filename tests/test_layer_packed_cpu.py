"""CPU checks of the packed encoder-layer op (no GPU): the dispatcher registration with fake kernels, the refusal of CPU tensors, the
size entry points, the `use_seqlen` keyword of SASRecQueryEncoderOps, and the properties of the tile plan as tests/_packed_ref.py states
it (the GPU test holds the device's plan against that statement)."""
import random

import pytest
import torch

import _packed_ref as PR

SHAPES = lambda D, F: [(3 * D, D), (3 * D,), (D, D), (D,), (F, D), (F,), (D, F), (D,), (D,), (D,), (D,), (D,)]  # noqa: E731
SUPPORTED = [(64, 2, 128), (64, 2, 256), (128, 2, 128)]


def test_ops_are_registered_with_fake_kernels_and_refuse_cpu_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import dr4sr_amd.ops as ops
    from dr4sr_amd import _lib
    lib = _lib.load()
    for n in ("sasrec_layer_packed", "sasrec_layer_packed_backward"):
        assert n in ops.OPS and hasattr(torch.ops.dr4sr_hip, n), n
        schema = str(getattr(torch.ops.dr4sr_hip, n).default._schema)
        assert "Tensor seqlen" in schema and "key_padding_mask" not in schema, schema
    o = torch.ops.dr4sr_hip
    for B, L, (D, H, F) in ((8, 50, SUPPORTED[1]), (3, 7, SUPPORTED[2])):
        with FakeTensorMode():
            x = torch.empty(B, L, D)
            sl = torch.empty(B, dtype=torch.int64)
            w = [torch.empty(s) for s in SHAPES(D, F)]
            y, saved = o.sasrec_layer_packed(x, sl, True, *w, H, 1e-12, 0.5, 7, 1, 0)
            assert y.shape == (B, L, D) and y.dtype == torch.float32 and saved.dim() == 1 and saved.dtype == torch.float32
            assert saved.numel() == lib.dr4sr_sasrec_layer_packed_saved_floats(B, L, D, H, F)
            gs = o.sasrec_layer_packed_backward(x, sl, False, *w, H, 1e-12, 0.0, 7, 1, 1, saved, torch.empty(B, L, D))
            assert [tuple(g.shape) for g in gs] == [(B, L, D)] + SHAPES(D, F)
    D, H, F = SUPPORTED[0]
    w = [torch.zeros(s) for s in SHAPES(D, F)]
    x, sl = torch.zeros(2, 12, D), torch.ones(2, dtype=torch.int64)
    with pytest.raises(_lib.Dr4srError):
        o.sasrec_layer_packed(x, sl, True, *w, H, 1e-12, 0.0, 7, 1, 0)
    with pytest.raises(_lib.Dr4srError):
        o.sasrec_layer_packed_backward(x, sl, True, *w, H, 1e-12, 0.0, 7, 1, 0, torch.zeros(8), torch.zeros(2, 12, D))


def test_size_entry_points_refuse_what_the_dense_op_refuses_and_save_no_more():
    from dr4sr_amd import _lib
    lib = _lib.load()
    E_ARG, E_SHAPE = -1, -2
    sizes = (lib.dr4sr_sasrec_layer_packed_saved_floats, lambda *a: lib.dr4sr_sasrec_layer_packed_workspace_bytes(*a, 0),
             lambda *a: lib.dr4sr_sasrec_layer_packed_workspace_bytes(*a, 1))
    bad = [(4, 65, 64, 2, 128), (4, 50, 96, 2, 128), (4, 50, 64, 4, 128), (4, 50, 128, 2, 256), (4, 50, 128, 4, 128), (4, 0, 64, 2, 128),
           (-1, 50, 64, 2, 128), (1 << 20, 64, 64, 2, 128)]
    for a in bad:
        want = lib.dr4sr_sasrec_layer_saved_floats(*a)
        assert want in (E_ARG, E_SHAPE), a
        for fn in sizes:
            assert fn(*a) == want, a
    for D, H, F in SUPPORTED:
        for B in (0, 1, 7, 256, 600, 8192):
            for L in (1, 2, 12, 50, 63, 64):
                n, dense = lib.dr4sr_sasrec_layer_packed_saved_floats(B, L, D, H, F), lib.dr4sr_sasrec_layer_saved_floats(B, L, D, H, F)
                assert 0 <= n <= dense and (B == 0 or n > 0), (B, L, D, F)
                f, b = sizes[1](B, L, D, H, F), sizes[2](B, L, D, H, F)
                assert 0 <= f <= b and f % 16 == 0 and b % 16 == 0, (B, L, D, F)
    assert _lib.probe("dr4sr_sasrec_layer_packed_chunk")() >= 64
    # the entry points answer before any launch: null pointers and bad shapes need no GPU
    assert lib.dr4sr_sasrec_layer_packed_fwd(None, None, 1, None, 1, 12, 64, 2, 128, 1e-12, 0.0, 0, 0, 0, None, None, None, 0, None) == E_ARG
    w = _lib.LayerWeights(*[1] * 12)
    g = _lib.LayerGrads(*[1] * 12)
    assert lib.dr4sr_sasrec_layer_packed_fwd(1, 1, 1, w, 1, 65, 64, 2, 128, 1e-12, 0.0, 0, 0, 0, 1, None, 1, 1 << 20, None) == E_SHAPE
    assert lib.dr4sr_sasrec_layer_packed_fwd(1, None, 1, w, 1, 12, 64, 2, 128, 1e-12, 0.0, 0, 0, 0, 1, None, 1, 1 << 20, None) == E_ARG
    assert lib.dr4sr_sasrec_layer_packed_fwd(1, 1, 1, w, 1, 12, 64, 2, 128, 1e-12, 0.0, 0, 0, 0, 1, None, 1, 8, None) == -3
    assert lib.dr4sr_sasrec_layer_packed_fwd(1, 1, 1, w, 1, 12, 64, 2, 128, 1e-12, 1.0, 0, 0, 0, 1, None, 1, 1 << 20, None) == E_ARG
    assert lib.dr4sr_sasrec_layer_packed_bwd(1, None, 1, w, 1, 12, 64, 2, 128, 1e-12, 0.0, 0, 0, 0, 1, 1, 1, g, 1, 1 << 30, None) == E_ARG
    assert lib.dr4sr_sasrec_layer_packed_bwd(1, 1, 1, w, 1, 12, 64, 2, 128, 1e-12, 0.0, 0, 0, 0, 1, 1, 1, g, 1, 8, None) == -3
    assert _lib.probe("dr4sr_sasrec_layer_packed_plan")(1, 1, 65, 1, 1, 1, 1, 1 << 20, None) == E_SHAPE


def test_module_keeps_its_state_dict_and_defaults_to_the_dense_op():
    from dr4sr_amd.module.layers import SASRecQueryEncoderOps
    N, L, D, F, NL = 30, 12, 64, 128, 2
    table = torch.nn.Embedding(N, D, padding_idx=0)
    args = ("item_id", D, L, 2, F, 0.5, "gelu", 1e-12, NL, table)
    m0, m1 = SASRecQueryEncoderOps(*args), SASRecQueryEncoderOps(*args, use_seqlen=True)
    assert m0.use_seqlen is False and m1.use_seqlen is True
    sd0, sd1 = m0.state_dict(), m1.state_dict()
    assert list(sd0) == list(sd1) and all(sd0[k].shape == sd1[k].shape for k in sd0)
    m1.load_state_dict(sd0)


HAND_MADE = [
    (12, [12, 0, 1, 5, 12, 3, 2]),
    (50, [50, 14, 1, 50, 15, 64, -3, 13, 50]),
    (64, [64, 63, 1]),
    (50, []),
    (50, [0, 0, 0]),
    (50, [0] * 70 + [3] + [0] * 70 + [4, 60]),               # zeros across a chunk edge
    (1, [1] * 200),                                          # 64 sequences fill a tile exactly
    (40, [40] * 122 + [3] * 12 + [40] * 30),
]


@pytest.mark.parametrize("C", [64, 128, 200])
def test_python_plan_has_the_properties_of_a_tile_plan(C):
    rnd = random.Random(C)
    cases = list(HAND_MADE)
    for L in (5, 50, 64):
        cases.append((L, [rnd.randint(-2, L + 5) for _ in range(700)]))
        cases.append((L, [rnd.choice((0, 0, 1, 2, 3, L)) for _ in range(333)]))
    for L, sl in cases:
        tile_of, row_of, n_tiles = PR.plan(sl, L, C)
        assert len(tile_of) == len(row_of) == len(sl)
        PR.check_plan(sl, L, C, tile_of, row_of, n_tiles)
        if not any(n > 0 for n in sl):
            assert n_tiles == 0
    # the worked examples of the kernel's header: 50 + 14 fills a tile, 15 + 50 does not fit, 64 clamps to 50, -3 to 0
    assert PR.plan(HAND_MADE[1][1], 50, C) == ([0, 0, 1, 1, 2, 3, -1, 3, 4], [0, 50, 0, 1, 0, 0, -1, 50, 0], 5)
    assert PR.plan(HAND_MADE[0][1], 12, C) == ([0, -1, 0, 0, 0, 0, 0], [0, -1, 12, 13, 18, 30, 33], 1)
    assert PR.plan(HAND_MADE[2][1], 64, C) == ([0, 1, 1], [0, 0, 63], 2)
    # a chunk edge closes the tile: sequence C starts tile 1 although it would fit
    assert PR.plan([1] * (C + 1), 8, C)[0][C - 1:] == [(C - 1) // 64, (C - 1) // 64 + 1]
