"""Pin oracle/fmlp_oracle.py (circular-convolution restatement of the spectral filter) against golden vectors from the reference,
and tests/_fmlp_ref.py (its rfft / irfft form on float64 leaves, the yardstick of tests/test_gpu_fmlp_scale.py) against that form."""
import os

import numpy as np
import pytest
import torch

from oracle import fmlp_oracle as FO
from oracle import sasrec_oracle as O


def load(golden_dir):
    z = np.load(os.path.join(golden_dir, "fmlp_d64.npz"))
    g = {k: z[k] for k in z.files}
    params = {k[6:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param.")}
    batch = {k[6:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("batch.")}
    return g, params, batch


@pytest.mark.parametrize("use_fft", [False, True])
def test_fmlp_forward(golden_dir, use_fft):
    g, p, b = load(golden_dir)
    nl = int(g["meta.layer_num"])
    q, acts = FO.fmlp_encode(p, b["in_item_id"], nl, use_fft=use_fft, return_all=True)
    for k in ("x0", "filter0", "layer0", "filter1", "layer1"):
        np.testing.assert_allclose(acts[k].numpy(), g["act." + k], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(q.numpy(), g["out.query"], rtol=2e-4, atol=2e-5)
    loss, pos, ng = O.score_bce(q, p["item_embedding.weight"], b["item_id"], b["neg_item"], True)
    np.testing.assert_allclose(float(loss), float(g["out.loss"]), rtol=2e-6)
    lnr, _, _ = O.score_bce(q, p["item_embedding.weight"], b["item_id"], b["neg_item"], False)
    np.testing.assert_allclose(lnr.numpy(), g["out.loss_noreduce"], rtol=2e-4, atol=1e-7)


def test_fmlp_gradients_and_adam(golden_dir):
    g, p, b = load(golden_dir)
    nl = int(g["meta.layer_num"])
    loss, q, grads = FO.grads_of(p, b, nl)
    for k, gv in grads.items():
        ref = g["grad." + k]
        assert float(np.abs(gv.numpy() - ref).max()) < 3e-4 * max(1e-8, float(np.abs(ref).max())), k
    # imaginary parts of the DC and Nyquist bins are ignored by irfft: zero gradient in the reference too
    gc = g["grad.item_encoder.layer.0.filterlayer.complex_weight"]
    assert np.abs(gc[0, 0, :, 1]).max() == 0 and np.abs(gc[0, 25, :, 1]).max() < 1e-9
    params = {k: v.clone() for k, v in p.items()}
    m = {k: torch.zeros_like(v) for k, v in params.items()}
    v = {k: torch.zeros_like(x) for k, x in params.items()}
    for t, tag in ((1, "adam1."), (2, "adam2.")):
        _, _, gr = FO.grads_of(params, b, nl)
        params = O.adam_step(params, gr, m, v, t, lr=float(g["meta.lr"]))
        for k in params:
            well = np.abs(g["grad." + k]) > 1e-5
            np.testing.assert_allclose(params[k].numpy()[well], g[tag + k][well], rtol=0, atol=5e-6)
            np.testing.assert_allclose(params[k].numpy(), g[tag + k], rtol=0, atol=2.1e-3)   # <= 2 Adam steps of lr: ill-conditioned |g|~eps elements


# ---- tests/_fmlp_ref.py: the float64 rfft / irfft form the GPU tests above B = 256 compare with (tests/test_gpu_fmlp_scale.py)
def _case(L, NL=2, B=6, N=150, seed=None):
    import _fmlp_ref as FR
    params, idx, tgt, neg = FR.make_case(B, L, NL, N, seed=300 + L if seed is None else seed)
    return params, {"in_item_id": idx, "item_id": tgt, "neg_item": neg}


def _assert_same_f64(loss, grads, loss_c, grads_c):
    """bound: 1e-12 on the loss, 1e-10 of each tensor's max-abs on the gradients (FFT vs circular form measured 1e-14 in float64: four
    orders of margin, and far below anything a comparison with fp32 kernels resolves)"""
    assert loss.dtype == torch.float64 and abs(float(loss) - float(loss_c)) < 1e-12
    assert set(grads) == set(grads_c)
    for k, gv in grads.items():
        assert gv.dtype == torch.float64
        d = float((gv - grads_c[k]).abs().max())
        assert d < 1e-10 * float(grads_c[k].abs().max()), (k, d)


def test_make_case_plants_its_edge_rows():
    import _fmlp_ref as FR
    for L in (2, 4, 50):
        _, idx, tgt, neg = FR.make_case(6, L, 1, 150, seed=1)
        assert bool((idx[0] != 0).all()) and int((idx[1] != 0).sum()) == 1 and idx[1, L - 1] != 0 and int(idx[2].abs().sum()) == 0
        if L >= 4:
            assert idx[3, L - 2] == 0 and idx[3, L - 1] != 0 and idx[3, L - 3] != 0
        assert tgt[4] == 0 and int((tgt == 0).sum()) == 1 and idx[5, L - 1] == idx[5, L - 2] != 0 and tgt[5] == tgt[0]
        assert neg.shape == (6, 1) and int(neg.min()) >= 1
        nv = (idx != 0).long()
        assert bool((nv[:, 1:] >= nv[:, :-1])[[0, 1, 2, 4, 5]].all()), "left-padded prefixes"


@pytest.mark.parametrize("L", list(range(2, 51, 2)))
def test_f64_fft_reference_equals_circular_form_at_every_even_length(L):
    import _fmlp_ref as FR
    params, batch = _case(L)
    loss, q, grads = FR.step_grads(params, batch, 2)
    loss_c, q_c, grads_c = FO.grads_of(params, batch, 2, dtype=torch.float64)
    _assert_same_f64(loss, grads, loss_c, grads_c)
    assert float((q - q_c).abs().max()) < 1e-12 * max(1.0, float(q_c.abs().max()))
    assert float(grads["item_embedding.weight"][0].abs().max()) == 0.0


def test_f64_fft_reference_vs_fp32_oracle():
    import _fmlp_ref as FR
    params, batch = _case(50, B=29, seed=7)
    loss, _, grads = FR.step_grads(params, batch, 2)
    loss_o, _, grads_o = FO.grads_of(params, batch, 2)
    assert abs(float(loss) - float(loss_o)) < 2e-6 * abs(float(loss))
    for k, gv in grads.items():
        ref = grads_o[k].numpy()
        assert float(np.abs(gv.numpy() - ref).max()) < 3e-4 * max(1e-8, float(np.abs(ref).max())), k


def test_f64_fft_and_circular_forms_agree_under_masks():
    import _fmlp_ref as FR
    B, L, NL, p = 6, 20, 2, 0.5
    params, batch = _case(L, NL=NL, seed=9)
    gen = torch.Generator().manual_seed(4)
    masks = {FO.SITE_EMB: (torch.rand(B, L, 64, generator=gen) >= p).float()}
    for l in range(NL):
        for kind in (FO.SITE_FILT, FO.SITE_FFN):
            masks[FO.site(kind, l)] = (torch.rand(B, L, 64, generator=gen) >= p).float()
    loss, _, grads = FR.step_grads(params, batch, NL, masks=masks, pdrop=p)
    loss_c, _, grads_c = FO.grads_of(params, batch, NL, masks=masks, pdrop=p, dtype=torch.float64)
    _assert_same_f64(loss, grads, loss_c, grads_c)
    loss_0, _, _ = FR.step_grads(params, batch, NL)
    assert abs(float(loss) - float(loss_0)) > 1e-4, "the masks reached the model"
    # the dense path's reference under the same masks: d_out on the query alone is the step without its scorer
    d_out = torch.randn(B, 64, generator=gen)
    out, g_enc = FR.encode_grads(params, batch["in_item_id"], d_out, NL, masks=masks, pdrop=p)
    leaf = {k: v.double().requires_grad_(True) for k, v in params.items()}
    out_c = FO.fmlp_encode(leaf, batch["in_item_id"], NL, 1e-12, masks, p)
    out_c.backward(d_out.double())
    out_c = out_c.detach()
    assert float((out - out_c).abs().max()) < 1e-12 * float(out_c.abs().max())
    for k, gv in g_enc.items():
        ref = leaf[k].grad if leaf[k].grad is not None else torch.zeros_like(leaf[k])
        assert float((gv - ref).abs().max()) <= 1e-10 * float(ref.abs().max()), k
