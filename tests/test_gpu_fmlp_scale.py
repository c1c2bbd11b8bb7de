"""FMLP above 256 rows, at every even L and through the dense (autograd) entry points, against float64 (tests/_fmlp_ref.py: the oracle's
rfft / irfft form on float64 leaves, pinned on the CPU by tests/test_fmlp_oracle.py).

What csrc/fmlp.hip and csrc/linear.hip do differently with the batch size, none of which a B <= 256 test reaches:
  B > 256 (FM_DMBLK)        k_fmlp_filter_bwd / k_fmlp_embed_bwd run 256 workgroups that walk several sequences each (LDS images re-used,
                            dmacc / dgam / dbet / accP carried across sequences)
  B L > 16384               64-row fp32-MFMA Intermediate kernels instead of the 32-row bf16x3 ones, ln_part per 64-row tile
  B L > 32768               second trip of k_fmlp_embed_fwd's (and the dense path's k_fmlp_last_bwd's) token loop
  B L / 64 / 8 > 160        launch_fmlp_wgrad's split cap = FM_DET_SPLITS, what the deterministic buffers are carved for
Bars: tests/test_gpu_fmlp.py's (REL per tensor, 3e-5 on the loss) unless a test says otherwise.  N = 997 items, so table rows collide.
Every test prints its worst figure and the tensor it belongs to (NOTEBOOK.md records them)."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import _fmlp_ref as FR  # noqa: E402
from oracle import fmlp_oracle as FO  # noqa: E402
from test_gpu_fmlp import REL, relerr  # noqa: E402

N = 997
LOSS_TOL = 3e-5
SAME = 1e-5            # "the same up to the order of the atomics": test_gpu_parity.py::test_second_backward_on_one_forward_gives_the_same_gradients
TABLE = FR.TABLE

LADDER = [(257, 2, 50),      # one workgroup of the filter / embedding backward takes a second sequence
          (327, 2, 50),      # 16350 tokens: the last batch in the 32-row bf16x3 form
          (328, 2, 50),      # 16400 tokens: the first in the 64-row fp32 form; the last tile holds 16 rows
          (700, 2, 50),      # 35000 tokens: second trip of the embedding loop; three sequences per backward workgroup
          (1700, 2, 50),     # 1329 weight-gradient tiles: the 160-split cap
          (400, 3, 20),      # B > 256 with a short L, still in the 32-row forms
          (1000, 4, 8),      # B > 256 with a short L, still in the 32-row forms
          (900, 1, 20)]      # the 64-row forms reached with a short L


@functools.lru_cache(maxsize=None)
def case(B, NL, L):
    """parameters, batch and the float64 step (loss, query, gradients) — built once per shape, shared, left unchanged"""
    params, idx, tgt, neg = FR.make_case(B, L, NL, N, seed=1000 + 13 * B + 7 * L + NL)
    batch = {"in_item_id": idx, "item_id": tgt, "neg_item": neg}
    return params, batch, FR.step_grads(params, batch, NL)


def build(params, NL, L, max_batch, p=0.0, seed=2023):
    from dr4sr_amd.fmlp_engine import FmlpEngine
    eng = FmlpEngine(N, L, 64, 256, NL, 1e-12, p, max_batch, "cuda", seed=seed)
    eng.load_named(params)
    return eng


def run_step(eng, batch):
    dev = eng.device
    plan = eng.make_plan(batch["in_item_id"].to(dev), batch["item_id"].to(dev), neg_item=batch["neg_item"].view(-1).contiguous().to(dev),
                         sample_neg=False)
    eng.fwd_bwd(plan)
    torch.cuda.synchronize()
    return plan


def engine_masks(eng, B, L, NL, step):
    """the library's own keep masks (dr4sr_dropout_mask): sites 0, 1 + 2 l, 2 + 2 l; element order [B, L, 64]"""
    masks = {FO.SITE_EMB: eng.dropout_mask(B * L * 64, 0, step).view(B, L, 64).cpu()}
    for l in range(NL):
        masks[FO.site(FO.SITE_FILT, l)] = eng.dropout_mask(B * L * 64, 1 + 2 * l, step).view(B, L, 64).cpu()
        masks[FO.site(FO.SITE_FFN, l)] = eng.dropout_mask(B * L * 64, 2 + 2 * l, step).view(B, L, 64).cpu()
    return masks


def check_grads(grads, ref, tag, bar=REL, scale=1.0):
    """every tensor of `grads` against scale * ref; prints the worst figure and its tensor"""
    fig = {k: relerr(v, (scale * ref[k]).cpu()) for k, v in grads.items()}
    worst = max(fig, key=lambda k: fig[k])
    print(f"{tag}: worst gradient {fig[worst]:.2e} ({worst})")
    bad = "; ".join(f"{k} {v:.2e}" for k, v in fig.items() if not v < bar)        # (not <: a NaN fails too)
    assert not bad, f"{tag}: at or above {bar:g}: {bad}"
    return fig


def check_table_rows(eng, batch):
    """the PAD row and every table row that no input id, target or negative names hold exactly zero"""
    g = eng.grad_views[TABLE].cpu()
    touched = torch.zeros(N, dtype=torch.bool)
    for k in ("in_item_id", "item_id", "neg_item"):
        touched[batch[k].reshape(-1)] = True
    touched[0] = False
    assert float(g[0].abs().max()) == 0.0, "the PAD row takes no gradient"
    assert bool((g[~touched] == 0).all()), "rows outside the batch take no gradient"


def check_step(eng, batch, ref, tag):
    loss_o, _, grads_o = ref
    loss, n = eng.loss_and_count()
    print(f"{tag}: loss {loss:.7f} vs {float(loss_o):.7f} (difference {abs(loss - float(loss_o)):.2e}), n = {n}")
    assert n == int((batch["item_id"] != 0).sum())
    assert abs(loss - float(loss_o)) < LOSS_TOL
    check_grads(eng.normalized_grads(), grads_o, tag)
    check_table_rows(eng, batch)


# ------------------------------------------------------------------------------------------------ a. the regime ladder
@pytest.mark.parametrize("B,NL,L", LADDER)
def test_fused_step_across_the_batch_regimes_vs_float64(B, NL, L):
    params, batch, ref = case(B, NL, L)
    eng = build(params, NL, L, B)
    run_step(eng, batch)
    check_step(eng, batch, ref, f"step B={B} NL={NL} L={L}")


# ------------------------------------------------------------------------------------------------ b. its corners, deterministic mode
@pytest.mark.parametrize("B,NL,L", [(328, 2, 50), (1700, 2, 50), (400, 3, 20)])
def test_deterministic_step_across_the_batch_regimes_vs_float64(monkeypatch, B, NL, L):
    monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    params, batch, ref = case(B, NL, L)
    flat = []
    for _ in range(2):                                     # two engines from the same inputs
        eng = build(params, NL, L, B)
        run_step(eng, batch)
        flat.append(eng.grads.clone())
    check_step(eng, batch, ref, f"deterministic step B={B} NL={NL} L={L}")
    assert torch.equal(flat[0], flat[1]), "deterministic mode: the flat gradient is a pure function of the batch"


# ------------------------------------------------------------------------------------------------ c. dropout above the thresholds
@pytest.mark.parametrize("B,NL,L", [(328, 2, 50), (300, 3, 20)])
def test_dropout_step_above_the_thresholds_vs_float64(B, NL, L):
    p = 0.5
    params, batch, _ = case(B, NL, L)
    eng = build(params, NL, L, B, p=p, seed=77)
    run_step(eng, batch)
    masks = engine_masks(eng, B, L, NL, int(eng.state[3]))
    keep = float(masks[FO.SITE_EMB].mean())
    print(f"dropout B={B} NL={NL} L={L}: keep rate of the embedding mask {keep:.4f}")
    assert abs(keep - (1 - p)) < 0.02
    ref = FR.step_grads(params, batch, NL, masks=masks, pdrop=p)
    check_step(eng, batch, ref, f"dropout step B={B} NL={NL} L={L}")


# ------------------------------------------------------------------------------------------------ d. every even L
@pytest.mark.parametrize("L", list(range(2, 51, 2)))
def test_fused_step_at_every_even_length_vs_float64(L):
    """conv4's S & 3 tail and clamped reads, the row groups past L, the DC / Nyquist bins and the (k r) % L tables all depend on L;
    B = 6: the planted edge rows of _fmlp_ref.make_case"""
    params, batch, ref = case(6, 1, L)
    eng = build(params, 1, L, 6)
    run_step(eng, batch)
    check_step(eng, batch, ref, f"step L={L}")


# ------------------------------------------------------------------------------------------------ e. the dense path
@functools.lru_cache(maxsize=None)
def dense_case(B, NL=2, L=50):
    params, batch, _ = case(B, NL, L)
    d_out = torch.randn(B, 64, generator=torch.Generator().manual_seed(40 + B))
    return params, batch["in_item_id"], d_out, FR.encode_grads(params, batch["in_item_id"], d_out, NL)


def dense_backward(eng, plan, training, d_out, calls=1):
    eng.grads.zero_()
    for _ in range(calls):
        eng.encode_bwd(plan, training, d_out)
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in eng.grad_views.items()}


@pytest.mark.parametrize("B,det", [(6, False), (300, False), (700, False), (300, True)])
def test_dense_encode_and_backward_vs_float64(monkeypatch, B, det):
    """dr4sr_fmlp_encode / dr4sr_fmlp_encode_bwd at engine level: eval forward, train forward under the library's own masks (p = 0.5), and
    the un-normalised gradients of each under a random d_out"""
    if det:
        monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    NL, L, p = 2, 50, 0.5
    params, idx, d_out, (out_o, grads_o) = dense_case(B)
    eng = build(params, NL, L, B, p=p, seed=31)
    idx_d, d_out_d = idx.cuda(), d_out.cuda()
    plan = eng.make_plan(idx_d, None)
    tag = f"dense B={B}{' deterministic' if det else ''}"
    out = eng.encode(plan, False)
    e = relerr(out, out_o)
    print(f"{tag}: eval out {e:.2e}")
    assert e < REL
    grads = dense_backward(eng, plan, False, d_out_d)
    check_grads(grads, grads_o, tag + " eval")
    assert float(grads[TABLE][0].abs().max()) == 0.0
    out_t = eng.encode(plan, True)
    masks = engine_masks(eng, B, L, NL, int(eng.state[3]))
    out_m, grads_m = FR.encode_grads(params, idx, d_out, NL, masks=masks, pdrop=p)
    e = relerr(out_t, out_m)
    print(f"{tag}: train out {e:.2e}")
    assert e < REL and relerr(out_t, out_o) > 1e-2, "the train forward is the masked one"
    grads = dense_backward(eng, plan, True, d_out_d)
    check_grads(grads, grads_m, tag + " train")
    assert float(grads[TABLE][0].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ f. the accumulate contract
@pytest.mark.parametrize("B,det", [(6, False), (300, False), (6, True), (300, True)])
def test_dense_backward_accumulates_into_the_gradients(monkeypatch, B, det):
    """include/dr4sr_hip.h, dr4sr_fmlp_encode_bwd: "parameter gradients ACCUMULATE into plan->grads" — two calls on one forward without a
    zero-fill leave twice the gradient in EVERY tensor (k_fmlp_dm_reduce used to store the position table's, losing the first call's)"""
    if det:
        monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    NL, L = 2, 50
    params, idx, d_out, (_, grads_o) = dense_case(B)
    eng = build(params, NL, L, B)
    idx_d, d_out_d = idx.cuda(), d_out.cuda()
    plan = eng.make_plan(idx_d, None)
    eng.encode(plan, False)
    once = dense_backward(eng, plan, False, d_out_d)
    twice = dense_backward(eng, plan, False, d_out_d, calls=2)
    tag = f"accumulate B={B}{' deterministic' if det else ''}"
    check_grads(twice, grads_o, tag + " 2 calls vs 2 x float64", scale=2.0)
    check_grads(twice, once, tag + " 2 calls vs 2 x 1 call", bar=SAME, scale=2.0)
    if det:
        for k, v in twice.items():
            assert torch.equal(v, 2 * once[k]), k


# ------------------------------------------------------------------------------------------------ g. the same contract on SASRec
@pytest.mark.parametrize("form", ["latency", "at_scale", "deterministic"])
def test_sasrec_dense_backward_accumulates_in_every_form(monkeypatch, form):
    """dr4sr_sasrec_encode_bwd promises the same (CL4SRec's two views rely on it): the B = 7, L = 12 batch of tests/test_gpu_input_weight.py,
    origin pooling, two calls without a zero-fill"""
    import test_gpu_input_weight as IW
    from dr4sr_amd import _lib
    env, expect = IW.FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    idx, sl, _ = IW.small_batch()
    eng = IW.make_engine(IW.random_params(IW.N, 64, IW.L, seed=77), 64)
    idx_d, sl_d = idx.cuda(), sl.cuda()
    plan = eng.make_plan(idx_d, None, sl_d)
    bits = int(_lib.load().dr4sr_sasrec_at_scale(C.byref(plan)))
    assert expect(bits), (form, bits)
    d_out = torch.randn(IW.B, IW.L, 64, generator=torch.Generator().manual_seed(6)).cuda()
    eng.encode(plan, False, _lib.POOL_ORIGIN)
    got = []
    for calls in (1, 2):
        eng.grads.zero_()
        for _ in range(calls):
            eng.encode_bwd(plan, False, _lib.POOL_ORIGIN, d_out)
        torch.cuda.synchronize()
        got.append({k: v.clone() for k, v in eng.grad_views.items()})
    once, twice = got
    assert float(once[IW.R.TABLE].abs().max()) > 0
    check_grads(twice, once, f"sasrec accumulate {form}", bar=SAME, scale=2.0)
    if form == "deterministic":
        for k, v in twice.items():
            assert torch.equal(v, 2 * once[k]), k


# ------------------------------------------------------------------------------------------------ h. a partial batch in a larger engine
@pytest.mark.parametrize("det", [False, True])
def test_partial_batch_through_rows_follows_the_plans_batch(monkeypatch, det):
    """an engine built for 328 rows (the 64-row forms' capacity) running a 100-row plan addressed through rows= takes the launch forms of
    B = 100, not of its capacity: the gradients of an engine built for 100 rows on the materialised batch"""
    if det:
        monkeypatch.setenv("DR4SR_DETERMINISTIC", "1")
    NL, L, M, B = 2, 50, 150, 100
    params, data, _ = case(M, NL, L)
    perm = 6 + torch.randperm(M - 6, generator=torch.Generator().manual_seed(8))
    rows = torch.cat([perm[:47], torch.arange(6), perm[47:94]])          # the planted edge rows, somewhere in the middle
    rows[60] = rows[20]                                                   # one dataset row twice
    assert rows.shape[0] == B
    neg = torch.randint(1, N, (B, 1), generator=torch.Generator().manual_seed(9))
    batch = {"in_item_id": data["in_item_id"][rows].contiguous(), "item_id": data["item_id"][rows].contiguous(), "neg_item": neg}
    ref = FR.step_grads(params, batch, NL)
    big = build(params, NL, L, 328)
    ds_idx, ds_tgt, rows_d, neg_d = data["in_item_id"].cuda(), data["item_id"].cuda(), rows.cuda(), neg.view(-1).contiguous().cuda()
    plan = big.make_plan(ds_idx, ds_tgt, rows=rows_d, neg_item=neg_d, sample_neg=False)
    assert plan.B == B
    big.fwd_bwd(plan)
    torch.cuda.synchronize()
    tag = f"rows= in a larger engine{' deterministic' if det else ''}"
    check_step(big, batch, ref, tag)
    small = build(params, NL, L, B)
    run_step(small, batch)
    if det:
        assert torch.equal(big.grads, small.grads)
    else:
        assert big.loss_and_count()[1] == small.loss_and_count()[1]
        check_grads(dict(big.grad_views), dict(small.grad_views), tag + " vs an engine of 100 rows", bar=SAME)
