"""The plan is the contract: everything an engine tells libdr4sr_hip.so goes through the plan struct (include/dr4sr_hip.h) plus a few
scalar arguments, so the three engines over FlatEngine (dr4sr_amd/flat_engine.py) are checked field by field against expectations written
out HERE, from the header's meaning of each field — never read back from the engine's own plan code.  Smallest shapes the libraries
accept; no kernel runs beyond allocations and the mean of a four-element seqlen tensor."""
import ctypes as C
import math

import pytest
import torch

from dr4sr_amd import _lib
from dr4sr_amd.engine import SasrecEngine
from dr4sr_amd.fmlp_engine import FmlpEngine
from dr4sr_amd.gru_engine import GruEngine

pytestmark = pytest.mark.gpu

DEV = "cuda"
L, MAX_B, SEED, P_DROP = 8, 4, 77, 0.25
GOLDEN = 0x9E3779B97F4A7C15

LAYER = "query_encoder.transformer_layer.layers.0."
FLAYER = "item_encoder.layer.0."
# name -> shape of the flat layout at the shapes below, in the header's order ("Flat parameter layout"); tensors lie back to back
LAYOUT = {
    "sasrec": [("item_embedding.weight", (40, 64)), ("query_encoder.position_emb.weight", (8, 64)),
               (LAYER + "self_attn.in_proj_weight", (192, 64)), (LAYER + "self_attn.in_proj_bias", (192,)),
               (LAYER + "self_attn.out_proj.weight", (64, 64)), (LAYER + "self_attn.out_proj.bias", (64,)),
               (LAYER + "linear1.weight", (128, 64)), (LAYER + "linear1.bias", (128,)), (LAYER + "linear2.weight", (64, 128)),
               (LAYER + "linear2.bias", (64,)), (LAYER + "norm1.weight", (64,)), (LAYER + "norm1.bias", (64,)),
               (LAYER + "norm2.weight", (64,)), (LAYER + "norm2.bias", (64,))],
    "fmlp": [("item_embedding.weight", (40, 64)), ("position_embeddings.weight", (8, 64)), ("LayerNorm.weight", (64,)), ("LayerNorm.bias", (64,)),
             (FLAYER + "filterlayer.complex_weight", (1, 5, 64, 2)), (FLAYER + "filterlayer.LayerNorm.weight", (64,)),
             (FLAYER + "filterlayer.LayerNorm.bias", (64,)), (FLAYER + "intermediate.dense_1.weight", (256, 64)),
             (FLAYER + "intermediate.dense_1.bias", (256,)), (FLAYER + "intermediate.dense_2.weight", (64, 256)),
             (FLAYER + "intermediate.dense_2.bias", (64,)), (FLAYER + "intermediate.LayerNorm.weight", (64,)),
             (FLAYER + "intermediate.LayerNorm.bias", (64,))],
    "gru": [("item_embedding.weight", (40, 64)), ("query_encoder.0.3.gru.weight_ih_l0", (384, 64)), ("query_encoder.0.3.gru.weight_hh_l0", (384, 128)),
            ("query_encoder.1.weight", (64, 128)), ("query_encoder.1.bias", (64,))],
}
# the shape fields of each plan struct
SHAPE = {
    "sasrec": dict(L=8, D=64, H=2, F=128, n_layer=1, n_items=40, ln_eps=1e-12),
    "fmlp": dict(L=8, D=64, F=256, n_layer=1, n_items=40, ln_eps=1e-12),
    "gru": dict(L=8, D=64, H=128, n_layer=1, n_items=40),
}
NEG_SCRATCH = {"sasrec": 32, "fmlp": 4, "gru": 32}          # max_batch * L negatives; FMLP draws one per row
KINDS = ("sasrec", "fmlp", "gru")


def build(kind, **kw):
    if kind == "sasrec":
        return SasrecEngine(40, 8, 64, 2, 128, 1, 1e-12, P_DROP, MAX_B, DEV, seed=SEED, n_slots=2, **kw)
    if kind == "fmlp":
        return FmlpEngine(40, 8, 64, 256, 1, 1e-12, P_DROP, MAX_B, DEV, seed=SEED, **kw)
    return GruEngine(40, 8, 64, 128, 1, P_DROP, MAX_B, DEV, seed=SEED, **kw)


@pytest.fixture(scope="module")
def engines():
    made = {k: build(k) for k in KINDS}
    made["sasrec"].mean_len = 3.5               # per-batch plans take their regime hint from it (no synchronisation)
    return made


def i64(*shape):
    return torch.ones(*shape, dtype=torch.int64, device=DEV)


def batch(kind, B=MAX_B, seqlen=True):
    """(positional make_plan arguments of a materialised batch, the same as a dict of plan fields)"""
    ids, tgt = i64(B, L), (i64(B) if kind == "fmlp" else i64(B, L))
    if kind == "fmlp":
        return (ids, tgt), dict(in_item_id=ids, item_id=tgt)
    sl = i64(B) if seqlen else None
    return (ids, tgt, sl), dict(in_item_id=ids, item_id=tgt, seqlen=sl)


def f32(x):
    return C.c_float(x).value


def fields(plan):
    return {name: (getattr(plan, name) or 0) for name, _ in plan._fields_}


def expected(kind, eng, B, tensors, **over):
    """every field of a plan of `eng` over `tensors` (field -> tensor or None), with the defaults of a fresh engine; `over` replaces"""
    e = dict(abi_version=_lib.ABI_VERSION, B=B, p_drop=f32(P_DROP), seed=SEED,
             params=eng.params.data_ptr(), grads=eng.grads.data_ptr(), adam_m=eng.adam_m.data_ptr(), adam_v=eng.adam_v.data_ptr(),
             n_params=sum(math.prod(s) for _, s in LAYOUT[kind]),
             in_item_id=0, item_id=0, rows=0, neg_item=0, sample_neg=0,
             workspace=eng.workspace.data_ptr(), workspace_bytes=eng.ws_bytes, state=eng.state.data_ptr(),
             lr=f32(1e-3), beta1=f32(0.9), beta2=f32(0.999), adam_eps=f32(1e-8), weight_decay=f32(1e-4 if kind == "gru" else 0.0),
             optimizer=_lib.OPT_ADAM, perm=0, n_perm=0, perm_stride=0, perm_offset=0, perm_counter=0, loss_log=0)
    e.update({k: (f32(v) if k == "ln_eps" else v) for k, v in SHAPE[kind].items()})
    if kind != "fmlp":
        e["seqlen"] = 0
    if kind == "sasrec":
        e["expected_tokens"] = 0
    e.update({k: t.data_ptr() for k, t in tensors.items() if t is not None})
    e.update(over)
    return e


def kept(eng):
    out = []
    for t in eng._keep:
        out += list(t) if isinstance(t, tuple) else [t]
    return out


def holds(eng, *tensors):
    return all(any(t is k for k in kept(eng)) for t in tensors)


@pytest.mark.parametrize("kind", KINDS)
def test_direct_batch_given_negatives_against_sampled(engines, kind):
    eng = engines[kind]
    assert eng.ws_bytes > 0 and eng.workspace.numel() == eng.ws_bytes
    assert eng.neg_scratch.numel() == NEG_SCRATCH[kind] and eng.neg_scratch.dtype == torch.int64
    args, t = batch(kind)
    hint = dict(expected_tokens=14) if kind == "sasrec" else {}          # 4 rows * mean_len 3.5
    neg = i64(NEG_SCRATCH[kind])
    plan = eng.make_plan(*args, neg_item=neg)
    assert fields(plan) == expected(kind, eng, MAX_B, t, neg_item=neg.data_ptr(), sample_neg=0, **hint)
    assert plan.workspace_bytes == eng.ws_bytes > 0
    assert holds(eng, neg, *[x for x in args])
    plan = eng.make_plan(*args)                                            # no negatives: the step samples into the engine's scratch
    assert fields(plan) == expected(kind, eng, MAX_B, t, neg_item=eng.neg_scratch.data_ptr(), sample_neg=1, **hint)
    assert holds(eng, eng.neg_scratch, *[x for x in args])
    plan = eng.make_plan(*args, neg_item=neg, sample_neg=True)             # the caller's buffer, filled by the step
    assert fields(plan) == expected(kind, eng, MAX_B, t, neg_item=neg.data_ptr(), sample_neg=1, **hint)


@pytest.mark.parametrize("kind", KINDS)
def test_rows_form_perm_sel_and_loss_log(engines, kind):
    eng = engines[kind]
    args, t = batch(kind)                                                  # here: dataset tensors of 4 rows
    rows = torch.tensor([2, 0, 3], dtype=torch.int64, device=DEV)
    # SASRec's hint for dataset tensors: B * mean(min(seqlen, L)) of the WHOLE tensor = 3 * 1.0
    hint = dict(expected_tokens=3) if kind == "sasrec" else {}
    plan = eng.make_plan(*args, rows=rows)
    assert fields(plan) == expected(kind, eng, 3, t, rows=rows.data_ptr(), neg_item=eng.neg_scratch.data_ptr(), sample_neg=1, **hint)
    assert holds(eng, rows)
    perm = torch.arange(10, dtype=torch.int64, device=DEV)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    log = torch.zeros(5, dtype=torch.float32, device=DEV)
    plan = eng.make_plan(*args, rows=rows, perm_sel=(perm, 6, 3, counter), loss_log=log)
    assert fields(plan) == expected(kind, eng, 3, t, rows=rows.data_ptr(), neg_item=eng.neg_scratch.data_ptr(), sample_neg=1,
                                    perm=perm.data_ptr(), n_perm=10, perm_stride=6, perm_offset=3, perm_counter=counter.data_ptr(),
                                    loss_log=log.data_ptr(), **hint)
    assert holds(eng, rows, perm, counter, log, *[x for x in args])


@pytest.mark.parametrize("kind", KINDS)
def test_optimizer_settings_are_read_when_the_plan_is_made(kind):
    eng = build(kind)
    if kind == "sasrec":
        eng.mean_len = 3.5
    eng.lr, eng.betas, eng.adam_eps, eng.weight_decay, eng.optimizer = 0.02, (0.8, 0.95), 1e-6, 0.125, _lib.OPT_RMSPROP
    eng.p_drop = 0.5
    args, t = batch(kind)
    hint = dict(expected_tokens=14) if kind == "sasrec" else {}
    plan = eng.make_plan(*args)
    assert fields(plan) == expected(kind, eng, MAX_B, t, neg_item=eng.neg_scratch.data_ptr(), sample_neg=1, lr=f32(0.02), beta1=f32(0.8),
                                    beta2=f32(0.95), adam_eps=f32(1e-6), weight_decay=f32(0.125), optimizer=_lib.OPT_RMSPROP, p_drop=0.5, **hint)


def test_sasrec_slots(engines):
    eng = engines["sasrec"]
    assert len(eng.workspaces) == len(eng.states) == 2 and eng.workspace is eng.workspaces[0] and eng.state is eng.states[0]
    assert eng.workspaces[1].numel() == eng.ws_bytes and eng.states[1].numel() == _lib.STATE_WORDS
    assert eng.workspaces[1].data_ptr() != eng.workspace.data_ptr() and eng.states[1].data_ptr() != eng.state.data_ptr()
    args, t = batch("sasrec")
    p0 = eng.make_plan(*args, slot=0)
    assert fields(p0) == expected("sasrec", eng, MAX_B, t, neg_item=eng.neg_scratch.data_ptr(), sample_neg=1, expected_tokens=14)
    assert p0.seed == SEED
    p1 = eng.make_plan(*args, slot=1)
    assert fields(p1) == expected("sasrec", eng, MAX_B, t, neg_item=eng.neg_scratch.data_ptr(), sample_neg=1, expected_tokens=14,
                                  workspace=eng.workspaces[1].data_ptr(), state=eng.states[1].data_ptr(), seed=(SEED + GOLDEN) % 2 ** 64)


def test_sasrec_expected_tokens():
    assert not torch.cuda.is_current_stream_capturing()
    eng = build("sasrec")                       # its own engine: the cache of dataset-tensor means is keyed by address, and a tensor of
    eng.mean_len = 3.5                          # an earlier test may have lived where `lens` does
    (ids, tgt, _), _ = batch("sasrec")
    lens = torch.tensor([1, 2, 3, 10], dtype=torch.int64, device=DEV)
    assert eng.make_plan(ids, tgt, lens, expected_tokens=7).expected_tokens == 7
    rows = torch.arange(4, dtype=torch.int64, device=DEV)
    assert eng.make_plan(ids, tgt, lens, rows=rows).expected_tokens == 14        # dataset tensor: 4 * mean(min(len, 8)) = 4 * 3.5
    assert eng.mean_len == 3.5
    assert eng.make_plan(ids, tgt, i64(4)).expected_tokens == 14                   # per-batch tensor: 4 * mean_len, whatever it holds
    assert eng.make_plan(ids, None, None).expected_tokens == 0


def test_sasrec_grad_buckets_for_leaves_the_kept_tensors(engines):
    eng = engines["sasrec"]
    args, _ = batch("sasrec")
    eng.make_plan(*args)
    keep = eng._keep
    assert holds(eng, *args)
    buckets = eng.grad_buckets_for(4)
    assert eng._keep is keep and holds(eng, *args)
    n = sum(math.prod(s) for _, s in LAYOUT["sasrec"])
    assert buckets[0][0] == 0 and buckets[-1][1] == n + _lib.GRAD_TAIL             # the ranges cover the flat gradient and its tail


@pytest.mark.parametrize("kind", KINDS)
def test_make_plan_errors(engines, kind):
    eng = engines[kind]
    args, _ = batch(kind)
    with pytest.raises(_lib.Dr4srError, match="batch 5 > max_batch 4"):
        eng.make_plan(i64(5, L), *args[1:])
    with pytest.raises(_lib.Dr4srError, match=r"in_item_id must be \[rows, 8\]"):
        eng.make_plan(i64(4, L - 1), *args[1:])
    if kind == "fmlp":                                                      # one query per row: [rows] targets (it has no seqlen to get wrong)
        with pytest.raises(_lib.Dr4srError, match="one query per row"):
            eng.make_plan(args[0], i64(4, L))
        return
    with pytest.raises(_lib.Dr4srError, match="one query per position"):
        eng.make_plan(args[0], i64(4), args[2])
    with pytest.raises(_lib.Dr4srError, match=r"seqlen must be \[4\]"):
        eng.make_plan(args[0], args[1], i64(3))


@pytest.mark.parametrize("kind", KINDS)
def test_views_are_the_listed_slices_of_the_flat_buffers(engines, kind):
    eng = engines[kind]
    assert list(eng.views) == list(eng.grad_views) == eng.names == [n for n, _ in LAYOUT[kind]]
    assert eng.params.numel() == eng.adam_m.numel() == eng.adam_v.numel() == eng.n_params == eng.grads.numel() - _lib.GRAD_TAIL
    off = 0
    for name, shape in LAYOUT[kind]:
        v, g = eng.views[name], eng.grad_views[name]
        assert tuple(v.shape) == tuple(g.shape) == shape and v.is_contiguous() and g.is_contiguous(), name
        assert v.data_ptr() == eng.params.data_ptr() + 4 * off and g.data_ptr() == eng.grads.data_ptr() + 4 * off, name
        off += math.prod(shape)
    assert off == eng.n_params
