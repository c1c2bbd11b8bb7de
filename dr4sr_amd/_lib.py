"""ctypes binding of libdr4sr_hip.so (the C ABI declared in include/dr4sr_hip.h).

There is NO fallback: if the HIP library is missing or fails to load, importing any compute path
of dr4sr_amd raises.  PyTorch is only used for device memory and streams (tensor.data_ptr(),
torch.cuda.current_stream().cuda_stream).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DR4SR_LIB_PATH") or os.path.join(_HERE, "csrc", "libdr4sr_hip.so")     # override: A/B runs of two builds on one box

ABI_VERSION = 10
COMM_ID_BYTES = 128           # DR4SR_COMM_ID_BYTES (the RCCL unique id, a host buffer)
GRAD_TAIL = 4
STATE_WORDS = 16
STATE_STEP, STATE_T, STATE_NVALID, STATE_RNGSTEP = 0, 1, 2, 3
POOL_NONE, POOL_ORIGIN, POOL_LAST, POOL_MEAN = 0, 1, 2, 3
SITE_EMB, SITE_ATTN, SITE_PROJ, SITE_ACT, SITE_FFN = 0, 1, 2, 3, 4
OPT_ADAM, OPT_SGD, OPT_ADAGRAD, OPT_RMSPROP = 0, 1, 2, 3        # DR4SR_OPT_* (include/dr4sr_hip.h)
RANK_NONE = 2 ** 31 - 1       # DR4SR_RANK_NONE: dr4sr_target_rank's answer for a row whose target is not a valid item
RANK_METRICS = ("ndcg", "recall", "precision", "map", "mrr", "hit", "f1")      # slot order of dr4sr_rank_metrics_accumulate


def check_ids(idx, n_items: int, what: str = "index"):
    """raise what torch.nn.Embedding raises for ids outside [0, n_items) — the HIP gathers clamp them (csrc/embed.hip).  One small
    launch + one host read: for dataset tensors (once) and the dense API op, never inside the fused training step"""
    import torch
    if idx is None or idx.numel() == 0:
        return
    bad = torch.zeros(1, dtype=torch.int32, device=idx.device)
    t = idx.contiguous()
    check(load().dr4sr_check_ids(ptr(t), t.numel(), int(n_items), ptr(bad), cur_stream()), "dr4sr_check_ids")
    if int(bad):
        raise IndexError(f"index out of range in self ({what}: {int(bad)} ids outside [0, {int(n_items)}))")


def set_env(name: str, value=None):
    """set (value=None: unset) a DR4SR_* switch in os.environ AND make the loaded library read it: libdr4sr_hip.so caches every switch
    per call site until dr4sr_reload_env() bumps its generation (csrc/common.h), so a plain os.environ change after the first call of an
    entry point would be silently ignored"""
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = str(value)
    if _lib is not None:
        _lib.dr4sr_reload_env()


def optimizer_settings(name: str, weight_decay: float):
    """/root/reference model/basemodel.py:79-98 -> (DR4SR_OPT_* kind, (beta1, beta2), eps, weight_decay): each optimizer with torch's
    defaults as the reference constructs it — Adam(lr, weight_decay), SGD(lr, weight_decay) (no momentum), Adagrad(lr, weight_decay)
    (eps 1e-10, lr_decay 0, accumulator 0), RMSprop(lr, weight_decay) (alpha 0.99 carried in beta2, eps 1e-8, no momentum, not
    centered); an UNKNOWN name falls back to Adam(lr) without weight decay, as the reference's else branch does.  'sparse_adam': the
    reference builds torch.optim.SparseAdam over dense nn.Embedding gradients, which raises at its first step — the same RuntimeError
    is raised here, when the optimizer is built."""
    n = str(name).lower()
    if n == "adam":
        return OPT_ADAM, (0.9, 0.999), 1e-8, float(weight_decay)
    if n == "sgd":
        return OPT_SGD, (0.9, 0.999), 1e-8, float(weight_decay)
    if n == "adagrad":
        return OPT_ADAGRAD, (0.9, 0.999), 1e-10, float(weight_decay)
    if n == "rmsprop":
        return OPT_RMSPROP, (0.9, 0.99), 1e-8, float(weight_decay)
    if n == "sparse_adam":
        raise RuntimeError("SparseAdam does not support dense gradients, please consider Adam instead")
    return OPT_ADAM, (0.9, 0.999), 1e-8, 0.0

KERNEL_IDS = {"prep": 0, "embed_fwd": 1, "qkv_fwd": 2, "attn_fwd": 3, "post_fwd": 4, "score": 5, "transpose": 6,
              "post_bwd": 7, "attn_bwd": 8, "qkv_bwd": 9, "embed_bwd": 10, "wgrad": 11, "adam": 12, "zero_grads": 13,
              "embqkv_fwd": 14, "post_mid": 15, "qkv_embed_bwd": 16, "wgrad_fused": 17}

FMLP_KERNEL_IDS = {"filter_fwd": 0, "ffn_fwd": 1, "ffn_bwd": 2, "filter_bwd": 3, "wgrad": 4}      # DR4SR_FK_* (include/dr4sr_hip_hooks.h)

_f32p = C.c_void_p
_i64p = C.c_void_p


# The three training plans of include/dr4sr_hip.h are mostly the same fields in the same order; the blocks they share, in struct order:
_PLAN_BUFFERS = [("seed", C.c_uint64),
                 ("params", _f32p), ("grads", _f32p), ("adam_m", _f32p), ("adam_v", _f32p),
                 ("n_params", C.c_int64)]
_PLAN_WORKSPACE = [("sample_neg", C.c_int32),
                   ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                   ("state", C.c_void_p)]
_PLAN_OPTIMIZER = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("adam_eps", C.c_float), ("weight_decay", C.c_float)]
_PLAN_PERM_LOG = [("perm", _i64p), ("n_perm", C.c_int64), ("perm_stride", C.c_int64), ("perm_offset", C.c_int64),
                  ("perm_counter", C.c_void_p),
                  ("loss_log", _f32p)]


def _i32(*names):
    return [(n, C.c_int32) for n in names]


def _ptrs(*names):
    return [(n, _i64p) for n in names]


class SasrecPlan(C.Structure):
    """mirror of `dr4sr_sasrec_plan` (include/dr4sr_hip.h); the only plan that ends ..., loss_log, expected_tokens, optimizer"""
    _fields_ = (_i32("abi_version", "B", "L", "D", "H", "F", "n_layer", "n_items") + [("ln_eps", C.c_float), ("p_drop", C.c_float)]
                + _PLAN_BUFFERS + _ptrs("in_item_id", "item_id", "seqlen", "rows", "neg_item") + _PLAN_WORKSPACE + _PLAN_OPTIMIZER
                + _PLAN_PERM_LOG + _i32("expected_tokens", "optimizer"))


class SasrecInputs(C.Structure):
    """mirror of `dr4sr_sasrec_inputs` (include/dr4sr_hip.h): the encoder's optional per-token input scale and its gradient"""
    _fields_ = [("input_weight", _f32p), ("d_input_weight", _f32p)]


LAYER_TENSORS = ("in_proj_weight", "in_proj_bias", "out_proj_weight", "out_proj_bias", "linear1_weight", "linear1_bias", "linear2_weight",
                 "linear2_bias", "norm1_weight", "norm1_bias", "norm2_weight", "norm2_bias")


class LayerWeights(C.Structure):
    """mirror of `dr4sr_layer_weights` (include/dr4sr_hip.h): the 12 tensors of one encoder layer in the flat layout's order"""
    _fields_ = [(n, _f32p) for n in LAYER_TENSORS]


class LayerGrads(C.Structure):
    """mirror of `dr4sr_layer_grads` (include/dr4sr_hip.h): the same 12, writable"""
    _fields_ = [(n, _f32p) for n in LAYER_TENSORS]


FMLP_LAYER_TENSORS = ("complex_weight", "filter_ln_weight", "filter_ln_bias", "dense_1_weight", "dense_1_bias", "dense_2_weight", "dense_2_bias",
                      "inter_ln_weight", "inter_ln_bias")


class FmlpLayerWeights(C.Structure):
    """mirror of `dr4sr_fmlp_layer_weights` (include/dr4sr_hip.h): the 9 tensors of one FMLP layer in the flat layout's order"""
    _fields_ = [(n, _f32p) for n in FMLP_LAYER_TENSORS]


class FmlpLayerGrads(C.Structure):
    """mirror of `dr4sr_fmlp_layer_grads` (include/dr4sr_hip.h): the same 9, writable"""
    _fields_ = [(n, _f32p) for n in FMLP_LAYER_TENSORS]


class MetaWeighting(C.Structure):
    """mirror of `dr4sr_meta_weighting` (include/dr4sr_hip.h)"""
    _fields_ = [("phi", _f32p), ("gumbel", _f32p), ("user_id", _i64p), ("gate_in", C.c_void_p), ("gate_out", C.c_void_p),
                ("weight_out", _f32p), ("tau", C.c_float)]


class FmlpPlan(C.Structure):
    """mirror of `dr4sr_fmlp_plan` (include/dr4sr_hip.h): no H, no seqlen"""
    _fields_ = (_i32("abi_version", "B", "L", "D", "F", "n_layer", "n_items") + [("ln_eps", C.c_float), ("p_drop", C.c_float)]
                + _PLAN_BUFFERS + _ptrs("in_item_id", "item_id", "rows", "neg_item") + _PLAN_WORKSPACE + _PLAN_OPTIMIZER
                + _i32("optimizer") + _PLAN_PERM_LOG)


class GruPlan(C.Structure):
    """mirror of `dr4sr_gru4rec_plan` (include/dr4sr_hip.h): no F, no ln_eps"""
    _fields_ = (_i32("abi_version", "B", "L", "D", "H", "n_layer", "n_items") + [("p_drop", C.c_float)]
                + _PLAN_BUFFERS + _ptrs("in_item_id", "item_id", "seqlen", "rows", "neg_item") + _PLAN_WORKSPACE + _PLAN_OPTIMIZER
                + _i32("optimizer") + _PLAN_PERM_LOG)


class RegenPlan(C.Structure):
    """mirror of `dr4sr_regen_plan` (include/dr4sr_hip.h, ABI 9)"""
    _fields_ = [
        ("abi_version", C.c_int32),
        ("n_rows", C.c_int32), ("K", C.c_int32), ("max_len", C.c_int32),
        ("D", C.c_int32), ("H", C.c_int32), ("F", C.c_int32), ("n_layer", C.c_int32),
        ("ln_eps", C.c_float),
        ("params", _f32p),
        ("n_params", C.c_int64),
    ]


REGEN_TENSORS = 70            # DR4SR_REGEN_TENSORS
REGEN_SCORE_TENSORS = 98      # DR4SR_REGEN_SCORE_TENSORS

_PLANP = C.POINTER(SasrecPlan)
_FPLANP = C.POINTER(FmlpPlan)
_GPLANP = C.POINTER(GruPlan)
_RPLANP = C.POINTER(RegenPlan)

# name -> (restype, argtypes); every symbol include/dr4sr_hip.h and include/dr4sr_hip_hooks.h (test / measurement hooks) declare
SYMBOLS = {
    "dr4sr_abi_version": (C.c_int, []),
    "dr4sr_sasrec_plan_sizeof": (C.c_int, []),
    "dr4sr_sasrec_param_layout": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "dr4sr_sasrec_workspace_bytes": (C.c_int64, [_PLANP]),
    "dr4sr_sasrec_workspace_offsets": (C.c_int, [_PLANP, C.c_int32, C.POINTER(C.c_int64)]),
    "dr4sr_sasrec_at_scale": (C.c_int, [C.c_void_p]),
    "dr4sr_sasrec_fwd_bwd": (C.c_int, [_PLANP, C.c_void_p]),
    "dr4sr_adam_step": (C.c_int, [_PLANP, C.c_void_p]),
    "dr4sr_sasrec_fwd_bwd_weighted": (C.c_int, [_PLANP, C.c_void_p, C.c_void_p]),
    "dr4sr_sasrec_fwd_bwd_weighted_prepared": (C.c_int, [_PLANP, C.c_void_p, C.c_void_p]),
    "dr4sr_sasrec_train_step": (C.c_int, [_PLANP, C.c_void_p]),
    "dr4sr_sasrec_train_steps": (C.c_int, [_PLANP, C.c_int32, C.c_void_p]),
    "dr4sr_sasrec_fwd_bwd_prepared": (C.c_int, [_PLANP, C.c_void_p]),
    "dr4sr_adam_step_prepare_next": (C.c_int, [_PLANP, C.c_void_p]),
    "dr4sr_sasrec_grad_buckets": (C.c_int, [_PLANP, C.POINTER(C.c_int64)]),
    "dr4sr_sasrec_fwd_bwd_phase": (C.c_int, [_PLANP, C.c_int32, C.c_int32, C.c_void_p]),
    "dr4sr_sasrec_encode": (C.c_int, [_PLANP, C.c_int32, C.c_int32, _f32p, C.c_void_p]),
    "dr4sr_sasrec_encode_bwd": (C.c_int, [_PLANP, C.c_int32, C.c_int32, _f32p, C.c_void_p]),
    "dr4sr_sasrec_encode_w": (C.c_int, [_PLANP, C.POINTER(SasrecInputs), C.c_int32, C.c_int32, _f32p, C.c_void_p]),
    "dr4sr_sasrec_encode_w_bwd": (C.c_int, [_PLANP, C.POINTER(SasrecInputs), C.c_int32, C.c_int32, _f32p, C.c_void_p]),
    "dr4sr_select_rows": (C.c_int, [_i64p, C.c_int64, _i64p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "dr4sr_embed_gather_posadd": (C.c_int, [_f32p, _f32p, _i64p, _f32p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "dr4sr_score_bce_fwd": (C.c_int, [_f32p, _f32p, _i64p, _i64p, _f32p, _f32p, _f32p, _f32p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "dr4sr_score_bce_bwd": (C.c_int, [_f32p, _f32p, _i64p, _i64p, _f32p, _f32p, _f32p, _f32p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "dr4sr_score_bpr_fwd": (C.c_int, [_f32p, _f32p, _i64p, _i64p, _f32p, _f32p, _f32p, _f32p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "dr4sr_score_bpr_bwd": (C.c_int, [_f32p, _f32p, _i64p, _i64p, _f32p, _f32p, _f32p, _f32p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "dr4sr_loss_from_scores_fwd": (C.c_int, [_f32p, _f32p, C.c_int64, C.c_int32, C.c_int32, _f32p, _f32p, C.c_void_p]),
    "dr4sr_loss_from_scores_bwd": (C.c_int, [_f32p, _f32p, C.c_int64, C.c_int32, C.c_int32, _f32p, _f32p, _f32p, _f32p, C.c_void_p]),
    "dr4sr_neg_sample": (C.c_int, [_i64p, C.c_int64, C.c_int32, C.c_uint64, C.c_uint32, C.c_void_p]),
    "dr4sr_neg_sample_dev": (C.c_int, [_i64p, C.c_int64, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p]),
    "dr4sr_dropout_mask": (C.c_int, [_f32p, C.c_int64, C.c_float, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p]),
    "dr4sr_fmlp_plan_sizeof": (C.c_int, []),
    "dr4sr_fmlp_param_layout": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "dr4sr_fmlp_workspace_bytes": (C.c_int64, [_FPLANP]),
    "dr4sr_fmlp_fwd_bwd": (C.c_int, [_FPLANP, C.c_void_p]),
    "dr4sr_fmlp_train_step": (C.c_int, [_FPLANP, C.c_void_p]),
    "dr4sr_fmlp_encode": (C.c_int, [_FPLANP, C.c_int32, _f32p, C.c_void_p]),
    "dr4sr_fmlp_encode_bwd": (C.c_int, [_FPLANP, C.c_int32, _f32p, C.c_void_p]),
    "dr4sr_gru4rec_plan_sizeof": (C.c_int, []),
    "dr4sr_gru4rec_param_layout": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "dr4sr_gru4rec_workspace_bytes": (C.c_int64, [_GPLANP]),
    "dr4sr_gru4rec_uses_cooperative": (C.c_int, [C.c_int32, C.c_int32]),
    "dr4sr_gru4rec_uses_wavefront": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "dr4sr_gru4rec_fwd_bwd": (C.c_int, [_GPLANP, C.c_void_p]),
    "dr4sr_gru4rec_train_step": (C.c_int, [_GPLANP, C.c_void_p]),
    "dr4sr_gru4rec_encode": (C.c_int, [_GPLANP, C.c_int32, C.c_int32, _f32p, C.c_void_p]),
    "dr4sr_gru4rec_encode_bwd": (C.c_int, [_GPLANP, C.c_int32, C.c_int32, _f32p, C.c_void_p]),
    "dr4sr_adam_flat": (C.c_int, [_f32p, _f32p, _f32p, _f32p, C.c_int64, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "dr4sr_reload_env": (C.c_int, []),
    "dr4sr_build_flags": (C.c_int, []),
    "dr4sr_sasrec_launch_kernel": (C.c_int, [_PLANP, C.c_int32, C.c_int32, C.c_void_p]),
    "dr4sr_sasrec_launch_kernel_weighted": (C.c_int, [_PLANP, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "dr4sr_gru4rec_launch_kernel": (C.c_int, [_GPLANP, C.c_int32, C.c_int32, C.c_void_p]),
    "dr4sr_fmlp_launch_kernel": (C.c_int, [_FPLANP, C.c_int32, C.c_int32, C.c_void_p]),
    "dr4sr_meta_param_count": (C.c_int64, [C.c_int32]),
    "dr4sr_meta_select_workspace_floats": (C.c_int64, [C.c_int64]),
    "dr4sr_meta_select_workspace_floats_d": (C.c_int64, [C.c_int64, C.c_int32]),
    "dr4sr_meta_select_fwd": (C.c_int, [_f32p, _f32p, _f32p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_float, _i64p, _i64p, C.c_int64, C.c_int32,
                                        C.c_int32, C.c_void_p, C.c_void_p, _f32p, C.c_void_p]),
    "dr4sr_meta_select_bwd": (C.c_int, [_f32p, _f32p, _f32p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_float, _i64p, _i64p, C.c_int64, C.c_int32,
                                        C.c_int32, C.c_void_p, _f32p, _f32p, _f32p, _f32p, _f32p, C.c_void_p]),
    "dr4sr_meta_select_fwd_d": (C.c_int, [_f32p, _f32p, _f32p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_float, _i64p, _i64p, C.c_int64, C.c_int32,
                                          C.c_int32, C.c_void_p, C.c_void_p, _f32p, C.c_void_p]),
    "dr4sr_meta_select_bwd_d": (C.c_int, [_f32p, _f32p, _f32p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_float, _i64p, _i64p, C.c_int64, C.c_int32,
                                          C.c_int32, C.c_void_p, _f32p, _f32p, _f32p, _f32p, _f32p, C.c_void_p]),
    "dr4sr_fd_step_size": (C.c_int, [_f32p, _f32p, C.c_int64, C.c_float, _f32p, C.c_void_p]),
    "dr4sr_fd_step_size_scratch_floats": (C.c_int64, []),
    "dr4sr_fd_step_size_ws": (C.c_int, [_f32p, _f32p, C.c_int64, C.c_float, _f32p, _f32p, C.c_void_p]),
    "dr4sr_fd_shift": (C.c_int, [_f32p, _f32p, _f32p, _f32p, C.c_float, C.c_int64, C.c_void_p]),
    "dr4sr_fd_neumann": (C.c_int, [_f32p, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p, C.c_float, C.c_int64, C.c_void_p]),
    "dr4sr_fd_diff": (C.c_int, [_f32p, _f32p, _f32p, _f32p, _f32p, _f32p, C.c_float, C.c_int64, C.c_void_p]),
    "dr4sr_fd_diff4": (C.c_int, [_f32p, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p, C.c_float, C.c_int64, C.c_void_p]),
    "dr4sr_scale_by": (C.c_int, [_f32p, _f32p, _f32p, C.c_int64, C.c_void_p]),
    "dr4sr_meta_opt_step": (C.c_int, [C.c_int32, _f32p, _f32p, _f32p, _f32p, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                      C.c_float, C.c_void_p, _f32p, C.c_void_p]),
    "dr4sr_meta_sgd_step": (C.c_int, [_f32p, _f32p, _f32p, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p,
                                      _f32p, C.c_void_p]),
    "dr4sr_cl_augment": (C.c_int, [_i64p, _i64p, _i64p, _i64p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double,
                                   C.c_int64, C.c_uint64, C.c_uint32, C.c_void_p]),
    "dr4sr_cl_augment_dev": (C.c_int, [_i64p, _i64p, _i64p, _i64p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double,
                                       C.c_int64, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p]),
    "dr4sr_cl_augment2_dev": (C.c_int, [_i64p, _i64p, _i64p, _i64p, _i64p, _i64p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                        C.c_double, C.c_int64, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p]),
    "dr4sr_cl_augment2_rows_dev": (C.c_int, [_i64p, _i64p, _i64p, _i64p, _i64p, _i64p, _i64p, C.c_int32, C.c_int32, C.c_int32, C.c_double,
                                             C.c_double, C.c_double, C.c_int64, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p]),
    "dr4sr_cl_prepare": (C.c_int, [_i64p, C.c_int32, C.c_void_p, _f32p, _f32p, C.c_int64, C.c_void_p]),
    "dr4sr_cl_prepare_rows": (C.c_int, [_i64p, _i64p, C.c_int32, C.c_void_p, _f32p, _f32p, C.c_int64, C.c_void_p]),
    "dr4sr_cl_prepare_rows_step": (C.c_int, [_i64p, _i64p, C.c_int32, C.c_void_p, _f32p, _f32p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]),
    "dr4sr_infonce_bwd_scaled": (C.c_int, [_f32p, _f32p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, _f32p, _f32p, _f32p, C.c_float, C.c_int32,
                                           _f32p, _f32p, C.c_void_p]),
    "dr4sr_cl_scalars": (C.c_int, [_f32p, _f32p, C.c_float, _f32p, _f32p, C.c_void_p]),
    "dr4sr_fmlp_adam_step": (C.c_int, [_FPLANP, C.c_void_p]),
    "dr4sr_gru4rec_adam_step": (C.c_int, [_GPLANP, C.c_void_p]),
    "dr4sr_gru4rec_train_steps": (C.c_int, [_GPLANP, C.c_int32, C.c_void_p]),
    "dr4sr_check_ids": (C.c_int, [_i64p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "dr4sr_optimizer_flat": (C.c_int, [C.c_int32, _f32p, _f32p, _f32p, _f32p, C.c_int64, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float,
                                       C.c_float, C.c_void_p]),
    "dr4sr_cl_scalars_dp": (C.c_int, [_f32p, C.c_int32, C.c_int64, _f32p, C.c_float, _f32p, _f32p, C.c_void_p]),
    "dr4sr_infonce_fwd": (C.c_int, [_f32p, _f32p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, _f32p, _f32p, _f32p, C.c_void_p]),
    "dr4sr_infonce_bwd": (C.c_int, [_f32p, _f32p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, _f32p, _f32p, _f32p, _f32p, C.c_void_p]),
    "dr4sr_full_score_topk": (C.c_int, [_f32p, _f32p, _i64p, _f32p, _i64p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "dr4sr_full_score_topk_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int32]),
    "dr4sr_full_score_topk_masked_ws": (C.c_int, [_f32p, _f32p, _i64p, C.c_void_p, _f32p, _i64p, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                                  C.c_int32, _f32p, C.c_int64, C.c_void_p]),
    "dr4sr_full_score_topk_ws": (C.c_int, [_f32p, _f32p, _i64p, _f32p, _i64p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                           _f32p, C.c_int64, C.c_void_p]),
    "dr4sr_full_score_topk_form": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64]),          # test hook (include/dr4sr_hip_hooks.h)
    # ABI 8: the data-parallel transport (csrc/comm.hip, RCCL on the caller's stream); comm handles are opaque pointers
    "dr4sr_comm_unique_id": (C.c_int, [C.c_void_p]),
    "dr4sr_comm_init_rank": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "dr4sr_comm_destroy": (C.c_int, [C.c_void_p]),
    "dr4sr_comm_rank": (C.c_int, [C.c_void_p]),
    "dr4sr_comm_world": (C.c_int, [C.c_void_p]),
    "dr4sr_comm_async_error": (C.c_int, [C.c_void_p]),
    "dr4sr_comm_error_string": (C.c_char_p, [C.c_int]),
    "dr4sr_allreduce_f32": (C.c_int, [C.c_void_p, _f32p, C.c_int64, C.c_void_p]),
    "dr4sr_allreduce_f64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    "dr4sr_allreduce_f32_async": (C.c_int, [C.c_void_p, _f32p, C.c_int64, C.c_void_p]),
    "dr4sr_comm_join": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dr4sr_allgather_bytes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "dr4sr_broadcast_bytes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    # ABI 9: dataset regeneration (csrc/regen.hip)
    "dr4sr_regen_plan_sizeof": (C.c_int, []),
    "dr4sr_regen_param_layout": (C.c_int64, [C.c_int32, C.c_int32, C.c_void_p]),
    "dr4sr_regen_workspace_bytes": (C.c_int64, [_RPLANP, C.c_int64, C.c_int32]),
    "dr4sr_regen_encode": (C.c_int, [_RPLANP, _i64p, _i64p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "dr4sr_regen_decode": (C.c_int, [_RPLANP, _i64p, _i64p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, _i64p,
                                     C.c_void_p, C.c_void_p]),
    # ABI 10: the regenerator's pre-training pairs (csrc/pairs.hip)
    "dr4sr_pairs_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int32]),
    "dr4sr_pairs_match": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, _i64p, C.c_int64, C.c_int64, C.c_uint64, C.c_int64,
                                    C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    # additive to ABI 10: pattern mining for the regenerator (csrc/mine.hip)
    "dr4sr_mine_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int32, C.c_int64]),
    "dr4sr_mine_patterns": (C.c_int, [C.c_void_p, _i64p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_int64,
                                      C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, _i64p, C.c_void_p]),
    # additive to ABI 10: teacher-forced scoring of the regenerator (csrc/regen_score.hip)
    "dr4sr_regen_score_param_layout": (C.c_int64, [C.c_int32, C.c_int32, C.c_void_p]),
    "dr4sr_regen_score_workspace_bytes": (C.c_int64, [_RPLANP, C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "dr4sr_regen_score_condition": (C.c_int, [_RPLANP, _i64p, _i64p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, _f32p, C.c_void_p]),
    "dr4sr_regen_score": (C.c_int, [_RPLANP, _i64p, _i64p, _i64p, _i64p, C.c_int64, C.c_int32, C.c_int32, _f32p, C.c_int32, C.c_int32,
                                    C.c_void_p, C.c_int64, _f32p, C.c_void_p]),
    # additive to ABI 10: gradients of teacher-forced scoring (csrc/regen_score_bwd.hip)
    "dr4sr_regen_score_bwd_workspace_bytes": (C.c_int64, [_RPLANP, C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "dr4sr_regen_score_bwd": (C.c_int, [_RPLANP, _i64p, _i64p, _i64p, _i64p, C.c_int64, C.c_int32, C.c_int32, _f32p, C.c_int32, C.c_int32, _f32p,
                                        C.c_void_p, C.c_int64, _f32p, _f32p, _f32p, C.c_int32, C.c_void_p]),
    "dr4sr_regen_score_condition_bwd_workspace_bytes": (C.c_int64, [_RPLANP, C.c_int64, C.c_int32]),
    "dr4sr_regen_score_condition_bwd": (C.c_int, [_RPLANP, _i64p, _i64p, C.c_int64, C.c_int32, _f32p, C.c_void_p, C.c_int64, _f32p, C.c_int32,
                                                  C.c_void_p]),
    # additive to ABI 10: train mode (dropout) of the four teacher-forced calls: (p, seed, step, pair0) in front of the stream
    "dr4sr_regen_score_condition_train": (C.c_int, [_RPLANP, _i64p, _i64p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, _f32p,
                                                    C.c_float, C.c_uint64, C.c_uint32, C.c_int64, C.c_void_p]),
    "dr4sr_regen_score_train": (C.c_int, [_RPLANP, _i64p, _i64p, _i64p, _i64p, C.c_int64, C.c_int32, C.c_int32, _f32p, C.c_int32, C.c_int32,
                                          C.c_void_p, C.c_int64, _f32p, C.c_float, C.c_uint64, C.c_uint32, C.c_int64, C.c_void_p]),
    "dr4sr_regen_score_bwd_train": (C.c_int, [_RPLANP, _i64p, _i64p, _i64p, _i64p, C.c_int64, C.c_int32, C.c_int32, _f32p, C.c_int32, C.c_int32,
                                              _f32p, C.c_void_p, C.c_int64, _f32p, _f32p, _f32p, C.c_int32, C.c_float, C.c_uint64, C.c_uint32,
                                              C.c_int64, C.c_void_p]),
    "dr4sr_regen_score_condition_bwd_train": (C.c_int, [_RPLANP, _i64p, _i64p, C.c_int64, C.c_int32, _f32p, C.c_void_p, C.c_int64, _f32p,
                                                        C.c_int32, C.c_float, C.c_uint64, C.c_uint32, C.c_int64, C.c_void_p]),
    # additive to ABI 10: the condition head of the pre-training step (csrc/regen_head.hip)
    "dr4sr_regen_head_fwd": (C.c_int, [_f32p, _f32p, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_int64, C.c_uint64, C.c_uint32, C.c_int64,
                                       _f32p, _f32p, _f32p, _f32p, C.c_void_p]),
    "dr4sr_regen_head_bwd": (C.c_int, [_f32p, _f32p, _f32p, _f32p, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_int64, C.c_int64,
                                       _f32p, _f32p, _f32p, C.c_int64, C.c_void_p]),
    # additive to ABI 10: graph propagation of the item table for the GNN model (csrc/gnn.hip)
    "dr4sr_gnn_split_rows": (C.c_int32, []),
    "dr4sr_gnn_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int64]),
    "dr4sr_gnn_propagate": (C.c_int, [_i64p, C.c_void_p, _f32p, C.c_int32, C.c_int32, C.c_int32, _f32p, _f32p, C.c_int32, C.c_void_p, C.c_int64,
                                      C.c_void_p]),
    # additive to ABI 10: evaluation by target rank + metric sums on the device (csrc/rank.hip)
    "dr4sr_target_rank_workspace_bytes": (C.c_int64, [C.c_int64]),
    "dr4sr_target_rank": (C.c_int, [_f32p, _f32p, _i64p, _i64p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                    C.c_int64, C.c_void_p]),
    "dr4sr_rank_metrics_accumulate": (C.c_int, [C.c_void_p, _f32p, C.c_int64, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_void_p,
                                                C.c_void_p]),
    "dr4sr_crash_line_set": (C.c_int, [C.c_char_p, C.c_int32, C.c_int32]),           # measurement hook (include/dr4sr_hip_hooks.h)
    # additive to ABI 10: the stateless encoder-layer op, sequence pooling and dropout on dense tensors (csrc/layer_op.hip)
    "dr4sr_sasrec_layer_saved_floats": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "dr4sr_sasrec_layer_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "dr4sr_sasrec_layer_fwd": (C.c_int, [_f32p, C.c_void_p, C.c_int32, C.POINTER(LayerWeights), C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_float, C.c_float, C.c_uint64, C.c_uint32, C.c_int32, _f32p, _f32p, C.c_void_p]),
    "dr4sr_sasrec_layer_bwd": (C.c_int, [_f32p, C.c_void_p, C.c_int32, C.POINTER(LayerWeights), C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_float, C.c_float, C.c_uint64, C.c_uint32, C.c_int32, _f32p, _f32p, _f32p,
                                         C.POINTER(LayerGrads), C.c_void_p, C.c_int64, C.c_void_p]),
    "dr4sr_seq_pool_fwd": (C.c_int, [_f32p, _i64p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _f32p, C.c_void_p]),
    "dr4sr_seq_pool_bwd": (C.c_int, [_f32p, _i64p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _f32p, C.c_void_p]),
    "dr4sr_dropout_apply": (C.c_int, [_f32p, C.c_int64, C.c_float, C.c_uint64, C.c_uint32, C.c_uint32, _f32p, C.c_void_p]),
    "dr4sr_embed_gather_posadd_bwd": (C.c_int, [_f32p, _i64p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f32p, _f32p, C.c_void_p]),
    # additive to ABI 10: the stateless FMLP layer op and the LayerNorm op on dense tensors (csrc/fmlp_op.hip)
    "dr4sr_fmlp_layer_saved_floats": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "dr4sr_fmlp_layer_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "dr4sr_fmlp_layer_fwd": (C.c_int, [_f32p, C.POINTER(FmlpLayerWeights), C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float,
                                       C.c_uint64, C.c_uint32, C.c_int32, _f32p, _f32p, C.c_void_p, C.c_int64, C.c_void_p]),
    "dr4sr_fmlp_layer_bwd": (C.c_int, [_f32p, C.POINTER(FmlpLayerWeights), C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float,
                                       C.c_uint64, C.c_uint32, C.c_int32, _f32p, _f32p, _f32p, C.POINTER(FmlpLayerGrads), C.c_void_p, C.c_int64,
                                       C.c_void_p]),
    "dr4sr_layer_norm_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int32]),
    "dr4sr_layer_norm_fwd": (C.c_int, [_f32p, _f32p, _f32p, C.c_int64, C.c_int32, C.c_float, _f32p, C.c_void_p]),
    "dr4sr_layer_norm_bwd": (C.c_int, [_f32p, _f32p, C.c_int64, C.c_int32, C.c_float, _f32p, _f32p, _f32p, _f32p, C.c_void_p, C.c_int64,
                                       C.c_void_p]),
    # additive to ABI 10: the stateless GRU layer op on dense tensors (csrc/gru_op.hip)
    "dr4sr_gru_layer_saved_floats": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "dr4sr_gru_layer_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "dr4sr_gru_layer_fwd": (C.c_int, [_f32p, _f32p, _f32p, _i64p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _f32p, _f32p, C.c_void_p,
                                      C.c_int64, C.c_void_p]),
    "dr4sr_gru_layer_bwd": (C.c_int, [_f32p, _f32p, _f32p, _i64p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _f32p, _f32p, _f32p, _f32p,
                                      _f32p, _f32p, C.c_void_p, C.c_int64, C.c_void_p]),
    # additive to ABI 10: the encoder-layer op with sequence lengths, short sequences sharing a tile (csrc/layer_packed.hip)
    "dr4sr_sasrec_layer_packed_saved_floats": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "dr4sr_sasrec_layer_packed_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "dr4sr_sasrec_layer_packed_fwd": (C.c_int, [_f32p, _i64p, C.c_int32, C.POINTER(LayerWeights), C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                                C.c_int32, C.c_float, C.c_float, C.c_uint64, C.c_uint32, C.c_int32, _f32p, _f32p, C.c_void_p,
                                                C.c_int64, C.c_void_p]),
    "dr4sr_sasrec_layer_packed_bwd": (C.c_int, [_f32p, _i64p, C.c_int32, C.POINTER(LayerWeights), C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                                C.c_int32, C.c_float, C.c_float, C.c_uint64, C.c_uint32, C.c_int32, _f32p, _f32p, _f32p,
                                                C.POINTER(LayerGrads), C.c_void_p, C.c_int64, C.c_void_p]),
}

_lib = None


class Dr4srError(RuntimeError):
    pass


# additive entry points of ABI 10 that a library named by DR4SR_LIB_PATH (the OTHER build of an A/B run, tools/lib_ab.sh) may predate; the
# tree's own library must export them like every other symbol
_AFTER_PARENT_AB = ("dr4sr_sasrec_encode_w", "dr4sr_sasrec_encode_w_bwd", "dr4sr_mine_workspace_bytes", "dr4sr_mine_patterns",
                    "dr4sr_sasrec_layer_saved_floats", "dr4sr_sasrec_layer_workspace_bytes", "dr4sr_sasrec_layer_fwd", "dr4sr_sasrec_layer_bwd",
                    "dr4sr_seq_pool_fwd", "dr4sr_seq_pool_bwd", "dr4sr_dropout_apply", "dr4sr_embed_gather_posadd_bwd",
                    "dr4sr_fmlp_layer_saved_floats", "dr4sr_fmlp_layer_workspace_bytes", "dr4sr_fmlp_layer_fwd", "dr4sr_fmlp_layer_bwd",
                    "dr4sr_layer_norm_workspace_bytes", "dr4sr_layer_norm_fwd", "dr4sr_layer_norm_bwd",
                    "dr4sr_gru_layer_saved_floats", "dr4sr_gru_layer_workspace_bytes", "dr4sr_gru_layer_fwd", "dr4sr_gru_layer_bwd",
                    "dr4sr_sasrec_layer_packed_saved_floats", "dr4sr_sasrec_layer_packed_workspace_bytes", "dr4sr_sasrec_layer_packed_fwd",
                    "dr4sr_sasrec_layer_packed_bwd")


def load():
    """dlopen the library once and type every entry point.  Raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise Dr4srError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C dr4sr_amd/csrc`).  dr4sr_amd has no CPU / PyTorch fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        if name in _AFTER_PARENT_AB and os.environ.get("DR4SR_LIB_PATH") and not hasattr(lib, name):
            continue                     # an older build under A/B: the call raises AttributeError where it is made
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    v = lib.dr4sr_abi_version()
    if v != ABI_VERSION:
        raise Dr4srError(f"libdr4sr_hip.so ABI {v} != binding ABI {ABI_VERSION}")
    if lib.dr4sr_sasrec_plan_sizeof() != C.sizeof(SasrecPlan):
        raise Dr4srError("ctypes mirror of dr4sr_sasrec_plan does not match the compiled struct")
    if lib.dr4sr_fmlp_plan_sizeof() != C.sizeof(FmlpPlan):
        raise Dr4srError("ctypes mirror of dr4sr_fmlp_plan does not match the compiled struct")
    if lib.dr4sr_gru4rec_plan_sizeof() != C.sizeof(GruPlan):
        raise Dr4srError("ctypes mirror of dr4sr_gru4rec_plan does not match the compiled struct")
    if lib.dr4sr_regen_plan_sizeof() != C.sizeof(RegenPlan):
        raise Dr4srError("ctypes mirror of dr4sr_regen_plan does not match the compiled struct")
    _lib = lib
    return lib


# probe entry points (include/dr4sr_hip_probes.h): device primitives run on their own, for tests/.  Bound on first use, not in load(): a
# library built before they existed must still load through DR4SR_LIB_PATH
LANE_PROBE_NAMES = ("group16_sum", "group8_sum", "wave_sum", "xg_max", "xg_sum", "fold", "xor1")      # DR4SR_LP_*
PROBE_SYMBOLS = {
    "dr4sr_lane_probe": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    # the tile plan of the packed encoder-layer op on its own (csrc/layer_packed.hip)
    "dr4sr_sasrec_layer_packed_chunk": (C.c_int32, []),
    "dr4sr_sasrec_layer_packed_plan": (C.c_int, [_i64p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                                 C.c_void_p]),
}


def probe(name: str):
    """a typed probe entry point of the loaded library; raises if the library does not export it"""
    fn = getattr(load(), name)           # AttributeError if the symbol is not exported
    fn.restype, fn.argtypes = PROBE_SYMBOLS[name]
    return fn


_ERR = {-1: "DR4SR_E_ARG (null pointer / bad size)", -2: "DR4SR_E_SHAPE (unsupported D/H/F/L)",
        -3: "DR4SR_E_WS (workspace too small)"}


def check(rc: int, what: str):
    if rc != 0:
        raise Dr4srError(f"{what} failed: {_ERR.get(rc, 'hipError_t ' + str(rc))}")


def ptr(t):
    """device pointer of a contiguous torch tensor (or None)"""
    if t is None:
        return None
    assert t.is_contiguous(), "dr4sr_amd kernels need contiguous tensors"
    return C.c_void_p(t.data_ptr())


def cur_stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
