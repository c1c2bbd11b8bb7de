"""GruEngine — flat-buffer training engine for the reference's GRU4Rec (model/gru4rec.py) on top of dr4sr_gru4rec_* (C ABI)."""
from __future__ import annotations

import torch

from . import _lib
from .flat_engine import FlatEngine


def gru_param_names(n_layer):
    names = ["item_embedding.weight"]
    for l in range(n_layer):
        names += [f"query_encoder.0.3.gru.weight_ih_l{l}", f"query_encoder.0.3.gru.weight_hh_l{l}"]
    return names + ["query_encoder.1.weight", "query_encoder.1.bias"]


def gru_param_shapes(n_items, D, H, n_layer):
    shapes = [(n_items, D)]
    for l in range(n_layer):
        shapes += [(3 * H, D if l == 0 else H), (3 * H, H)]
    return shapes + [(D, H), (D,)]


class GruEngine(FlatEngine):
    MODEL, PLAN, PREFIX, ADAM_STEP = "GRU4Rec", _lib.GruPlan, "dr4sr_gru4rec_", "dr4sr_gru4rec_adam_step"
    BUILT_FOR = "L <= 64, D = 64 or 128, hidden 128 or 256"
    POOLED = (_lib.POOL_LAST,)
    train_steps = FlatEngine._train_steps

    def __init__(self, n_items, L=50, D=64, H=256, n_layer=2, p_drop=0.2, max_batch=256, device="cuda", seed=2023, lr=1e-3,
                 betas=(0.9, 0.999), adam_eps=1e-8, weight_decay=1e-4):
        self.n_items, self.L, self.D, self.H, self.n_layer = n_items, L, D, H, n_layer     # KEPT DIFFERENCE: no F and no ln_eps
        super().__init__(gru_param_names(n_layer), gru_param_shapes(n_items, D, H, n_layer), (n_items, D, H, n_layer), L,
                         p_drop, max_batch, device, seed, lr, betas, adam_eps, weight_decay)

    def _fill_shape(self, p):
        p.L, p.D, p.H, p.n_layer, p.n_items = self.L, self.D, self.H, self.n_layer, self.n_items

    def _shape_text(self):
        return f"GRU4Rec shape L={self.L} D={self.D} hidden={self.H} layers={self.n_layer}"

    def _alloc_workspace(self):
        # KEPT DIFFERENCE: zero ONCE: the cooperative recurrence's granule tags / launch counter live in it
        return torch.zeros(self.ws_bytes, dtype=torch.uint8, device=self.device)

    def check_coop(self):
        """the cooperative recurrence never hangs: a wait that runs out sets a sticky error word (int32 word 2 of the workspace,
        include/dr4sr_hip.h) and the results of that launch are garbage — turn it into an exception (host sync: call per epoch)"""
        if int(self.workspace[:16].view(torch.int32)[2]) != 0:
            raise _lib.Dr4srError("cooperative GRU recurrence: an exchange wait timed out (workgroups not co-resident?); "
                                  "set DR4SR_GRU_NOCOOP=1 to use the single-workgroup recurrence")

    check_device_error = check_coop

    def uses_cooperative(self, B: int) -> bool:
        """True when a batch of B sequences runs the multi-CU cooperative recurrence on this device (csrc/gru_coop.hip)"""
        return bool(self.lib.dr4sr_gru4rec_uses_cooperative(int(B), int(self.H)))

    def uses_wavefront(self, B: int) -> bool:
        """True when a batch of B sequences runs both layers' forward recurrences in ONE launch, the second layer behind the first
        (csrc/gru_coop.hip k_gru_fwd_wave: two layers, hidden 256, batches the 16-slice cooperative form takes)"""
        return bool(self.lib.dr4sr_gru4rec_uses_wavefront(int(B), int(self.H), int(self.n_layer), int(self.L)))

    def loss_and_count(self):
        self.check_coop()                          # KEPT DIFFERENCE
        return super().loss_and_count()
