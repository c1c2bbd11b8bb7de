"""FMLP with the class surface of the reference's model/fmlp.py (FMLP :8-51) and module/layers.py:740-807
(FilterLayer, Intermediate, Layer, FMLPEncoder), carrying parameters under the reference's state-dict names:
  item_embedding.weight, position_embeddings.weight, LayerNorm.{weight,bias},
  item_encoder.layer.{i}.filterlayer.{complex_weight, LayerNorm.*}, item_encoder.layer.{i}.intermediate.{dense_1,dense_2,LayerNorm}.*
Every Parameter is a view into FmlpEngine's flat buffer; arithmetic runs in libdr4sr_hip.so (dr4sr_fmlp_*).
As in the reference, sizes are fixed (L = 50, D = 64, hidden 256), dropout is 0.5 regardless of configs/fmlp.yaml, and
forward returns the encoder output at the LAST position in train and eval — the data must be per-prefix, left-padded rows
with scalar targets (dataset/dataset_transform.ipynb of the reference; README.md:78)."""
from __future__ import annotations

import torch
import torch.nn as nn

from ..fmlp_engine import FmlpEngine
from .basemodel import FlatEngineModel, _Encode
from .sasrec import _Embedding, _LayerNorm, _Linear, _bind


class FilterLayer(nn.Module):
    def __init__(self, eng, prefix):
        super().__init__()
        _bind(self, "complex_weight", eng.views[prefix + "complex_weight"], eng.grad_views[prefix + "complex_weight"])
        self.complex_weight.data.copy_(torch.randn(self.complex_weight.shape) * 0.02)       # layers.py:743
        self.out_dropout = nn.Dropout(0.5)
        self.LayerNorm = _LayerNorm(eng, prefix + "LayerNorm.", 64, 1e-12)


class Intermediate(nn.Module):
    def __init__(self, eng, prefix):
        super().__init__()
        self.dense_1 = _Linear(eng, prefix + "dense_1.", 256, 64)
        self.dense_2 = _Linear(eng, prefix + "dense_2.", 64, 256)
        self.LayerNorm = _LayerNorm(eng, prefix + "LayerNorm.", 64, 1e-12)
        self.dropout = nn.Dropout(0.5)


class Layer(nn.Module):
    def __init__(self, eng, prefix):
        super().__init__()
        self.filterlayer = FilterLayer(eng, prefix + "filterlayer.")
        self.intermediate = Intermediate(eng, prefix + "intermediate.")


class FMLPEncoder(nn.Module):
    def __init__(self, eng, num_hidden_layers=2):
        super().__init__()
        self.layer = nn.ModuleList([Layer(eng, f"item_encoder.layer.{i}.") for i in range(num_hidden_layers)])
        for lyr in self.layer[1:]:               # the reference deep-copies ONE layer: identical complex_weight everywhere
            lyr.filterlayer.complex_weight.data.copy_(self.layer[0].filterlayer.complex_weight.data)


class FMLP(FlatEngineModel):
    _raw_enc_args = ()                 # one query per row, the last position's: the engine's encode takes no pooling

    def _plan_args(self, fields):    # ... and its make_plan no lengths (left-padded rows)
        return ()

    def __init__(self, config, dataset_list) -> None:
        super().__init__(config, dataset_list)
        if self.embed_dim != 64 or self.max_seq_len != 50:
            raise ValueError("FMLP hard-codes embed_dim 64 and max_seq_len 50 (reference model/fmlp.py:11-12)")
        self.engine = FmlpEngine(self.num_items, 50, 64, 256, config["model"]["layer_num"], 1e-12, 0.5, self._max_batch(config),
                                 self.device, **self._engine_kw())
        self.device = self.engine.device
        eng = self.engine
        self.item_embedding = _Embedding(eng, "item_embedding.weight", self.num_items, 64, padding_idx=0)
        self.position_embeddings = _Embedding(eng, "position_embeddings.weight", 50, 64)
        self.LayerNorm = _LayerNorm(eng, "LayerNorm.", 64, 1e-12)
        self.dropout = nn.Dropout(0.5)
        self.item_encoder = FMLPEncoder(eng, num_hidden_layers=config["model"]["layer_num"])
        self._alloc_step_buffers(1)

    def forward(self, batch, need_pooling=True):
        return _Encode.apply(self, self.item_embedding.weight, batch["in_" + self.fiid], (), {}, bool(self.training), ())
