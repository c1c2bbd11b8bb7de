"""Dataset regeneration — stage 3 of DR4SR (the reference's 3.Hybrid_inference.py) on the GPU.

The pre-trained regenerator (the reference's `Generator`: nn.Transformer d 64, 2 heads, 2 + 2 post-norm layers, FFN 256, erf-GELU,
plus `condition_linear` that turns the encoder memory into K condition memories) greedy-decodes every training sequence under each
condition; the decoded sequences, deduplicated, become new training rows of `train_regen.pth` — what `train_file: '_regen'` reads.

    model = RegenModel.from_state_dict(torch.load("regenerator.pth"), "cuda")
    model.translate([src0, src1, ...], condition=2)            # what the reference's translate() returns, one tensor per source
    hybrid_inference("dataset/amazon-toys/toy/")               # writes train_regen.pth exactly as the reference does

backend="hip" runs csrc/regen.hip through the C ABI (dr4sr_regen_encode / dr4sr_regen_decode: all steps of a chunk of rows on the
device, no host sync per token).  backend="torch" is a batched eager restatement of the same math (padding masks, full prefix
recompute); it runs on CPU or GPU and is the cross-check of the kernels, not a fall-back: nothing switches to it on its own.
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
import os

import torch
import torch.nn.functional as F

from . import _lib

D, H, FF, N_LAYER, N_POS, MAX_LEN, LN_EPS = 64, 2, 256, 2, 50, 25, 1e-12
NUM_ITEM = {"toy": 11925, "sport": 18358, "beauty": 12102, "yelp": 20034}     # 3.Hybrid_inference.py:237-242
ROWS_PER_CALL = 16384          # decode rows per HIP call: ~1.3 GB of workspace (csrc/regen.hip, about 77 KB per row)
ROWS_PER_TORCH = 2048          # decode rows per torch batch ([rows, n_rows] logits)
MAX_SEQ_LEN = 50

_ENC = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
        "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")
_DEC = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
        "multihead_attn.in_proj_weight", "multihead_attn.in_proj_bias", "multihead_attn.out_proj.weight", "multihead_attn.out_proj.bias",
        "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias",
        "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias", "norm3.weight", "norm3.bias")


def param_names():
    """state-dict names in the order of the flat layout (include/dr4sr_hip.h, dr4sr_regen_param_layout)"""
    names = ["item_embedding.weight", "position_embedding.weight"]
    names += [f"transformer.encoder.layers.{i}.{n}" for i in range(N_LAYER) for n in _ENC]
    names += ["transformer.encoder.norm.weight", "transformer.encoder.norm.bias"]
    names += [f"transformer.decoder.layers.{i}.{n}" for i in range(N_LAYER) for n in _DEC]
    names += ["transformer.decoder.norm.weight", "transformer.decoder.norm.bias"]
    names += ["condition_linear.0.weight", "condition_linear.0.bias", "condition_linear.2.weight", "condition_linear.2.bias"]
    return names


def param_shapes(n_rows: int, K: int):
    enc = [(3 * D, D), (3 * D,), (D, D), (D,), (FF, D), (FF,), (D, FF), (D,), (D,), (D,), (D,), (D,)]
    dec = [(3 * D, D), (3 * D,), (D, D), (D,), (3 * D, D), (3 * D,), (D, D), (D,), (FF, D), (FF,), (D, FF), (D,)] + [(D,)] * 6
    return ([(n_rows, D), (N_POS, D)] + enc * N_LAYER + [(D,), (D,)] + dec * N_LAYER + [(D,), (D,)]
            + [(K * D, D), (K * D,), (K * D, K * D), (K * D,)])


class RegenModel:
    """the reference's Generator at inference (eval mode: dropout off), from its state dict"""

    def __init__(self, params: dict, n_rows: int, K: int, device):
        self.device = torch.device(device)
        self.n_rows, self.K = int(n_rows), int(K)
        self.n_item = self.n_rows - 2
        self.sos, self.eos = self.n_item, self.n_item + 1
        self.p = {k: v.to(self.device, torch.float32).contiguous() for k, v in params.items()}
        self._flat = None
        self.record_gaps = None        # a list: the torch restatement appends (gap, top) [rows, 24] per batch it decodes

    @classmethod
    def from_state_dict(cls, sd: dict, device="cuda", dataset: str | None = None):
        """`sd`: the reference's regenerator.pth as saved (2.Pretrain_regenerator.py:318).  condition_encoder.* is ignored (it is
        only used in training); item_embedding_decoder.weight must be the same table as item_embedding.weight (the reference ties
        them).  N and K come from the tensors; with a known `dataset` name N is checked against the reference's num_item_dict."""
        if "item_embedding.weight" not in sd or "condition_linear.2.weight" not in sd:
            raise ValueError("not a regenerator state dict: item_embedding.weight / condition_linear.2.weight missing")
        E = sd["item_embedding.weight"]
        dec = sd.get("item_embedding_decoder.weight")
        if dec is not None and not torch.equal(dec.cpu(), E.cpu()):
            raise ValueError("item_embedding_decoder.weight differs from item_embedding.weight (the reference ties them)")
        n_rows = int(E.shape[0])
        KD = int(sd["condition_linear.2.weight"].shape[0])
        if KD % D or int(sd["condition_linear.2.weight"].shape[1]) != KD:
            raise ValueError(f"condition_linear.2.weight has shape {tuple(sd['condition_linear.2.weight'].shape)}, expected [64K, 64K]")
        K = KD // D
        if dataset is not None and dataset in NUM_ITEM and NUM_ITEM[dataset] + 2 != n_rows:
            raise ValueError(f"item table has {n_rows} rows; dataset '{dataset}' has {NUM_ITEM[dataset]} items (+ SOS, EOS)")
        params = {}
        for name, shape in zip(param_names(), param_shapes(n_rows, K)):
            if name not in sd:
                raise ValueError(f"state dict lacks {name}")
            if tuple(sd[name].shape) != shape:
                raise ValueError(f"{name}: shape {tuple(sd[name].shape)}, expected {shape}")
            params[name] = sd[name].detach()
        return cls(params, n_rows, K, device)

    # ------------------------------------------------------------------------------------------------ HIP
    def flat(self):
        """the flat fp32 parameter buffer of dr4sr_regen_param_layout"""
        if self._flat is None:
            lib = _lib.load()
            off = (C.c_int64 * _lib.REGEN_TENSORS)()
            n = lib.dr4sr_regen_param_layout(self.n_rows, self.K, off)
            if n < 0:
                _lib.check(int(n), "dr4sr_regen_param_layout")
            buf = torch.empty(int(n), dtype=torch.float32, device=self.device)
            for i, name in enumerate(param_names()):
                t = self.p[name].reshape(-1)
                buf[off[i]:off[i] + t.numel()] = t
            self._flat = buf
        return self._flat

    def plan(self):
        p = _lib.RegenPlan()
        p.abi_version = _lib.ABI_VERSION
        p.n_rows, p.K, p.max_len = self.n_rows, self.K, MAX_LEN
        p.D, p.H, p.F, p.n_layer = D, H, FF, N_LAYER
        p.ln_eps = LN_EPS
        flat = self.flat()
        p.params = flat.data_ptr()
        p.n_params = flat.numel()
        return p

    def _pack(self, src_list):
        lens = [int(len(s)) for s in src_list]
        if any(n > N_POS for n in lens):
            raise ValueError(f"a source of {max(lens)} ids: the regenerator's position table has {N_POS} rows (the reference fails "
                             f"for len(src) > {N_POS})")
        if any(n < 1 for n in lens):
            raise ValueError("an empty source")
        Ls = max(lens)
        src = torch.full((len(src_list), Ls), self.sos, dtype=torch.int64)
        for i, s in enumerate(src_list):
            src[i, :lens[i]] = torch.as_tensor(s, dtype=torch.int64).reshape(-1).cpu()
        if int(src.min()) < 0 or int(src.max()) >= self.n_rows:
            raise IndexError(f"source ids outside [0, {self.n_rows})")
        return src, torch.tensor(lens, dtype=torch.int64)

    def _decode_hip(self, src, lens, cond0, n_cond):
        """tokens [n_cond * S, MAX_LEN] int64 and len [n_cond * S] int32 (condition-major), on the host"""
        lib = _lib.load()
        plan = self.plan()
        S = src.shape[0]
        src_d, len_d = src.to(self.device).contiguous(), lens.to(self.device).contiguous()
        nb = lib.dr4sr_regen_workspace_bytes(C.byref(plan), S, n_cond)
        if nb < 0:
            _lib.check(int(nb), "dr4sr_regen_workspace_bytes")
        ws = torch.empty(int(nb), dtype=torch.uint8, device=self.device)
        tok = torch.empty(n_cond * S, MAX_LEN, dtype=torch.int64, device=self.device)
        ln = torch.empty(n_cond * S, dtype=torch.int32, device=self.device)
        st = _lib.cur_stream()
        _lib.check(lib.dr4sr_regen_encode(C.byref(plan), _lib.ptr(src_d), _lib.ptr(len_d), S, src.shape[1], cond0, n_cond,
                                          C.c_void_p(ws.data_ptr()), int(nb), st), "dr4sr_regen_encode")
        _lib.check(lib.dr4sr_regen_decode(C.byref(plan), _lib.ptr(src_d), _lib.ptr(len_d), S, src.shape[1], cond0, n_cond,
                                          C.c_void_p(ws.data_ptr()), int(nb), _lib.ptr(tok), _lib.ptr(ln), st), "dr4sr_regen_decode")
        return tok.cpu(), ln.cpu()

    # ------------------------------------------------------------------------------------------------ torch restatement
    def _mha(self, pre, xq, xkv, key_bias):
        W, b = self.p[pre + ".in_proj_weight"], self.p[pre + ".in_proj_bias"]
        B, Lq, _ = xq.shape
        Lk = xkv.shape[1]
        q = F.linear(xq, W[:D], b[:D]).view(B, Lq, H, D // H).transpose(1, 2)
        k = F.linear(xkv, W[D:2 * D], b[D:2 * D]).view(B, Lk, H, D // H).transpose(1, 2)
        v = F.linear(xkv, W[2 * D:], b[2 * D:]).view(B, Lk, H, D // H).transpose(1, 2)
        s = (q @ k.transpose(-1, -2)) / math.sqrt(D // H) + key_bias
        o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, Lq, D)
        return F.linear(o, self.p[pre + ".out_proj.weight"], self.p[pre + ".out_proj.bias"])

    def _ln(self, x, pre):
        return F.layer_norm(x, (D,), self.p[pre + ".weight"], self.p[pre + ".bias"], LN_EPS)

    def _ffn(self, x, pre):
        h = F.gelu(F.linear(x, self.p[pre + ".linear1.weight"], self.p[pre + ".linear1.bias"]))
        return F.linear(h, self.p[pre + ".linear2.weight"], self.p[pre + ".linear2.bias"])

    def _encode_torch(self, src, lens):
        """encoder (no attention mask in the reference; key padding here only hides the batch's padding) + encoder.norm"""
        E, P = self.p["item_embedding.weight"], self.p["position_embedding.weight"]
        Ls = src.shape[1]
        x = E[src] + P[:Ls]
        pad = torch.arange(Ls, device=src.device)[None, :] >= lens[:, None]
        kb = torch.zeros(pad.shape, device=src.device).masked_fill(pad, float("-inf"))[:, None, None, :]
        for i in range(N_LAYER):
            pre = f"transformer.encoder.layers.{i}"
            x = self._ln(x + self._mha(pre + ".self_attn", x, x, kb), pre + ".norm1")
            x = self._ln(x + self._ffn(x, pre), pre + ".norm2")
        return self._ln(x, "transformer.encoder.norm"), kb

    def _decode_torch(self, src, lens, cond0, n_cond, rows_per_batch=ROWS_PER_TORCH):
        src, lens = src.to(self.device), lens.to(self.device)
        S = src.shape[0]
        mem0, kb0 = self._encode_torch(src, lens)
        c1 = torch.relu(F.linear(mem0, self.p["condition_linear.0.weight"], self.p["condition_linear.0.bias"]))
        W2, b2 = self.p["condition_linear.2.weight"], self.p["condition_linear.2.bias"]
        toks, lns = [], []
        for c in range(n_cond):
            k = cond0 + c
            mem = F.linear(c1, W2[k * D:(k + 1) * D], b2[k * D:(k + 1) * D])       # features k*64:(k+1)*64 (3.Hybrid_inference.py:146)
            for a in range(0, S, rows_per_batch):
                g = None
                if self.record_gaps is not None:
                    m = min(S, a + rows_per_batch) - a
                    g = (torch.full((m, MAX_LEN - 1), float("nan"), device=self.device), torch.full((m, MAX_LEN - 1), float("nan"), device=self.device))
                    self.record_gaps.append(g)
                t, n = self._greedy_torch(src[a:a + rows_per_batch], mem[a:a + rows_per_batch], kb0[a:a + rows_per_batch], g)
                toks.append(t)
                lns.append(n)
        return torch.cat(toks).cpu(), torch.cat(lns).cpu()

    def _greedy_torch(self, src, mem, kb, gaps=None):
        """greedy_decode (3.Hybrid_inference.py:185-208) over a batch of rows, recomputing the whole prefix at each step"""
        E, P = self.p["item_embedding.weight"], self.p["position_embedding.weight"]
        R = src.shape[0]
        ys = torch.full((R, 1), self.sos, dtype=torch.int64, device=self.device)
        alive = torch.ones(R, dtype=torch.bool, device=self.device)
        n = torch.ones(R, dtype=torch.int32, device=self.device)
        for i in range(MAX_LEN - 1):
            idx = alive.nonzero().squeeze(1)
            if idx.numel() == 0:
                break
            y = ys[idx]
            T = y.shape[1]
            x = E[y] + P[:T]
            causal = torch.full((T, T), float("-inf"), device=self.device).triu(1)
            for l in range(N_LAYER):
                pre = f"transformer.decoder.layers.{l}"
                x = self._ln(x + self._mha(pre + ".self_attn", x, x, causal), pre + ".norm1")
                x = self._ln(x + self._mha(pre + ".multihead_attn", x, mem[idx], kb[idx]), pre + ".norm2")
                x = self._ln(x + self._ffn(x, pre), pre + ".norm3")
            h = self._ln(x[:, -1], "transformer.decoder.norm")
            logits = h @ E.T
            if i <= 1:      # inference_mask: ids of src (the padding repeats SOS, which is in ys) and not in ys
                allowed = torch.zeros_like(logits, dtype=torch.bool).scatter(-1, src[idx], True)
            else:           # inference_mask_generative
                allowed = torch.ones_like(logits, dtype=torch.bool)
            allowed = allowed.scatter(-1, y, False)
            masked = logits.masked_fill(~allowed, float("-inf"))
            nxt = masked.argmax(-1)
            if gaps is not None:     # best - second-best allowed logit, and the best (the cross-checks' tie rule)
                v = torch.topk(masked, 2, dim=-1).values
                gaps[0][idx, i] = v[:, 0] - v[:, 1]
                gaps[1][idx, i] = v[:, 0]
            col = torch.zeros(R, dtype=torch.int64, device=self.device)
            col[idx] = nxt
            ys = torch.cat([ys, col[:, None]], 1)
            n[idx] += 1
            alive[idx] = nxt != self.eos
        out = torch.zeros(R, MAX_LEN, dtype=torch.int64, device=self.device)
        out[:, :ys.shape[1]] = ys
        out[torch.arange(MAX_LEN, device=self.device)[None, :] >= n[:, None].long()] = 0
        return out, n

    # ------------------------------------------------------------------------------------------------ public
    @torch.no_grad()
    def decode(self, src_list, cond0: int = 0, n_cond: int | None = None, backend: str = "hip"):
        """greedy decode of every source under conditions cond0 .. cond0 + n_cond - 1: a list (condition-major, as the reference
        appends them) of token lists [SOS, ..., EOS or the 24th item]"""
        n_cond = self.K - cond0 if n_cond is None else int(n_cond)
        if not (0 <= cond0 and n_cond >= 1 and cond0 + n_cond <= self.K):
            raise ValueError(f"conditions {cond0}..{cond0 + n_cond - 1} outside 0..{self.K - 1}")
        if backend not in ("hip", "torch"):
            raise ValueError(f"backend must be 'hip' or 'torch', not {backend!r}")
        src, lens = self._pack(src_list)
        S = src.shape[0]
        per = {c: [None] * S for c in range(n_cond)}
        chunk = max(1, ROWS_PER_CALL // n_cond) if backend == "hip" else max(1, 4 * ROWS_PER_TORCH)
        for a in range(0, S, chunk):
            b = min(S, a + chunk)
            Lc = int(lens[a:b].max())
            fn = self._decode_hip if backend == "hip" else self._decode_torch
            tok, ln = fn(src[a:b, :Lc].contiguous(), lens[a:b].contiguous(), cond0, n_cond)
            tl, nl = tok.tolist(), ln.tolist()
            for c in range(n_cond):
                for j in range(b - a):
                    r = c * (b - a) + j
                    per[c][a + j] = tl[r][:nl[r]]
        return [per[c][s] for c in range(n_cond) for s in range(S)]

    @torch.no_grad()
    def decode_with_gaps(self, src_list, cond0: int = 0, n_cond: int | None = None):
        """backend="torch" decode that also returns, per row (same order) and step, the gap between the best and the second-best
        ALLOWED logit and the best logit (NaN after the row ended): a step whose gap is within rounding may legitimately differ"""
        n_cond = self.K - cond0 if n_cond is None else int(n_cond)
        self.record_gaps = []
        try:
            src, lens = self._pack(src_list)
            S = src.shape[0]
            toks = self.decode(src_list, cond0, n_cond, "torch")
            chunk = max(1, 4 * ROWS_PER_TORCH)
            gap = torch.empty(n_cond * S, MAX_LEN - 1)
            top = torch.empty(n_cond * S, MAX_LEN - 1)
            it = iter(self.record_gaps)
            for a in range(0, S, chunk):
                b = min(S, a + chunk)
                for c in range(n_cond):
                    for a2 in range(a, b, ROWS_PER_TORCH):
                        g, t = next(it)
                        m = g.shape[0]
                        gap[c * S + a2:c * S + a2 + m] = g.cpu()
                        top[c * S + a2:c * S + a2 + m] = t.cpu()
        finally:
            self.record_gaps = None
        return toks, gap, top

    def translate(self, src_list, condition: int, backend: str = "hip"):
        """the reference's translate(model, src) under set_condition(condition), for every source: one int64 tensor each"""
        return [torch.tensor(t, dtype=torch.int64) for t in self.decode(src_list, condition, 1, backend)]


def random_state_dict(n_item: int = NUM_ITEM["toy"], K: int = 5, seed: int = 0, std: float = 0.1):
    """a seeded random regenerator state dict in the reference's names (normal weights, LayerNorm weight 1 / bias 0): the
    measurement's worst case (no row stops early) and the synthetic cross-checks' model"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in zip(param_names(), param_shapes(n_item + 2, K)):
        if name.split(".")[-2].startswith("norm") or name.startswith("transformer.encoder.norm") or name.startswith("transformer.decoder.norm"):
            sd[name] = torch.ones(shape) if name.endswith("weight") else torch.zeros(shape)
        else:
            sd[name] = std * torch.randn(shape, generator=g)
    sd["item_embedding_decoder.weight"] = sd["item_embedding.weight"]
    return sd


def source_rows(original_data):
    """3.Hybrid_inference.py:250-254: [SOS] + hist[:seqlen] + [target[seqlen - 1]] + [EOS] per train row, without SOS / EOS"""
    return [list(r[1][:r[3]]) + [r[2][r[3] - 1]] for r in original_data]


def regen_rows(token_lists, max_seq_len: int = MAX_SEQ_LEN):
    """3.Hybrid_inference.py:265-290: decoded token lists (condition-major) -> the new training rows, in the reference's order"""
    train_set = set()
    for toks in token_lists:
        train_set.add(tuple(int(v) for v in toks[1:-1]))

    def truncate_or_pad(seq):
        return seq[-max_seq_len:] if len(seq) > max_seq_len else seq + [0] * (max_seq_len - len(seq))

    rows = []
    for t in train_set:
        seq = list(t)
        seq_len = sum(a != 0 for a in seq[:-1])
        if seq_len == 0:
            continue
        rows.append([1, truncate_or_pad(seq[:-1]), truncate_or_pad(seq[1:]), seq_len, [1] * max_seq_len, [0] * max_seq_len])
    return rows


def hybrid_inference(root_path: str, ckpt_name: str = "regenerator.pth", begin: int = 0, end: int = 1000000, backend: str = "hip",
                     device="cuda", out_name: str = "train_regen.pth"):
    """3.Hybrid_inference.py's __main__: reads train.pth, patterns.pth and the regenerator under root_path, decodes rows
    begin*5000 : end*5000 under every condition, writes original_rows + patterns + new_rows to train_regen.pth; returns the path"""
    parts = root_path.split("/")
    dataset = parts[-2] if len(parts) >= 2 else None        # e.g. 'toy' in './dataset/amazon-toys/toy/' (:236)
    sd = torch.load(os.path.join(root_path, ckpt_name), map_location="cpu")
    model = RegenModel.from_state_dict(sd, device, dataset=dataset)
    original_data = torch.load(os.path.join(root_path, "train.pth"))
    ori_pattern = torch.load(os.path.join(root_path, "patterns.pth"))
    seqs = source_rows(original_data)[begin * 5000:end * 5000]
    src = [[model.sos] + s + [model.eos] for s in seqs]
    tokens = model.decode(src, 0, model.K, backend) if src else []
    out_path = os.path.join(root_path, out_name)
    torch.save(original_data + ori_pattern + regen_rows(tokens), out_path)
    return out_path


def main(argv=None):
    ap = argparse.ArgumentParser(description="DR4SR stage 3: regenerate train_regen.pth with the pre-trained regenerator")
    ap.add_argument("--root_path", type=str, default="./dataset/amazon-toys/toy/", help="The path to the dataset.")
    ap.add_argument("--ckpt_name", type=str, default="regenerator.pth", help="The name of pretrained regenerator")
    ap.add_argument("--begin", "-b", type=int, default=0, help="Used for multi-processing. Beginning of the inference.")
    ap.add_argument("--end", "-e", type=int, default=1000000, help="Used for multi-processing. End of the inference.")
    ap.add_argument("--gpu", type=int, default=0)
    a = ap.parse_args(argv)
    torch.cuda.set_device(a.gpu)
    path = hybrid_inference(a.root_path, a.ckpt_name, a.begin, a.end, "hip", torch.device("cuda", a.gpu))
    print(path)


if __name__ == "__main__":
    main()
