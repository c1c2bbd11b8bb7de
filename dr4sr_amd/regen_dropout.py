"""Train-mode dropout of the regenerator: the sites, the element index and the numpy restatement of the kernels' keep decisions.

The kernels (csrc/regen_score_fwd.h, DropPhilox) regenerate every mask from (seed, step, site, element index) with the project's
Philox4x32-10 convention (csrc/common.h: one call covers 8 consecutive elements, 16-bit decisions, keep iff r16 >= round(p * 65536)).
This module is the exactly-equal host side: the torch restatement (regen_torch.score_forward) and the reference fixture
(tools/make_regen_train_golden.py) multiply by what keep_* return, so a float64 run sees the masks the HIP run sees.

Sites (DESIGN.md has the table): site(stack, layer, kind) with stack 0 source encoder, 1 condition encoder, 2 decoder;
an encoder layer has kinds 0 attention probabilities, 1 attention output, 2 FFN hidden, 3 FFN output; a decoder layer has
0 self probabilities, 1 self output, 2 cross probabilities, 3 cross output, 4 FFN hidden, 5 FFN output; SITE_SRC_EMB and
SITE_TGT_EMB are the two embedding sites (the condition encoder and the decoder share SITE_TGT_EMB, as the reference drops tgt_emb once).

Element index (64-bit, fixed strides: nothing depends on Ls, T, the tile or the chunk), `pair` the GLOBAL pair index pair0 + p:
  hidden sites (embeddings, attention / FFN outputs)   (pair * 64 + position) * 64 + column
  FFN hidden                                           (pair * 64 + position) * 256 + column
  attention probabilities                              ((pair * 2 + head) * 64 + query position) * 64 + key position
"""
import numpy as np

SITE_BASE = 0x52470000
SITE_SRC_EMB = SITE_BASE + 96
SITE_TGT_EMB = SITE_BASE + 97
SITE_GUMBEL = SITE_BASE + 98      # the condition head's Gumbel noise (csrc/regen_head.hip): 32-bit words, four elements per call
GUMBEL_STRIDE = 8                 # elements per pair in the noise stream's index, whatever K <= 8 is
STACK_SRC, STACK_COND, STACK_DEC = 0, 1, 2
ROWS = 64            # positions per pair in every index (the position table has 50 rows)
N_SITES = 30
_M32 = np.uint64(0xFFFFFFFF)


def site(stack: int, layer: int, kind: int) -> int:
    return SITE_BASE + stack * 32 + layer * 8 + kind


def all_sites():
    """name -> (site id, class) of the 30 sites; class is 'hidden', 'ffn' or 'probs'"""
    out = {"src_emb": (SITE_SRC_EMB, "hidden"), "tgt_emb": (SITE_TGT_EMB, "hidden")}
    for stack, stem in ((STACK_SRC, "enc"), (STACK_COND, "cond")):
        for l in range(2):
            for kind, (nm, cls) in enumerate((("probs", "probs"), ("attn_out", "hidden"), ("ffn_hidden", "ffn"), ("ffn_out", "hidden"))):
                out[f"{stem}{l}.{nm}"] = (site(stack, l, kind), cls)
    for l in range(2):
        for kind, (nm, cls) in enumerate((("self_probs", "probs"), ("self_out", "hidden"), ("cross_probs", "probs"), ("cross_out", "hidden"),
                                          ("ffn_hidden", "ffn"), ("ffn_out", "hidden"))):
            out[f"dec{l}.{nm}"] = (site(STACK_DEC, l, kind), cls)
    assert len(out) == N_SITES and len({v[0] for v in out.values()}) == N_SITES
    return out


class RegenDropout:
    """the dropout of one training step: drop probability p, and the (seed, step) that name its masks.  The same value given to the
    condition encoder's and the decoder's calls of a step makes them share the tgt_emb mask, as the reference does"""

    def __init__(self, p: float = 0.5, seed: int = 0, step: int = 0):
        if not (0.0 <= float(p) < 1.0):
            raise ValueError(f"dropout p must be in [0, 1), not {p!r}")
        self.p, self.seed, self.step = float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFF

    def __repr__(self):
        return f"RegenDropout(p={self.p}, seed={self.seed}, step={self.step})"

    def threshold(self) -> int:
        """csrc/common.h make_rng: keep iff the 16-bit draw >= round(p * 65536), computed in fp32"""
        t = np.float32(np.float32(self.p) * np.float32(65536.0) + np.float32(0.5))
        return 65535 if t >= np.float32(65535.0) else int(t)

    def scale(self) -> np.float32:
        return np.float32(1.0) / (np.float32(1.0) - np.float32(self.p))


def eval_mode(dropout) -> bool:
    """None and p = 0 are eval mode: the entry points without dropout, bit for bit"""
    if dropout is not None and not isinstance(dropout, RegenDropout):
        raise TypeError(f"dropout must be a RegenDropout or None, not {type(dropout).__name__}")
    return dropout is None or dropout.p == 0.0


def philox4x32_10(c0, c1, c2, c3, seed: int):
    """the four words of philox4x32_10(counter (c0, c1, c2, c3), key (seed low, seed high)) for uint32-valued arrays (csrc/common.h)"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def _keep8(d: RegenDropout, site_id: int, call):
    """bool [..., 8]: the keep decisions of the 8 elements of Philox call `call` (uint64 array) of the site's stream"""
    call = np.asarray(call, dtype=np.uint64)
    w = philox4x32_10(call & _M32, call >> np.uint64(32), np.uint64(site_id), np.uint64(d.step), d.seed)
    halves = []
    for x in w:
        halves += [x & np.uint64(0xFFFF), x >> np.uint64(16)]
    return np.stack(halves, -1) >= np.uint64(d.threshold())


def keep_elements(d: RegenDropout, site_id: int, idx):
    """fp32 keep factors (0 or 1 / (1 - p)) of arbitrary element indices of a site's stream"""
    idx = np.asarray(idx, dtype=np.uint64)
    calls, inv = np.unique(idx >> np.uint64(3), return_inverse=True)
    k8 = _keep8(d, site_id, calls)
    keep = k8[inv.reshape(idx.shape), (idx & np.uint64(7)).astype(np.int64)]
    return np.where(keep, d.scale(), np.float32(0.0)).astype(np.float32)


def keep_rows(d: RegenDropout, site_id: int, pairs, n_pos: int, n_col: int):
    """fp32 [n, n_pos, n_col]: the factors of a hidden (n_col 64) or FFN-hidden (n_col 256) site for the given GLOBAL pair indices"""
    pairs = np.asarray(pairs, dtype=np.uint64).reshape(-1)
    if n_pos > ROWS or n_col % 8:
        raise ValueError("a site has 64 positions per pair and its columns come in eights")
    row = pairs[:, None] * np.uint64(ROWS) + np.arange(n_pos, dtype=np.uint64)[None, :]
    call = (row[:, :, None] * np.uint64(n_col) + np.arange(0, n_col, 8, dtype=np.uint64)[None, None, :]) >> np.uint64(3)
    keep = _keep8(d, site_id, call).reshape(len(pairs), n_pos, n_col)
    return np.where(keep, d.scale(), np.float32(0.0)).astype(np.float32)


def keep_probs(d: RegenDropout, site_id: int, pairs, n_q: int, n_k: int):
    """fp32 [n, 2, n_q, n_k]: the factors of an attention-probability site (2 heads) for the given GLOBAL pair indices"""
    pairs = np.asarray(pairs, dtype=np.uint64).reshape(-1)
    if n_q > ROWS or n_k > ROWS:
        raise ValueError("a site has 64 query and 64 key positions per pair and head")
    row = ((pairs[:, None, None] * np.uint64(2) + np.arange(2, dtype=np.uint64)[None, :, None]) * np.uint64(ROWS)
           + np.arange(n_q, dtype=np.uint64)[None, None, :])
    call = (row[..., None] * np.uint64(ROWS) + np.arange(0, ROWS, 8, dtype=np.uint64)) >> np.uint64(3)
    keep = _keep8(d, site_id, call).reshape(len(pairs), 2, n_q, ROWS)[..., :n_k]
    return np.where(keep, d.scale(), np.float32(0.0)).astype(np.float32)


def gumbel_u(words):
    """fp32 uniforms of 32-bit Philox words, bit for bit the device's (csrc/regen_head.hip gumbel_of): ((r >> 8) + 0.5) * 2^-24 with
    the sum and the product rounded to fp32.  Above 2^23 the + 0.5 is a tie that rounds to even, and the largest 24-bit value would
    round up to u = 1, where -log(-log(u)) is infinite: u is held at the largest fp32 below 1, so it lies strictly inside (0, 1)"""
    r = np.asarray(words, dtype=np.uint64) & _M32
    u = ((r >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    return np.minimum(u, np.nextafter(np.float32(1.0), np.float32(0.0))).astype(np.float32)


def gumbel_words(seed: int, step: int, pairs, K: int):
    """uint64 [n, K]: the Philox words of the noise elements (pair, k) of GLOBAL pair indices: element e = pair * 8 + k is word e & 3
    of call e >> 2 of the SITE_GUMBEL stream of (seed, step)"""
    if not (1 <= int(K) <= GUMBEL_STRIDE):
        raise ValueError(f"K must be in 1..{GUMBEL_STRIDE}, not {K!r}")
    pairs = np.asarray(pairs, dtype=np.uint64).reshape(-1)
    e = pairs[:, None] * np.uint64(GUMBEL_STRIDE) + np.arange(int(K), dtype=np.uint64)[None, :]
    call = e >> np.uint64(2)
    w = np.stack(philox4x32_10(call & _M32, call >> np.uint64(32), np.uint64(SITE_GUMBEL), np.uint64(int(step) & 0xFFFFFFFF),
                               int(seed) & 0xFFFFFFFFFFFFFFFF), -1)
    return np.take_along_axis(w, (e & np.uint64(3)).astype(np.int64)[..., None], -1)[..., 0]


def gumbel_noise(seed: int, step: int, pairs, K: int):
    """float32 [n, K]: the Gumbel(0, 1) noise the condition head generates for the given GLOBAL pair indices at (seed, step).  u is
    the device's bit for bit; the two logs run in float64 here and the result is rounded to fp32 (the device's double logs may leave
    the last fp32 bit different)"""
    u = gumbel_u(gumbel_words(seed, step, pairs, K)).astype(np.float64)
    return (-np.log(-np.log(u))).astype(np.float32)
