"""What the tests of torch.ops.dr4sr_hip.sasrec_layer_packed share: the tile plan of csrc/layer_packed.hip stated in plain Python, the
masks of post-padded rows, and the float64 yardstick (tests/_layer_ref.py with key_pad = pos >= n_b and a d_out zeroed at the pads)."""
import torch

import _layer_ref as LR

TILE_ROWS = 64


def clamp(seqlen, L):
    return [min(max(int(n), 0), L) for n in seqlen]


def plan(seqlen, L, C):
    """-> (tile_of, row_of, n_tiles): the sequences in index order, in chunks of C planned independently; a chunk starts a tile; a
    sequence without rows belongs to no tile (-1, -1); one that does not fit behind the rows of the open tile starts the next"""
    n = clamp(seqlen, L)
    tile_of, row_of, tiles = [-1] * len(n), [-1] * len(n), 0
    for c0 in range(0, len(n), C):
        is_open, r = False, 0
        for b in range(c0, min(c0 + C, len(n))):
            if n[b] == 0:
                continue
            if not is_open or r + n[b] > TILE_ROWS:
                tiles, r, is_open = tiles + 1, 0, True
            tile_of[b], row_of[b] = tiles - 1, r
            r += n[b]
    return tile_of, row_of, tiles


def check_plan(seqlen, L, C, tile_of, row_of, n_tiles):
    """the properties a plan must have, whoever made it"""
    n = clamp(seqlen, L)
    members = {}
    for b, (t, r) in enumerate(zip(tile_of, row_of)):
        if n[b] == 0:
            assert t == -1, (b, t)
            continue
        assert 0 <= t < n_tiles and r >= 0, (b, t, r)                    # in exactly one tile (it has one entry)
        members.setdefault(t, []).append(b)
    assert sorted(members) == list(range(n_tiles)), "tiles are numbered without gaps"
    last_first = -1
    for t in range(n_tiles):
        bs = members[t]
        assert bs[0] > last_first, "tiles are numbered in the order of their first sequence"
        last_first = bs[0]
        assert len({b // C for b in bs}) == 1, ("one chunk", t, bs)
        between = [b for b in range(bs[0], bs[-1] + 1) if n[b] > 0]
        assert between == bs, ("consecutive", t, bs)
        end = 0
        for b in bs:                                                    # rows in sequence order, no overlap, no more than 64
            assert row_of[b] >= end, ("overlap", t, b)
            end = row_of[b] + n[b]
        assert end <= TILE_ROWS, (t, end)


def valid_mask(seqlen, L):
    """[B, L] bool: pos < n_b"""
    n = torch.tensor(clamp(seqlen, L)).view(-1, 1)
    return torch.arange(L).view(1, L) < n


def zero_pads(t, seqlen):
    return torch.where(valid_mask(seqlen, t.shape[1]).unsqueeze(-1), t, torch.zeros((), dtype=t.dtype))


def fill_pads(t, seqlen, value):
    return torch.where(valid_mask(seqlen, t.shape[1]).unsqueeze(-1), t, torch.full((), value, dtype=t.dtype))


def ref64(x, seqlen, p, H, eps, causal, d_out, n_layer=1, masks=None, pdrop=0.0):
    """-> (y, dx, {name: gradient}) in float64; d_out is zeroed at the pads, so no gradient carries anything from a pad row"""
    L = x.shape[1]
    p64 = {k: v.double() for k, v in p.items()}
    m64 = None if masks is None else {k: v.double() for k, v in masks.items()}
    return LR.layer_grads(x.double(), ~valid_mask(seqlen, L), p64, H, eps, causal, zero_pads(d_out.double(), seqlen), n_layer, m64, pdrop)
