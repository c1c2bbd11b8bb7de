"""Exact reference tests of the evaluation top-k (csrc/topk.hip) in every launch form.

q and E hold small integers stored in fp32, so every dot product is an integer far below 2^24: exact in fp32 in ANY summation
order (the per-row FMA chains, MFMA 32x32x2).  There is therefore no tolerance: the reference is an int64 matmul on the CPU with the
PAD column, the history and the blocked items at -inf and a stable descending sort (ties -> ascending id, the rule topk.hip documents
for all its forms); scores must be torch.equal and so must the ids at every position whose reference score is finite.

Three calls serve every case: dr4sr_full_score_topk (one workgroup per row), dr4sr_full_score_topk_ws (score GEMM + selection, or the
fused form under DR4SR_TOPK_FUSED=1) and dr4sr_full_score_topk_masked_ws (item_blocked all zero: bit-identical to the unmasked call;
about half of the items blocked: its own reference).  dr4sr_full_score_topk_form (include/dr4sr_hip_hooks.h) says which form a call
takes, and after a fused call the overflow flag behind the score matrix says whether the candidate path or the two-kernel fall-back
produced the output; predict_fused() computes that flag on the CPU from the exact scores.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

NEG = float("-inf")
EMIT_CHUNK, EMIT_CAPL, CAPC, TIE_CAP, STRIDE = 512, 80, 2048, 128, 8     # csrc/topk.hip: the fused form's buffers


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dr4sr_amd import _lib
    _lib.load()                       # fail loudly if the HIP library is missing
    return torch.device("cuda")


# ------------------------------------------------------------------------------------------------ inputs (CPU, integers in fp32)
def make_tables(values, B, N, D, gen):
    """u8: entries uniform in [-8, 8] (sparse ties).  neg: q = -(|q| + 1), E = |E| + 1 (every score negative: the ~u branch of f2key).
    tern: E in {-1, 0, 1}; row b of q has m = (1, 2, 3, D)[b % 4] entries of +-1 and zeros elsewhere, so a row's scores take 2m + 1
    values only: tie groups of N / 3 (m = 1: the selection's candidate set overflows -> radix path with ordered tie compaction across
    256-wide chunks), N / 9, N / 27 at the top, and the dense row for sparse ties among small integers.
    tern3: the same with m = 3 in every row (N / 27 items share the top score)."""
    if values in ("u8", "neg"):
        q = torch.randint(-8, 9, (B, D), generator=gen)
        E = torch.randint(-8, 9, (N, D), generator=gen)
        if values == "neg":
            q, E = -(q.abs() + 1), E.abs() + 1
    else:
        E = torch.randint(-1, 2, (N, D), generator=gen)
        q = torch.zeros(B, D, dtype=torch.int64)
        for b in range(B):
            m = 3 if values == "tern3" else (1, 2, 3, D)[b % 4]
            cols = torch.randperm(D, generator=gen)[:m]
            q[b, cols] = torch.randint(0, 2, (m,), generator=gen) * 2 - 1
    return q, E


def exact_scores(q, E):
    return q.long() @ E.long().T                          # [B, N] int64: what every form must compute exactly


def make_blocked(s, gen):
    """about half of the items blocked, never the two best of any row (so that the planted history words below keep their meaning)"""
    N = s.shape[1]
    blocked = (torch.rand(N, generator=gen) < 0.5).to(torch.uint8)
    v = s.double().clone()
    v[:, 0] = NEG
    blocked[v.topk(min(2, N - 1), dim=1)[1].flatten()] = 0
    return blocked


def make_hist(s, Lh, gen):
    """a history with everything a history may hold: the row's second-best item (it must disappear), the same id again, PAD, ids
    outside [0, N) (-1, N, N + 7, 2^31 + 3) and 2^32 + the row's BEST item — a word whose low 32 bits name an item but which names
    none: every form must ignore it and return that item first — then random valid ids"""
    B, N = s.shape
    assert Lh >= 8
    v = s.double().clone()
    v[:, 0] = NEG
    top = v.topk(min(2, N - 1), dim=1)[1]
    hist = torch.randint(0, N, (B, Lh), generator=gen)
    hist[:, 0] = top[:, -1]
    hist[:, 1] = top[:, -1]
    hist[:, 2] = 0
    hist[:, 3] = -1
    hist[:, 4] = N
    hist[:, 5] = N + 7
    hist[:, 6] = 2 ** 31 + 3
    hist[:, 7] = 2 ** 32 + top[:, 0]
    return hist


def hist_mask(hist, B, N):
    m = torch.zeros(B, N, dtype=torch.bool)
    if hist is not None:
        ok = (hist >= 0) & (hist < N)
        rows = torch.arange(B).view(-1, 1).expand_as(hist)
        m[rows[ok], hist[ok]] = True
    return m


def masked_scores(s, hist, blocked):
    v = s.double().clone()                                # integers below 2^24: exact
    v[:, 0] = NEG
    if blocked is not None:
        v[:, blocked.bool()] = NEG
    v[hist_mask(hist, *s.shape)] = NEG
    return v


def reference(s, hist, blocked, k):
    """(scores [B, k] fp32, ids [B, k]) : stable descending sort = ties by ascending id; positions >= min(k, N): -inf / id 0"""
    B, N = s.shape
    srt, idx = torch.sort(masked_scores(s, hist, blocked), dim=1, descending=True, stable=True)
    kk = min(k, N)
    rs = torch.full((B, k), NEG, dtype=torch.float32)
    ri = torch.zeros(B, k, dtype=torch.int64)
    rs[:, :kk] = srt[:, :kk].float()
    ri[:, :kk] = idx[:, :kk]
    return rs, ri


def predict_fused(s, hist, blocked, k):
    """What the fused form does with these exact scores (csrc/topk.hip): the bound of a row is the k-th largest valid score of the
    subset {1 + 8 j} (history and blocked items out; -inf with fewer than k valid ones), every unblocked item (history included: it is
    dropped later) with score >= bound is a candidate.  The batch overflows when a (row, 512-item chunk) has more than 80 candidates,
    a row more than 2048, or more than 128 of a row's candidates outside its history reach the k-th score among them.
    -> (flag, worst chunk count, worst row count, worst survivor count)"""
    B, N = s.shape
    hm = hist_mask(hist, B, N)
    emit = torch.ones(N, dtype=torch.bool)
    emit[0] = False
    if blocked is not None:
        emit &= ~blocked.bool()
    v = s.double()
    sub_ids = torch.arange(1, N, STRIDE)
    sub = v[:, sub_ids].clone()
    sub[:, ~emit[sub_ids]] = NEG
    sub[hm[:, sub_ids]] = NEG
    bound = sub.sort(dim=1, descending=True)[0][:, k - 1] if sub.shape[1] >= k else torch.full((B,), NEG, dtype=torch.float64)
    cand = emit.view(1, N) & (v >= bound.view(B, 1))
    pad = (-N) % EMIT_CHUNK
    chunks = torch.nn.functional.pad(cand, (0, pad)).view(B, -1, EMIT_CHUNK).sum(-1)
    worst_chunk, worst_row = int(chunks.max()), int(cand.sum(1).max())
    live = cand & ~hm
    lv = torch.where(live, v, torch.full_like(v, NEG))
    kth = lv.sort(dim=1, descending=True)[0][:, min(k, N) - 1]           # -inf: fewer than k live candidates, all of them survive
    worst_tie = int((live & (v >= kth.view(B, 1))).sum(1).max())
    flag = int(worst_chunk > EMIT_CAPL or worst_row > CAPC or worst_tie > TIE_CAP)
    return flag, worst_chunk, worst_row, worst_tie


# ------------------------------------------------------------------------------------------------ the three calls
def lds_stride(N):
    return (N + 63) // 64 * 64


def call_per_row(dev, q, E, hist, k):
    from dr4sr_amd import _lib
    lib = _lib.load()
    B, D = q.shape
    N = E.shape[0]
    sc = torch.full((B, k), float("nan"), device=dev)
    it = torch.full((B, k), -5, dtype=torch.int64, device=dev)
    _lib.check(lib.dr4sr_full_score_topk(_lib.ptr(q), _lib.ptr(E), _lib.ptr(hist), _lib.ptr(sc), _lib.ptr(it), B, D, N,
                                         0 if hist is None else hist.shape[1], k, _lib.cur_stream()), "topk")
    return sc.cpu(), it.cpu()


def call_ws(dev, q, E, hist, blocked, k, masked):
    """-> scores, ids, form bits, the workspace's flag word after the call (-7: the call did not write it)"""
    from dr4sr_amd import _lib
    lib = _lib.load()
    B, D = q.shape
    N = E.shape[0]
    Lh = 0 if hist is None else hist.shape[1]
    nb = int(lib.dr4sr_full_score_topk_workspace_bytes(B, N))
    ws = torch.zeros(nb // 4, dtype=torch.int32, device=dev)
    ws[B * lds_stride(N)] = -7
    form = int(lib.dr4sr_full_score_topk_form(B, D, N, Lh, k, nb))
    assert form >= 0, form
    sc = torch.full((B, k), float("nan"), device=dev)
    it = torch.full((B, k), -5, dtype=torch.int64, device=dev)
    if masked:
        _lib.check(lib.dr4sr_full_score_topk_masked_ws(_lib.ptr(q), _lib.ptr(E), _lib.ptr(hist), _lib.ptr(blocked), _lib.ptr(sc),
                                                       _lib.ptr(it), B, D, N, Lh, k, _lib.ptr(ws), nb, _lib.cur_stream()), "topk_masked_ws")
    else:
        _lib.check(lib.dr4sr_full_score_topk_ws(_lib.ptr(q), _lib.ptr(E), _lib.ptr(hist), _lib.ptr(sc), _lib.ptr(it), B, D, N, Lh, k,
                                                _lib.ptr(ws), nb, _lib.cur_stream()), "topk_ws")
    return sc.cpu(), it.cpu(), form, int(ws[B * lds_stride(N)])


def assert_exact(got, ref, k, N, what):
    (sc, it), (rs, ri) = got, ref
    assert torch.equal(sc, rs), "%s: scores differ at %s" % (what, (sc != rs).nonzero()[:4].tolist())
    fin = torch.isfinite(rs)
    bad = fin & (it != ri)
    assert not bool(bad.any()), "%s: ids differ at %s: got %s, reference %s" % (what, bad.nonzero()[:4].tolist(), it[bad][:4].tolist(),
                                                                                 ri[bad][:4].tolist())
    kk = min(k, N)
    assert bool((it[:, kk:] == 0).all()) and bool(torch.isinf(sc[:, kk:]).all()), what


def run_case(dev, values, B, N, D, k, hist_kind, seed, fused=None):
    """every call of one case against its reference.  fused: None = no claim (the switch is off), else (expected bit 0, expected flag
    per mask or None).  -> {mask name: (form, flag)}"""
    gen = torch.Generator().manual_seed(seed)
    q, E = make_tables(values, B, N, D, gen)
    s = exact_scores(q, E)
    hist = make_hist(s, 12, gen) if hist_kind == "oob" else None
    blocked = make_blocked(s, gen)
    qd, Ed = q.float().to(dev), E.float().to(dev)
    hd = None if hist is None else hist.to(dev)
    ref_open, ref_half = reference(s, hist, None, k), reference(s, hist, blocked, k)
    assert_exact(call_per_row(dev, qd, Ed, hd, k), ref_open, k, N, "per-row")
    sc, it, form, flag = call_ws(dev, qd, Ed, hd, None, k, masked=False)
    assert_exact((sc, it), ref_open, k, N, "ws (form %d, flag %d)" % (form, flag))
    zeros = torch.zeros(N, dtype=torch.uint8, device=dev)
    sc0, it0, form0, flag0 = call_ws(dev, qd, Ed, hd, zeros, k, masked=True)
    assert torch.equal(sc0, sc) and torch.equal(it0, it) and (form0, flag0) == (form, flag), "a mask of zeros must change nothing"
    bd = blocked.to(dev)
    sch, ith, formh, flagh = call_ws(dev, qd, Ed, hd, bd, k, masked=True)
    assert_exact((sch, ith), ref_half, k, N, "masked_ws (form %d, flag %d)" % (formh, flagh))
    assert not bool(blocked[ith[torch.isfinite(sch)]].any())
    return {"open": (form, flag), "half": (formh, flagh)}, s, hist, blocked


# ------------------------------------------------------------------------------------------------ two-kernel form and per-row kernel
# (B, N, k, history): N = 50 with k = 100 (k > N), N = 2000: the selection keeps the row in LDS; N = 6000: it reads the workspace.
# B = 65: a second 64-row tile with 63 empty rows.  k = 1, 20, 128 (the cap).  none: Lh = 0 with hist = NULL.
SHAPES = [(1, 50, 100, "oob"), (65, 50, 20, "none"), (65, 2000, 20, "oob"), (1, 2000, 128, "none"), (65, 2000, 1, "oob"),
          (1, 6000, 20, "none"), (65, 6000, 128, "oob"), (5, 6000, 1, "oob")]


@pytest.mark.parametrize("B,N,k,hist_kind", SHAPES)
@pytest.mark.parametrize("values", ["u8", "tern", "neg"])
@pytest.mark.parametrize("D", [64, 128])
def test_topk_exact_two_kernel_and_per_row(dev, monkeypatch, D, values, B, N, k, hist_kind):
    monkeypatch.delenv("DR4SR_TOPK_FUSED", raising=False)
    forms, _, _, _ = run_case(dev, values, B, N, D, k, hist_kind, seed=1000 * D + N + k + B)
    want = 2 if N <= 2000 else 0                          # bit 1: row in LDS; bit 0 never without the switch
    assert forms["open"] == (want, -7) and forms["half"] == (want, -7), forms


@pytest.mark.parametrize("D", [64, 128])
def test_topk_exact_through_the_torch_op_without_history(dev, D):
    """torch.ops.dr4sr_hip.full_score_topk(q, E, None, item_blocked, k): hist = NULL with Lh = 0 reaches the library"""
    import dr4sr_amd.ops  # noqa: F401  (registers the ops)
    B, N, k = 3, 2000, 20
    gen = torch.Generator().manual_seed(77 + D)
    q, E = make_tables("tern", B, N, D, gen)
    s = exact_scores(q, E)
    blocked = make_blocked(s, gen)
    for bl in (None, blocked):
        sc, it = torch.ops.dr4sr_hip.full_score_topk(q.float().to(dev), E.float().to(dev), None, None if bl is None else bl.to(dev), k)
        assert_exact((sc.cpu(), it.cpu()), reference(s, None, bl, k), k, N, "op, blocked %s" % (bl is not None))


# ------------------------------------------------------------------------------------------------ fused form
def test_topk_form_query_pins_the_fused_boundary(dev, monkeypatch):
    """Per row the fused form's buffers take 4 sub_s + 8 * 2048 + 8 bytes (+ 256 once) and must fit in front of the 4 lds_s bytes of
    the score row: N = 4736 -> 18 952 > 18 944, never; N = 4737 -> 18 952 + 256 / B <= 19 200 from B = 2 on; one row needs N >= 4801."""
    from dr4sr_amd import _lib
    lib = _lib.load()

    def form(B, N, k=20, D=64, slack=0):
        return int(lib.dr4sr_full_score_topk_form(B, D, N, 12, k, int(lib.dr4sr_full_score_topk_workspace_bytes(B, N)) + slack))
    monkeypatch.delenv("DR4SR_TOPK_FUSED", raising=False)
    assert form(2, 4737) == 2 and form(65, 11925) == 0 and form(2, 2000) == 2          # without the switch: never fused
    monkeypatch.setenv("DR4SR_TOPK_FUSED", "1")
    for D in (64, 128):
        assert form(2, 4095, D=D) & 1 == 0 and form(70, 4096, k=128, D=D) & 1 == 0
        assert form(2, 4736, D=D) & 1 == 0 and form(65, 4736, D=D) & 1 == 0
        assert form(1, 4737, D=D) & 1 == 0 and form(2, 4737, D=D) & 1 == 1 and form(65, 4737, D=D) & 1 == 1
        assert form(1, 4800, D=D) & 1 == 0 and form(1, 4801, D=D) & 1 == 1
        assert form(2, 11925, k=100, D=D) == 1 and form(2, 11925, k=128, D=D) == 1
    assert form(2, 4737) == 3 and form(2, 6000) == 1                                   # bit 1: the fall-back's selection, row in LDS up to 24 KiB
    # errors the call would return: k outside [1, 128], n_items < 2 (ARG = -1), an unsupported width (SHAPE = -2), a short workspace (WS = -3)
    assert form(2, 4737, k=0) == -1 and form(2, 4737, k=129) == -1 and form(2, 1) == -1 and form(2, 4737, D=96) == -2
    assert form(2, 4737, slack=-257) == -3 and form(2, 4737, slack=-256) >= 0


# name: (values, B, N, k, claimed flag).  The claims are CONDITIONS on the inputs, checked on the CPU by predict_fused before the GPU
# runs: (a) the candidate path's own output is compared (worst chunk <= 70 of 80, worst row <= 1500 of 2048, survivors <= 128);
# (b) a 512-item chunk holds clearly more than 80 candidates (k * 8 = 1024 expected over 10 chunks); (c) clearly more than 128 items
# tie at the k-th score (N / 27 items share a row's top score 3) while no chunk and no row is near its limit.
FUSED = {
    "a_k20_smallest": ("u8", 2, 4737, 20, 0),
    "a_k20_one_row": ("u8", 1, 4801, 20, 0),
    "a_k20_two_row_tiles": ("u8", 65, 4800, 20, 0),
    "a_k100": ("u8", 3, 11925, 100, 0),
    "a_k1_negative": ("neg", 2, 4800, 1, 0),
    "b_chunk_overflow": ("u8", 2, 4800, 128, 1),
    "b_chunk_overflow_two_row_tiles": ("u8", 65, 4800, 128, 1),
    "c_tie_overflow": ("tern3", 2, 12000, 20, 1),
}
FUSED_SEED = 1


@pytest.mark.parametrize("name", list(FUSED))
@pytest.mark.parametrize("D", [64, 128])
def test_topk_exact_fused(dev, monkeypatch, D, name):
    values, B, N, k, claim = FUSED[name]
    monkeypatch.setenv("DR4SR_TOPK_FUSED", "1")
    forms, s, hist, blocked = run_case(dev, values, B, N, D, k, "oob", seed=FUSED_SEED + D)
    for mask, bl in (("open", None), ("half", blocked)):
        flag, chunk, row, tie = predict_fused(s, hist, bl, k)
        what = "%s D=%d %s: worst chunk %d / %d, worst row %d / %d, survivors at the k-th score %d / %d" % (
            name, D, mask, chunk, EMIT_CAPL, row, CAPC, tie, TIE_CAP)
        if name.startswith("a"):
            assert chunk <= 70 and row <= 1500 and tie <= TIE_CAP, what
        elif name.startswith("b"):
            assert chunk >= 96, what
        else:
            assert tie >= 160 and chunk <= 70 and row <= 1500, what
        assert flag == claim, what
        assert forms[mask][0] & 1 == 1, "%s: the call was not fused (form %d)" % (what, forms[mask][0])
        assert forms[mask][1] == flag, "%s: overflow flag %d, predicted %d" % (what, forms[mask][1], flag)


@pytest.mark.parametrize("D", [64, 128])
def test_topk_exact_just_below_the_fused_boundary(dev, monkeypatch, D):
    """N = 4736 under the switch: the form query says two-kernel, the flag word stays untouched, the result is exact"""
    monkeypatch.setenv("DR4SR_TOPK_FUSED", "1")
    forms, _, _, _ = run_case(dev, "u8", 2, 4736, D, 20, "oob", seed=9 + D)
    assert forms["open"] == (2, -7) and forms["half"] == (2, -7), forms


# ------------------------------------------------------------------------------------------------ float inputs against float64
@pytest.mark.parametrize("D", [64, 128])
def test_topk_float_against_float64(dev, monkeypatch, D):
    """0.1 randn tables, every call (per-row, two-kernel, fused; open and half-blocked) against float64 scores.  margin = twice the
    worst error of CPU fp32 q @ E.T against the same float64 (the rule of test_propagate_against_float64): the returned score of
    every returned id lies within it, and every float64 top-k item is returned unless its score is within it of the k-th score."""
    B, N, k, Lh = 8, 6000, 20, 12
    gen = torch.Generator().manual_seed(31 + D)
    q = torch.randn(B, D, generator=gen)
    E = 0.1 * torch.randn(N, D, generator=gen)
    s64 = q.double() @ E.double().T
    margin = 2.0 * float(((q @ E.T).double() - s64).abs().max())
    hist = make_hist(s64, Lh, gen)
    blocked = make_blocked(s64, gen)
    qd, Ed, hd, bd = q.to(dev), E.to(dev), hist.to(dev), blocked.to(dev)

    def check(sc, it, bl, what):
        v = s64.clone()
        v[:, 0] = NEG
        if bl is not None:
            v[:, bl.bool()] = NEG
        v[hist_mask(hist, B, N)] = NEG
        rs, ri = v.topk(k, dim=1)
        assert bool(torch.isfinite(sc).all()) and bool((sc[:, 1:] <= sc[:, :-1]).all()), what
        err = float((v.gather(1, it) - sc.double()).abs().max())
        assert err <= margin, "%s: returned scores off by %.3g, margin %.3g" % (what, err, margin)
        for b in range(B):
            missing = ri[b][~torch.isin(ri[b], it[b])]
            gap = float((v[b, missing] - rs[b, -1]).abs().max()) if missing.numel() else 0.0
            assert gap <= margin, "%s: row %d misses items %s, %.3g above the k-th score (margin %.3g)" % (what, b, missing.tolist(), gap, margin)
    check(*call_per_row(dev, qd, Ed, hd, k), None, "per-row")
    for fused in (False, True):
        if fused:
            monkeypatch.setenv("DR4SR_TOPK_FUSED", "1")
        else:
            monkeypatch.delenv("DR4SR_TOPK_FUSED", raising=False)
        sc, it, form, flag = call_ws(dev, qd, Ed, hd, None, k, masked=False)
        assert form & 1 == int(fused)
        check(sc, it, None, "ws form %d flag %d" % (form, flag))
        sc, it, form, flag = call_ws(dev, qd, Ed, hd, bd, k, masked=True)
        assert form & 1 == int(fused)
        check(sc, it, blocked, "masked_ws form %d flag %d" % (form, flag))
