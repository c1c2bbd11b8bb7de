"""Unit tests of the flat-vector helpers of the first-order hyper-gradient (csrc/meta.hip k_fd_*, k_scale_by): each kernel against
the formula of include/dr4sr_hip.h (the Hypergrad block) evaluated in float64 on the CPU.

n = 1, 255, 256, 257, 1000: one thread, one workgroup less one, exactly one, one more, several; n = 65 537 = 256 workgroups x 256
threads + 1: a second grid-stride trip in k_fd_step_size and a partial last workgroup in the elementwise kernels.

Bounds.  step size: relative 2e-6 (~32 fp32 epsilons: the longest chain of the two-level sum has 2 + 6 + 4 + 6 + 4 additions, then
a divide, a square root and a multiply).  shift: one fused multiply-add, 1 ulp of the float64 value.  neumann / diff / diff4 /
scale_by: the subtracted terms cancel, so the bound is absolute: 8 * 2^-24 times the sum of the MAGNITUDES of the terms (times the
outer factor) — every operation of the chain (two divides, the subtraction, the divide by 2e, the scale) rounds once, each relative
to a value no larger than that sum, and diff4's longest chain has seven of them.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 1000, 65537]
EPS8 = 8.0 * 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dr4sr_amd import _lib
    _lib.load()                       # fail loudly if the HIP library is missing
    return torch.device("cuda")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def step_size_data(n, seed):
    g = torch.Generator().manual_seed(seed)
    theta = torch.randn(n, generator=g)
    d = torch.randn(n, generator=g)
    d[torch.rand(n, generator=g) < 0.3] = 0.0             # ~30 % exact zeros: those elements of theta do not count either
    if n == 1:
        d[0] = 0.75
    return theta, d


def step_size_ref(theta, d, rel):
    t, dd = theta.double(), d.double()
    sd = float((dd * dd).sum())
    return float(torch.tensor(rel, dtype=torch.float32)) * (float((t * t)[dd != 0].sum()) / sd) ** 0.5 if sd > 0 else 0.0


@pytest.mark.parametrize("n", SIZES)
def test_fd_step_size(dev, n):
    from dr4sr_amd import _lib
    lib = _lib.load()
    rel = 1e-2
    scratch = torch.zeros(int(lib.dr4sr_fd_step_size_scratch_floats()), device=dev)

    def run_ws(theta, d):
        out = torch.full((1,), float("nan"), device=dev)
        _lib.check(lib.dr4sr_fd_step_size_ws(_lib.ptr(theta), _lib.ptr(d), n, rel, _lib.ptr(out), _lib.ptr(scratch), _lib.cur_stream()), "fd_step_size_ws")
        return out.cpu()
    th, d = step_size_data(n, n)
    thd, dd = th.to(dev), d.to(dev)
    ref = step_size_ref(th, d, rel)
    assert ref > 0
    e = [run_ws(thd, dd) for _ in range(3)]               # one scratch, three calls: the ticket is reset by every call
    err = abs(float(e[0]) - ref) / ref
    assert err <= 2e-6, "n = %d: e = %.9g, float64 %.9g, relative error %.3g" % (n, float(e[0]), ref, err)
    assert torch.equal(bits(e[0]), bits(e[1])) and torch.equal(bits(e[0]), bits(e[2])), [float(x) for x in e]
    th2, d2 = step_size_data(n, n + 7)                    # other data on the same scratch: no partial of the earlier calls survives
    th2 = 3.0 * th2
    th2d, d2d = th2.to(dev), d2.to(dev)
    ref2 = step_size_ref(th2, d2, rel)
    e2 = run_ws(th2d, d2d)
    err2 = abs(float(e2) - ref2) / ref2
    assert err2 <= 2e-6, "n = %d, second data set: e = %.9g, float64 %.9g, relative error %.3g" % (n, float(e2), ref2, err2)
    zero = torch.zeros(n, device=dev)
    ez = run_ws(th2d, zero)                               # no direction at all: exactly 0 (not 0 / 0)
    assert torch.equal(bits(ez), torch.zeros(1, dtype=torch.int32)), float(ez)
    e3 = run_ws(thd, dd)                                  # ... and the scratch still serves the first data set to the bit
    assert torch.equal(bits(e3), bits(e[0]))
    # the module-scratch form: same kernel, same reduction tree -> same bits; strictly after the calls above on the same stream
    torch.cuda.synchronize()
    for theta_d, dir_d, want in ((thd, dd, e[0]), (th2d, d2d, e2), (th2d, zero, ez), (thd, dd, e[0])):
        out = torch.full((1,), float("nan"), device=dev)
        _lib.check(lib.dr4sr_fd_step_size(_lib.ptr(theta_d), _lib.ptr(dir_d), n, rel, _lib.ptr(out), _lib.cur_stream()), "fd_step_size")
        torch.cuda.synchronize()
        assert torch.equal(bits(out), bits(want)), (float(out), float(want))


@pytest.mark.parametrize("n", SIZES)
def test_fd_shift(dev, n):
    from dr4sr_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(100 + n)
    x, d = torch.randn(n, generator=g), torch.randn(n, generator=g)
    e = torch.tensor([3.1e-3])
    xd, dd, ed = x.to(dev), d.to(dev), e.to(dev)
    for sign in (1.0, -1.0, 2.0, -2.0):
        out = torch.full((n,), float("nan"), device=dev)
        _lib.check(lib.dr4sr_fd_shift(_lib.ptr(out), _lib.ptr(xd), _lib.ptr(dd), _lib.ptr(ed), sign, n, _lib.cur_stream()), "fd_shift")
        ref = x.double() + (sign * e).float().double() * d.double()                # sign * e is exact in fp32 for +-1, +-2
        r32 = ref.float().abs()
        ulp = (torch.nextafter(r32, torch.full_like(r32, float("inf"))) - r32).double()
        err = (out.cpu().double() - ref).abs()
        assert bool((err <= ulp).all()), "n = %d, sign %g: worst error %.3g ulp" % (n, sign, float((err / ulp).max()))
    assert torch.equal(xd.cpu(), x) and torch.equal(dd.cpu(), d)


def _words(dev, *vals):
    return torch.tensor(list(vals), dtype=torch.float32, device=dev)


@pytest.mark.parametrize("n", SIZES)
def test_fd_diff_diff4_scale_by(dev, n):
    from dr4sr_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(200 + n)
    f = [torch.randn(n, generator=g) for _ in range(4)]
    f[1] = f[0] + 1e-3 * f[1]                             # the probes nearly cancel, as in a real central difference
    f[3] = f[2] + 2e-3 * f[3]
    fd = [t.to(dev) for t in f]
    nv = [37.0, 41.0, 43.0, 47.0]                         # four different n_valid words
    nvd, e, coef = _words(dev, *nv), 2.5e-3, -0.7
    ed = _words(dev, e)
    e32, c32 = float(ed.cpu()), float(torch.tensor(coef, dtype=torch.float32))
    a = [f[i].double() / nv[i] for i in range(4)]
    # diff
    out = torch.full((n,), float("nan"), device=dev)
    _lib.check(lib.dr4sr_fd_diff(_lib.ptr(out), _lib.ptr(fd[0]), _lib.ptr(fd[1]), _lib.ptr(nvd[0:1]), _lib.ptr(nvd[1:2]), _lib.ptr(ed), coef, n,
                                 _lib.cur_stream()), "fd_diff")
    ref = c32 * (a[0] - a[1]) / (2 * e32)
    bound = EPS8 * abs(c32) * (a[0].abs() + a[1].abs()) / (2 * e32)
    err = (out.cpu().double() - ref).abs()
    assert bool((err <= bound).all()), "diff n = %d: worst error / bound %.3g" % (n, float((err / bound).max()))
    # diff4: (4 D(e) - D(2e)) / 3
    out4 = torch.full((n,), float("nan"), device=dev)
    _lib.check(lib.dr4sr_fd_diff4(_lib.ptr(out4), _lib.ptr(fd[0]), _lib.ptr(fd[1]), _lib.ptr(fd[2]), _lib.ptr(fd[3]), _lib.ptr(nvd), _lib.ptr(ed),
                                  coef, n, _lib.cur_stream()), "fd_diff4")
    ref4 = c32 * (4 * (a[0] - a[1]) / (2 * e32) - (a[2] - a[3]) / (4 * e32)) / 3
    bound4 = EPS8 * abs(c32) * (4 * (a[0].abs() + a[1].abs()) / (2 * e32) + (a[2].abs() + a[3].abs()) / (4 * e32)) / 3
    err4 = (out4.cpu().double() - ref4).abs()
    assert bool((err4 <= bound4).all()), "diff4 n = %d: worst error / bound %.3g" % (n, float((err4 / bound4).max()))
    # e = 0: exact zeros — no NaN from the x / 0 intermediates
    zero = _words(dev, 0.0)
    for name in ("diff", "diff4"):
        o = torch.full((n,), float("nan"), device=dev)
        if name == "diff":
            _lib.check(lib.dr4sr_fd_diff(_lib.ptr(o), _lib.ptr(fd[0]), _lib.ptr(fd[1]), _lib.ptr(nvd[0:1]), _lib.ptr(nvd[1:2]), _lib.ptr(zero), coef,
                                         n, _lib.cur_stream()), "fd_diff")
        else:
            _lib.check(lib.dr4sr_fd_diff4(_lib.ptr(o), _lib.ptr(fd[0]), _lib.ptr(fd[1]), _lib.ptr(fd[2]), _lib.ptr(fd[3]), _lib.ptr(nvd),
                                          _lib.ptr(zero), coef, n, _lib.cur_stream()), "fd_diff4")
        assert torch.equal(bits(o), torch.zeros(n, dtype=torch.int32)), name
    # scale_by
    den = _words(dev, 37.0)
    os_ = torch.full((n,), float("nan"), device=dev)
    _lib.check(lib.dr4sr_scale_by(_lib.ptr(os_), _lib.ptr(fd[0]), _lib.ptr(den), n, _lib.cur_stream()), "scale_by")
    errs = (os_.cpu().double() - a[0]).abs()
    assert bool((errs <= EPS8 * a[0].abs()).all()), "scale_by n = %d" % n
    assert all(torch.equal(fd[i].cpu(), f[i]) for i in range(4))


@pytest.mark.parametrize("n", SIZES)
def test_fd_neumann(dev, n):
    """v -= lr (gp / np - gm / nm) / 2e ; pacc += v, both in place, pacc non-zero on entry"""
    from dr4sr_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(300 + n)
    v, pacc, gp, gm = (torch.randn(n, generator=g) for _ in range(4))
    gm = gp + 1e-3 * gm
    npw, nmw, e, lr = 37.0, 41.0, 2.5e-3, 0.05
    vd, pd, gpd, gmd = v.to(dev), pacc.to(dev), gp.to(dev), gm.to(dev)
    npd, nmd, ed = _words(dev, npw), _words(dev, nmw), _words(dev, e)
    e32, lr32 = float(ed.cpu()), float(torch.tensor(lr, dtype=torch.float32))
    _lib.check(lib.dr4sr_fd_neumann(_lib.ptr(vd), _lib.ptr(pd), _lib.ptr(gpd), _lib.ptr(gmd), _lib.ptr(npd), _lib.ptr(nmd), _lib.ptr(ed), lr, n,
                                    _lib.cur_stream()), "fd_neumann")
    a, b = gp.double() / npw, gm.double() / nmw
    ref_v = v.double() - lr32 * (a - b) / (2 * e32)
    bound_v = EPS8 * (v.double().abs() + lr32 * (a.abs() + b.abs()) / (2 * e32))
    err_v = (vd.cpu().double() - ref_v).abs()
    assert bool((err_v <= bound_v).all()), "v n = %d: worst error / bound %.3g" % (n, float((err_v / bound_v).max()))
    ref_p = pacc.double() + ref_v
    bound_p = bound_v + EPS8 * pacc.double().abs()
    err_p = (pd.cpu().double() - ref_p).abs()
    assert bool((err_p <= bound_p).all()), "pacc n = %d: worst error / bound %.3g" % (n, float((err_p / bound_p).max()))
    assert torch.equal(gpd.cpu(), gp) and torch.equal(gmd.cpu(), gm)
    # e = 0: v stays as it is (to the bit) and is added to pacc
    v0, p0, zero = v.to(dev), pacc.to(dev), _words(dev, 0.0)
    _lib.check(lib.dr4sr_fd_neumann(_lib.ptr(v0), _lib.ptr(p0), _lib.ptr(gpd), _lib.ptr(gmd), _lib.ptr(npd), _lib.ptr(nmd), _lib.ptr(zero), lr, n,
                                    _lib.cur_stream()), "fd_neumann")
    assert torch.equal(bits(v0), bits(v)) and torch.equal(p0.cpu(), pacc + v)
