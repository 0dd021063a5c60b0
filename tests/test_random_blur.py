"""RandomBlur (utils/augment.py, csrc/blur.hip): the fourth augmentation of the fine-tuning scripts
(post_training_utils/fine_tune_epoch.py:248-255: tio.RandomAffine(), tio.RandomBlur(), tio.RandomNoise(std=0.1), tio.RandomGamma()).

torchio is absent, so parity with it is UNPINNED, as for the other three.  What torchio 0.18.73 does is restated: per item three
standard deviations (one per axis, voxels), every channel through ``scipy.ndimage.gaussian_filter(channel, std)``.  scipy IS here,
and its rules are restated in ``blur_ref`` below (float64 is THE reference): per axis, one axis after the other (0, 1, 2),
radius = int(4 sigma + 0.5), weights exp(-k^2 / (2 sigma^2)) normalised in float64, an axis with sigma <= 1e-15 skipped, border mode
'reflect' (index i -> j = i mod 2n, then 2n - 1 - j if j >= n).  ``test_reference_equals_scipy`` holds that restatement against
scipy itself; ``test_host_tap_table`` holds the product's fp32 taps against scipy's impulse response.

Unit of error at a voxel (the convention of tests/test_loss_kernels.py): eps32 * G(|x|), eps32 = 2^-23, G(|x|) the same blur of |x|
in float64: the sum of the absolute values of what is added.  The reference of the parity test is ``blur_ref`` on the fp32 input
widened to double with the PRODUCT's fp32 taps widened to double, so the rounding of the taps is not charged to the kernel.
Bound: 3 x the worst ratio, on the same case, of the plain fp32 statement: ``blur_ref`` in numpy float32 (one rounding per product
and per sum, same taps, same order).  The bound is computed, not typed in; GPU cases print RATIO lines (run with -s) and LABNOTES.md
keeps the table.  A second check holds the kernel against scipy.ndimage.gaussian_filter itself (float64, its own weights): the
fp32 taps are the exact weights times (1 + d), |d| <= 2^-24, so each of the three passes moves a voxel by at most half a unit
more (to first order; the second-order term is 3 * 2^-48 relative): the bound there is the one above plus 1.5005 units.  That check is the
one a wrong radius rule or unnormalised weights on the host cannot pass, since the parity reference shares the host's table.

Every GPU output lives in a buffer with sentinel elements around it that no launch may touch, and starts as NaN so that a voxel
nobody wrote shows."""
import functools

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
EPS32 = 2.0 ** -23                # the spacing of fp32 at 1
FACTOR = 3.0
TAP_UNITS = 1.5005                # three passes, each tap within 2^-24 = half a unit of its float64 weight (see the docstring)
GUARD, SENT = 64, 7.25


# =========================================================================== the reference (any dtype; float64 is THE reference)
def radius_of(sigma):
    return int(4.0 * sigma + 0.5) if sigma > 1e-15 else 0


def weights64(sigma):
    r = radius_of(sigma)
    if r == 0:
        return np.ones(1)
    k = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 * k * k / (sigma * sigma))
    return w / w.sum()


def reflect_index(i, n):
    j = np.mod(i, 2 * n)
    return np.where(j >= n, 2 * n - 1 - j, j)


def corr_axis(v, w, axis):
    """out[i] = sum_k w[k] v[reflect(i + k - r)] along `axis`; the first product starts the sum, the others are added in index
    order; in the dtype of v (w is cast to it)"""
    w = np.asarray(w, dtype=v.dtype)
    r, n = len(w) // 2, v.shape[axis]
    vp = np.take(v, reflect_index(np.arange(-r, n + r), n), axis=axis)
    out = None
    for k in range(len(w)):
        sl = [slice(None)] * v.ndim
        sl[axis] = slice(k, k + n)
        t = vp[tuple(sl)] * w[k]
        out = t if out is None else out + t
    assert out.dtype == v.dtype
    return out


def blur_ref(v, ws):
    """[..., Lz, Hy, Wx] blurred with ws = (weights of axis 0, 1, 2), one axis after the other"""
    for d in range(3):
        if len(ws[d]) > 1:
            v = corr_axis(v, ws[d], v.ndim - 3 + d)
    return v


def product_table(stds):
    from vit_ae_plus_plus_amd.utils.augment import RandomBlur
    return RandomBlur.tap_table(torch.tensor(stds, dtype=torch.float64).reshape(-1, 3))


def item_weights(taps, radii, b, dtype):
    return [taps[b, d, :2 * int(radii[b, d]) + 1].numpy().astype(dtype) for d in range(3)]


# =========================================================================== CPU
SCIPY_CASES = [((5, 7, 3), (2.0, 0.05, 1.3)), ((12, 10, 9), (0.3, 1.99, 0.7)), ((2, 1, 40), (2, 2, 2)),
               ((32, 32, 32), (1.1, 0.124, 0.126)), ((3, 17, 96), (4.0, 0.9, 3.7))]


@pytest.mark.parametrize('shape,stds', SCIPY_CASES)
def test_reference_equals_scipy(shape, stds):
    from scipy import ndimage
    v = np.random.default_rng(sum(shape)).standard_normal(shape) * 3 + 1
    got = blur_ref(v, [weights64(float(s)) for s in stds])
    ref = ndimage.gaussian_filter(v, stds)
    assert got.dtype == np.float64 and np.abs(got - ref).max() <= 1e-12


def test_host_tap_table():
    from scipy import ndimage
    from vit_ae_plus_plus_amd.utils.augment import RandomBlur
    sigmas = [0.05, 0.124, 0.126, 0.7, 2.0, 4.0]
    taps, radii = RandomBlur.tap_table(torch.tensor([[s, s, s] for s in sigmas], dtype=torch.float64))
    assert taps.dtype == torch.float32 and taps.shape == (6, 3, 33) and radii.dtype == torch.int32
    assert radii[:, 0].tolist() == [0, 0, 1, 3, 8, 16] and torch.equal(radii[:, 1], radii[:, 0]) and torch.equal(radii[:, 2], radii[:, 0])
    impulse = np.zeros(33)
    impulse[16] = 1.0
    for i, s in enumerate(sigmas):
        r = int(radii[i, 0])
        resp = ndimage.gaussian_filter1d(impulse, s, mode='constant')
        for d in range(3):
            row = taps[i, d].double().numpy()
            assert np.abs(row[:2 * r + 1] - resp[16 - r:16 + r + 1]).max() <= 1e-7, (s, d)
            assert np.all(row[2 * r + 1:] == 0) and abs(row.sum() - 1) < 1e-6
            assert np.array_equal(row[:2 * r + 1], weights64(s).astype(np.float32).astype(np.float64))   # float64, rounded once
    assert taps[0, 0, 0] == 1.0 and taps[1, 2, 0] == 1.0                     # radius 0: one tap of exactly 1
    t0, r0 = RandomBlur.tap_table(torch.zeros(1, 3))                          # sigma = 0: scipy's skipped axis
    assert r0.tolist() == [[0, 0, 0]] and t0[0, :, 0].tolist() == [1.0, 1.0, 1.0]
    # a mixed item: the rows follow the axes
    _, rm = RandomBlur.tap_table(torch.tensor([[4.0, 0.05, 0.7], [0.126, 2.0, 0.124]]))
    assert rm.tolist() == [[16, 0, 3], [1, 8, 0]]


def test_constructor_and_draws():
    from vit_ae_plus_plus_amd.utils.augment import RandomBlur
    gen = lambda s: torch.Generator().manual_seed(s)
    assert RandomBlur().std == ((0.0, 2.0),) * 3
    for arg, ranges in [(1.5, [(0, 1.5)] * 3), ((0.5, 1.0), [(0.5, 1.0)] * 3), ((0, 1, 1, 2, 2, 3), [(0, 1), (1, 2), (2, 3)]),
                        ((0.7, 0.7), [(0.7, 0.7)] * 3)]:
        p = RandomBlur(std=arg, generator=gen(1)).get_params(256)
        assert p.shape == (256, 3) and p.dtype == torch.float32
        for d, (a, b) in enumerate(ranges):
            lo, hi = float(p[:, d].min()), float(p[:, d].max())
            assert a - 1e-7 <= lo and hi <= b + 1e-7, (arg, d, lo, hi)
            assert hi - lo >= 0.9 * (b - a)                                    # the whole range is drawn from
        assert not torch.equal(p[:, 0], p[:, 1]) or ranges[0][0] == ranges[0][1]   # one draw per axis, not one per item
    a, b = RandomBlur(generator=gen(7)), RandomBlur(generator=gen(7))
    pa = a.get_params(8)
    assert torch.equal(pa, b.get_params(8))
    assert torch.equal(RandomBlur(generator=gen(7)).get_params(3), pa[:3])     # item-major: three per item, item after item
    assert not torch.equal(a.get_params(8), pa)                                # the generator moves on
    for bad in (-1, (-0.5, 1), (2, 1), (0, 1, 0, 1, 3, 2), (0, 1, 2), (0, 1, 0, -1, 0, 1)):
        with pytest.raises(ValueError):
            RandomBlur(std=bad)


def test_refusals_on_the_host():
    from vit_ae_plus_plus_amd._abi import VitaeError
    from vit_ae_plus_plus_amd.utils.augment import RandomBlur
    with pytest.raises(VitaeError, match='16'):
        RandomBlur.tap_table(torch.tensor([[1.0, 4.2, 1.0]]))
    with pytest.raises(VitaeError, match='16'):
        RandomBlur().apply(torch.zeros(1, 1, 4, 4, 4), torch.tensor([[4.2, 0.0, 0.0]]))
    assert int(RandomBlur.tap_table(torch.tensor([[4.09, 4.09, 4.09]]))[1].max()) == 16
    with pytest.raises(VitaeError, match='no CPU fallback'):
        RandomBlur()(torch.zeros(1, 1, 4, 4, 4))
    with pytest.raises(VitaeError, match='no CPU fallback'):
        RandomBlur().apply(torch.zeros(1, 1, 4, 4, 4), torch.ones(1, 3))


def test_dropin_does_not_alias_torchio():
    from vit_ae_plus_plus_amd import _abi, dropin
    assert 'torchio' not in dropin._ALIASES and not any(k.startswith('torchio.') for k in dropin._ALIASES)
    assert _abi.CONSTS['VITAE_ABI_VERSION'] >= 52 and 'vitae_random_blur' in _abi.PROTOS
    assert _abi.CONSTS['VITAE_BLUR_MAX_RADIUS'] == 16 and _abi.CONSTS['VITAE_BLUR_MAX_TAPS'] == 33


# =========================================================================== GPU plumbing
class Buf:
    """A device array of `shape` inside a flat buffer with GUARD sentinel elements in front of it and behind it; NaN inside."""

    def __init__(self, shape):
        n = int(np.prod(shape))
        buf = torch.full((GUARD + n + GUARD,), SENT, dtype=torch.float32)
        buf[GUARD:GUARD + n] = float('nan')
        self.orig = buf.clone()
        self.buf, self.n = buf.cuda(), n
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        self.ptr = self.t.data_ptr()

    def intact(self):
        torch.cuda.synchronize()
        return bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[GUARD + self.n:] == SENT).all())

    def untouched(self):
        torch.cuda.synchronize()
        return torch.equal(self.buf.cpu().view(torch.int32), self.orig.view(torch.int32))


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def launch(xd, stds):
    """vitae_random_blur on the device batch xd with the product's table for `stds` -> the output, every voxel written and every
    sentinel (of the output and of the intermediate) intact"""
    from vit_ae_plus_plus_amd._abi import lib
    taps, radii = product_table(stds)
    B, C, Lz, Hy, Wx = xd.shape
    y, tmp = Buf(xd.shape), Buf(xd.shape)
    td, rd = taps.cuda(), radii.cuda()
    lib.vitae_random_blur(xd.data_ptr(), tmp.ptr, y.ptr, td.data_ptr(), rd.data_ptr(), radii.data_ptr(), B, C, Lz, Hy, Wx,
                          torch.cuda.current_stream().cuda_stream)
    assert y.intact() and tmp.intact()
    assert not bool(torch.isnan(y.t).any())
    return y.t


def volume(fam, shape, seed):
    z = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    return 3 * z + 1 if fam == 'gauss' else 1000 + z


def seam_shape():
    """Every seam of the kernels' tiling inside, and a ragged last tile on every axis: one z-tile + 3 planes, one band of rows + 5,
    one tile of columns + 7 (and a plane that is no multiple of the 64 columns a z slab)."""
    from vit_ae_plus_plus_amd._abi import const
    shape = (const('VITAE_BLUR_TILE_Z') + 3, const('VITAE_BLUR_TILE_Y') + 5, const('VITAE_BLUR_TILE_X') + 7)
    assert (shape[1] * shape[2]) % 64 != 0
    return shape


# (B, C, shape, the standard deviations of each item): the cap (4.0 -> 16), the default maximum (2.0 -> 8), an identity axis (0.05),
# either side of 0.125 (0.124 -> 0, 0.126 -> 1); item 0 and the last item differ
CASES = [
    (3, 2, (12, 10, 9), [(4.0, 2.0, 0.126), (0.124, 4.0, 2.0), (2.0, 0.05, 4.0)]),
    (2, 1, (5, 7, 3), [(2.0, 4.0, 2.0), (4.0, 0.126, 0.05)]),                      # every extent shorter than the radius
    (1, 1, (24, 16, 40), [(2.0, 0.05, 4.0)]),
    (2, 4, (32, 32, 32), [(0.124, 0.7, 0.126), (4.0, 0.05, 2.0)]),                 # 0.7: 4 sigma + 0.5 = 3.3 and 4 sigma = 2.8 differ
    (1, 2, (20, 33, 70), [(0.126, 4.0, 2.0)]),
    (2, 1, None, [(4.0, 4.0, 4.0), (2.0, 0.124, 0.05)]),                           # None: seam_shape()
]
FAMILIES = ['gauss', 'offset']


@functools.lru_cache(maxsize=None)
def case(i, fam):
    """-> the input, its float64 reference (product taps), the unit G(|x|), the plain fp32 statement's worst ratio, scipy's result"""
    from scipy import ndimage
    B, C, shape, stds = CASES[i]
    shape = shape or seam_shape()
    x = volume(fam, (B, C, *shape), 100 + 7 * i + FAMILIES.index(fam))
    taps, radii = product_table(stds)
    x64 = x.double().numpy()
    ref, unit, sci, e32 = np.empty_like(x64), np.empty_like(x64), np.empty_like(x64), 0.0
    for b in range(B):
        w64 = item_weights(taps, radii, b, np.float64)
        ref[b], unit[b] = blur_ref(x64[b], w64), EPS32 * blur_ref(np.abs(x64[b]), w64)
        f32 = blur_ref(x[b].numpy(), item_weights(taps, radii, b, np.float32))
        assert f32.dtype == np.float32
        e32 = max(e32, float((np.abs(f32.astype(np.float64) - ref[b]) / unit[b]).max()))
        for c in range(C):
            sci[b, c] = ndimage.gaussian_filter(x64[b, c], stds[b])
    assert unit.min() > 0
    for a in (ref, unit, sci):
        a.setflags(write=False)
    return x, ref, unit, e32, sci


def test_plain_fp32_statement_is_a_few_units():
    """The figure the GPU bound is 3 x of, on the CPU: between half a unit and four on every case (so the bound is a few units,
    neither zero nor loose), and the product-taps reference is within 1.5 units of scipy's own weights."""
    for i in range(len(CASES)):
        for fam in FAMILIES:
            x, ref, unit, e32, sci = case(i, fam)
            print(f'E32 case {i} {fam}: {e32:.2f} units; reference vs scipy {float((np.abs(ref - sci) / unit).max()):.2f} units')
            assert 0.5 <= e32 <= 4.0, (i, fam, e32)
            assert float((np.abs(ref - sci) / unit).max()) <= TAP_UNITS


# =========================================================================== GPU
@gpu
@pytest.mark.parametrize('fam', FAMILIES)
@pytest.mark.parametrize('i', range(len(CASES)))
def test_parity_per_voxel(i, fam):
    from vit_ae_plus_plus_amd.utils.augment import RandomBlur
    x, ref, unit, e32, sci = case(i, fam)
    stds = CASES[i][3]
    xd = x.cuda()
    y = launch(xd, stds)
    got = y.cpu().double().numpy()
    e = float((np.abs(got - ref) / unit).max())
    es = float((np.abs(got - sci) / unit).max())
    print(f'RATIO blur case {i} {tuple(x.shape)} {fam}: e={e:.2f} e32={e32:.2f} units, ratio={e / e32:.2f}; against scipy {es:.2f} units')
    assert e <= FACTOR * e32, (i, fam, e, e32)
    assert es <= FACTOR * e32 + TAP_UNITS, (i, fam, es, e32)
    # the public path allocates its own output: the same bits
    assert bits_equal(RandomBlur().apply(xd, torch.tensor(stds, dtype=torch.float64)), y)
    assert torch.equal(xd.cpu(), x)                                            # the input is left alone


@gpu
def test_exact_properties():
    shape = (20, 9, 15)                                                        # a plane of 135 columns: two full slabs of 64 and 7
    x = volume('gauss', (3, 2, *shape), 31)
    x[0, 0, 0, 0, 0], x[1, 1, 3, 2, 1] = -0.0, 0.0
    xd = x.cuda()
    # every radius 0: one copy
    ident = [(0.05, 0.1, 0.124), (0.0, 0.0, 0.0), (0.124, 0.05, 0.0)]
    assert int(product_table(ident)[1].max()) == 0
    y = launch(xd, ident)
    assert torch.equal(y, xd) and bits_equal(y, xd)
    # one identity item inside a blurred batch: its bits (a -0.0 among them) come through both kernels
    mixed = [(2.0, 0.7, 4.0), (0.05, 0.124, 0.0), (0.126, 4.0, 2.0)]
    xz = xd.clone()
    xz[1, 0, 0, 0, 0] = -0.0
    y = launch(xz, mixed)
    assert bits_equal(y[1], xz[1]) and not torch.equal(y[0], xz[0]) and not torch.equal(y[2], xz[2])
    # only the Lz pass runs (every y / x radius of the batch is 0), only the Hy / Wx pass: the identity item again
    for only in ([(2.0, 0.0, 0.0), (0.0, 0.0, 0.0), (4.0, 0.0, 0.0)], [(0.0, 2.0, 0.126), (0.0, 0.0, 0.0), (0.0, 0.0, 4.0)]):
        y1 = launch(xz, only)
        assert bits_equal(y1[1], xz[1]) and not torch.equal(y1[0], xz[0]) and not torch.equal(y1[2], xz[2])
    # two calls with one table
    assert bits_equal(launch(xz, mixed), y)
    # channels that are copies of each other
    xc = xd.clone()
    xc[:, 1] = xc[:, 0]
    yc = launch(xc, mixed)
    assert bits_equal(yc[:, 1], yc[:, 0])
    # (s, 0, 0): a (y, x) column's result does not depend on the other columns -- alone in the batch (the Lz pass only) and beside
    # an item that blurs on every axis (both passes; item 0 goes through the second as an identity)
    perm = torch.randperm(shape[1] * shape[2], generator=torch.Generator().manual_seed(5)).cuda()
    xp = xd.flatten(3)[..., perm].view(xd.shape).contiguous()
    for stds in ([(2.0, 0.0, 0.0), (4.0, 0.0, 0.0), (0.7, 0.0, 0.0)], [(2.0, 0.0, 0.0), (1.0, 1.0, 1.0), (4.0, 0.0, 0.0)]):
        ya, yb = launch(xd, stds), launch(xp, stds)
        for b in (0, 2):
            assert bits_equal(ya[b].flatten(2)[..., perm], yb[b].flatten(2))
            assert not torch.equal(ya[b], xd[b])


@gpu
def test_refusals_write_nothing():
    from vit_ae_plus_plus_amd._abi import VitaeError, lib
    B, C, shape = 2, 1, (6, 5, 4)
    xd = volume('gauss', (B, C, *shape), 41).cuda()
    taps, radii = product_table([(2.0, 1.0, 0.5), (1.0, 1.0, 1.0)])
    td, rd = taps.cuda(), radii.cuda()
    y, tmp = Buf(xd.shape), Buf(xd.shape)
    st = torch.cuda.current_stream().cuda_stream
    r17 = radii.clone()
    r17[1, 2] = 17
    neg = radii.clone()
    neg[0, 0] = -1
    ok = dict(x=xd.data_ptr(), tmp=tmp.ptr, y=y.ptr, taps=td.data_ptr(), radii=rd.data_ptr(), host=radii.data_ptr(), B=B, C=C,
              Lz=shape[0], Hy=shape[1], Wx=shape[2])
    INV, UNS = 'VITAE_ERR_INVALID_ARG', 'VITAE_ERR_UNSUPPORTED_SHAPE'
    bad = [(dict(host=r17.data_ptr(), radii=r17.cuda().data_ptr()), UNS), (dict(host=neg.data_ptr()), INV), (dict(y=xd.data_ptr()), INV),
           (dict(Lz=0), INV), (dict(Hy=0), INV), (dict(Wx=-1), INV), (dict(B=0), INV), (dict(C=0), INV), (dict(x=None), INV),
           (dict(y=None), INV), (dict(taps=None), INV), (dict(radii=None), INV), (dict(host=None), INV), (dict(tmp=None), INV),
           (dict(tmp=y.ptr), INV), (dict(tmp=xd.data_ptr()), INV), (dict(B=65536), UNS), (dict(C=65536), UNS)]
    before = xd.clone()
    for kw, code in bad:
        a = dict(ok, **kw)
        with pytest.raises(VitaeError, match=code):
            lib.vitae_random_blur(a['x'], a['tmp'], a['y'], a['taps'], a['radii'], a['host'], a['B'], a['C'], a['Lz'], a['Hy'], a['Wx'], st)
        assert y.untouched() and tmp.untouched() and torch.equal(xd, before), kw
    # the same arguments unchanged are served (tmp may be absent when one of the two passes is not needed)
    lib.vitae_random_blur(*[ok[k] for k in ('x', 'tmp', 'y', 'taps', 'radii', 'host', 'B', 'C', 'Lz', 'Hy', 'Wx')], st)
    assert y.intact() and tmp.intact() and not bool(torch.isnan(y.t).any())
    tz, rz = product_table([(2.0, 0.0, 0.0), (0.0, 0.0, 0.0)])
    tzd, rzd = tz.cuda(), rz.cuda()
    y2 = Buf(xd.shape)
    lib.vitae_random_blur(ok['x'], None, y2.ptr, tzd.data_ptr(), rzd.data_ptr(), rz.data_ptr(), B, C, *shape, st)
    assert y2.intact() and bits_equal(y2.t[1], xd[1]) and not bool(torch.isnan(y2.t).any())


@gpu
def test_compose_equals_one_by_one():
    from vit_ae_plus_plus_amd.utils.augment import Compose, RandomAffine, RandomBlur, RandomGamma, RandomNoise
    gen = lambda s: torch.Generator().manual_seed(s)
    x = volume('gauss', (3, 2, 12, 10, 9), 51)
    xd = x.cuda()
    noise = torch.randn(x.shape, generator=gen(52)).cuda()
    make = lambda: (RandomAffine(generator=gen(53)), RandomBlur(generator=gen(54)), RandomNoise(std=0.1, generator=gen(55)),
                    RandomGamma(log_gamma=(-0.3, 0.3), generator=gen(56)))
    ra, rb, rn, rg = make()
    one = rg(rn(rb(ra(xd)), noise=noise))
    ra2, rb2, rn2, rg2 = make()
    rn2.draw = lambda t: noise
    chain = Compose([ra2, rb2, rn2, rg2])(xd)
    assert torch.equal(chain, one) and bits_equal(chain, one)
    assert rb.last_params['std'].shape == (3, 3) and torch.equal(rb.last_params['std'], rb2.last_params['std'])
    assert torch.equal(rb.last_params['std'], RandomBlur(generator=gen(54)).get_params(3))
    assert 0 <= float(rb.last_params['std'].min()) and float(rb.last_params['std'].max()) <= 2
    assert not torch.equal(rb(xd), xd)


@gpu
def test_views_of_a_bench_size_batch_with_four_transforms():
    """2 x 4 x 96^3 through augmented_views with the fine-tuning chain: both views come out normalised; at sigma 2 on every axis the
    variance of white noise falls by more than half (the taps of one axis alone have sum of squares 0.14)."""
    from vit_ae_plus_plus_amd.utils.augment import Compose, RandomAffine, RandomBlur, RandomGamma, RandomNoise, augmented_views
    gen = lambda s: torch.Generator().manual_seed(s)
    g = torch.Generator(device='cuda').manual_seed(61)
    ax = torch.arange(96, device='cuda', dtype=torch.float32)
    smooth = torch.sin(ax / 7)[:, None, None] + torch.cos(ax / 9)[None, :, None] * torch.sin(ax / 5)[None, None, :]
    raw = 100 + 40 * smooth[None, None] * torch.tensor([1.0, 0.7, 1.3, 0.9], device='cuda').view(1, 4, 1, 1, 1) \
        + torch.randn(2, 4, 96, 96, 96, device='cuda', generator=g)
    rb = RandomBlur(generator=gen(63))
    tf = Compose([RandomAffine(generator=gen(62)), rb, RandomNoise(std=0.1, generator=gen(64)),
                  RandomGamma(log_gamma=(-0.3, 0.3), generator=gen(65))])
    v1, v2 = augmented_views(raw, tf, use_z_score=True)
    for v in (v1, v2):
        assert abs(float(v.double().mean(dim=(1, 2, 3, 4)).abs().max())) < 1e-4
        assert abs(float(v.double().var(dim=(1, 2, 3, 4)).max()) - 1) < 1e-4
    assert rb.last_params['std'].shape == (2, 3)
    assert float((v1 - v2).abs().mean()) > 1e-2 and float((v1 * v2).double().mean()) > 0.5
    white = torch.randn(2, 4, 96, 96, 96, device='cuda', generator=g)
    fixed = RandomBlur(std=(2, 2))
    out = fixed(white)
    assert torch.equal(fixed.last_params['std'], torch.full((2, 3), 2.0))
    v_in, v_out = white.double().var(dim=(1, 2, 3, 4)), out.double().var(dim=(1, 2, 3, 4))
    assert bool((v_out < 0.5 * v_in).all()), (v_in, v_out)
    assert float(v_out.max()) < 0.01 * float(v_in.min())          # 0.14^3 = 0.003 in the interior
