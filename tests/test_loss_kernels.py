"""The loss chain — csrc/loss.hip and csrc/loss_fused.hip — against float64, voxel by voxel (row by row for the cosine term).

References (validated on the CPU, no GPU needed).  Every operation is written out from the formulas of include/vitae_hip.h on top of
ONE primitive, ``corr1d`` (zero-padded cross-correlation along one axis, taps added in index order), and evaluated in float64 on the
fp32 inputs the kernels get: ``patchify_ref`` / ``unpatchify_ref`` (e = ((r p + s) p + q) C + c), ``recon_ref`` (masked MSE),
``blur_ref`` (x, then y, then z), ``sobel_ref`` (g0 = s(z) s(y) d(x), g1 = s(z) e(y) s(x), g2 = e(z) s(y) s(x); s = [1 2 1],
d = [1 0 -1], e = [-1 0 1]), ``edge_ref`` (E = sum_c m_c, m_c = |g_c|), the edge MSE, dpred through float64 autograd of
g_recon recon + g_edge edge_mse, and ``cos_ref`` (each norm clamped at 1e-8).  They equal oracle/mae_ref.py evaluated in float64 to
1e-12 — except the cosine GRADIENT of a row below the clamp: torch clamps the norm in place outside autograd and differentiates
as if it were |p|, 2.8e-3 away from the derivative of the formula the header states; the formula is the reference there.

Unit of error: per voxel, the first-order rounding scale of the operation = the sum of the absolute values of what is added,
computed from the float64 reference alone (``*_abs`` = the same correlations with |weights| on |values|):
  blur            S    = |k| * |k| * |k| * |vol|
  Sobel           A_ca = |w_a| * |vol_c|;   edge map  S_E = sum_c K_c,  K_c = sqrt(sum_a A_ca^2)
  target's edge   the same S_E formed on S (the blur's own scale) instead of |blurred|: both roundings, S >= |blurred| pointwise
  dpred           |recon term| + sum_a |w_a|^T * T_ca,   T_ca = coef (|Ep - Et| (|g_a| / m_c + K_c / m_c) + S_E |g_a| / m_c),
                  coef = 2 |g_edge| / (B V); the K_c / m_c term is the error of the DIRECTION g / m of a nearly cancelled Sobel vector
  cosine dp       per row, |coef| (|z|_inf / (np nz) + |c| |p|_inf / np^2), np, nz the clamped norms
  scalar sums     their own relative error (the sums of squares have no cancellation); the cosine scalar against
                  w sum_i |c_i| / (2 R), because the mean of cosines of random rows cancels
0 / 0 counts as 0 and x / 0 as inf: where the scale is zero (an unmasked patch with g_edge = 0) the kernel owes an exact zero.

Bound (the rule of tests/test_norm_kernels.py): e <= max(3 e32, 4 2^-24).  e32 is the same figure, on the same inputs, of the plain
fp32 statement of the operation on the CPU — the larger of torch's own ops (F.conv3d with the dense kernels, F.mse_loss, autograd,
F.cosine_similarity: ``torch32_*``) and the reference formula evaluated in fp32.  (Below the cosine clamp only the formula counts,
see above.)  bf16 copies are bitwise ``fp32 output .to(bfloat16)``; a launch that writes the bf16 copy alone writes the bits of
the launch that writes both.

Input families (``volumes``; CPU-tested for what they claim): gauss — N(0, 1) images, N(0, 0.5) prediction; offset — mean 50,
deviation 1 (the Sobel differences cancel: |g| / A < 0.05 in the interior); brain — images exactly 0 outside an ellipsoid, the
prediction there a non-zero noise below 1e-3 (so no |g| is exactly 0), 0.8 image + N(0, 0.1) inside; outlier — gauss with one 1e4 in
the prediction on the seam voxel of the shape's plan (one-pass: behind the first x-tile, y-segment and 6-plane z-tile; test_two_kernel_path: x = 32, y = 8, z = 8
of the 8 x 8 x 32 tiling, the middle of an axis that has no seam).  Every finite family has all m_c > 0 in float64 AND in fp32.  Masks: all ones,
one kept patch, a checkerboard over the patch grid.

Which test reaches which launch path (from the launchers):
  loss_fwd_bwd_kernel<true> / <false>   test_one_pass_loss (six shapes, ``one_pass_plan`` restates the launcher's tiling: all boundary
                        and Hy < 8; one full 60-column tile with two exact z-tiles; two x-tiles with a ragged z-tile; x-tiles
                        42 / 42 / 40 with Lz < 6; 64 pieces, tys = 12, segments 12 / 12 / 12 / 4; 256 pieces, one segment), both
                        piece maps (VITAE_LOSS_XCD = 0 / 1), test_non_finite_prediction (the bad voxel's patch masked, and unmasked: the edge term alone carries it)
  loss_fwd_fused_kernel, loss_bwd_fused_kernel<4, true>    test_one_pass_loss (the two-kernel path on the same cases)
  loss_bwd_fused_kernel<1, false> / <1, true> / <4, false>  test_two_kernel_path[(9,9,33) p=3 C=1 / (8,8,36) p=4 C=1 / (9,16,33) p=1 C=4]
  recon_fwd + unpatchify + sobel_mag_tiled, recon_bwd + sobel_bwd_components + sobel_bwd_scatter    test_two_kernel_path[C=2] and
                        [C=4, pred and dpred 4 bytes off 16: the unaligned fall-back, forward and backward]
  target_edge_kernel    test_target_edge (XO_T = 52: one column, one tile, 53 = 27 + 26, 105 = 35 x 3, 52 exactly; tys >= 16: Hy 17 / 33)
  blur_xy_kernel + blur_z_kernel    test_gauss_blur_11_taps (band of 22 rows: Hy 22 / 23 / 45; z chunk 32: Lz 32 / 33; Wx 5 / 33 / 252 /
                        384 — the last two ask for more than 64 KB of dynamic LDS), symmetric and asymmetric taps
  blur_axis_kernel      test_gauss_blur_generic_path (sigma 1 -> 5 taps, sigma 3 -> 15, VITAE_MAX_TAPS = 33, Wx = 388 with 11 taps)
  cosine_fwd_vec_kernel<1..4> / cosine_fwd_kernel + finalize, cosine_bwd_kernel   test_cosine (D 256 .. 1024 / 320, 7 and operands
                        4 bytes off; R = 1030 > the 1024 workgroups x ... one pass covers)
  every launcher's refusals    test_refusals_* (nothing is launched: the outputs keep their bits)

Every output lives in a buffer with sentinel elements around it (and in the cls row of dpred) that no launch may touch; outputs
start as NaN so an element nobody wrote shows.  GPU cases print ``RATIO`` lines (run with -s); LABNOTES.md keeps the table."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import mae_ref as R

GUARD, SENT = 64, 7.25           # SENT is exact in bf16
FACTOR, FLOOR = 3.0, 4.0 * 2.0 ** -24
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
NS = types.SimpleNamespace
S3, D3, E3 = (1.0, 2.0, 1.0), (1.0, 0.0, -1.0), (-1.0, 0.0, 1.0)
FAMILIES = ['gauss', 'offset', 'brain', 'outlier']
MASKS = ['ones', 'one', 'checker']
COS_EPS = 1e-8
cdiv = lambda a, b: (a + b - 1) // b


# =========================================================================== references (any dtype; float64 is THE reference)
def corr1d(v, w, dim):
    """zero-padded cross-correlation along `dim`: out[i] = sum_j w[j] v[i + j - len(w) // 2], the taps added in index order"""
    dim = dim % v.dim()
    n, rad = v.shape[dim], len(w) // 2
    vp = F.pad(v, [0, 0] * (v.dim() - 1 - dim) + [rad, rad])
    out = None
    for j, wj in enumerate(w):
        if wj == 0:
            continue
        t = vp.narrow(dim, j, n) * float(wj)
        out = t if out is None else out + t
    return out


def patchify_ref(vol, p):
    """[B, C, Lz, Hy, Wx] -> [B, L, p^3 C]: patch l = (gl g1 + gh) g2 + gw, element e = ((r p + s) p + q) C + c"""
    B, C, Lz, Hy, Wx = vol.shape
    x = vol.reshape(B, C, Lz // p, p, Hy // p, p, Wx // p, p)           # b c gl r gh s gw q
    return x.permute(0, 2, 4, 6, 3, 5, 7, 1).reshape(B, (Lz // p) * (Hy // p) * (Wx // p), p * p * p * C)


def unpatchify_ref(x, p, vol, C):
    Lz, Hy, Wx = vol
    x = x.reshape(x.shape[0], Lz // p, Hy // p, Wx // p, p, p, p, C)    # b gl gh gw r s q c
    return x.permute(0, 7, 1, 4, 2, 5, 3, 6).reshape(x.shape[0], C, Lz, Hy, Wx)


def recon_ref(pred, target, mask):
    """-> (the masked MSE, its numerator sum_masked mean_e (pred - target)^2 = what acc[VITAE_ACC_RECON] holds)"""
    s = (((pred - target) ** 2).mean(-1) * mask).sum()
    return s / mask.sum(), s


def blur_ref(vol, k):
    k = [float(t) for t in k]
    return corr1d(corr1d(corr1d(vol, k, -1), k, -2), k, -3)


def blur_abs(vol, k):
    return blur_ref(vol.abs(), [abs(float(t)) for t in k])


def _sobel(v, sz, sy, sx):
    return corr1d(corr1d(corr1d(v, sz, -3), sy, -2), sx, -1)


def sobel_ref(v):
    """[..., Lz, Hy, Wx] -> [..., 3, Lz, Hy, Wx]"""
    return torch.stack([_sobel(v, S3, S3, D3), _sobel(v, S3, E3, S3), _sobel(v, E3, S3, S3)], -4)


def sobel_abs(v):
    """A_a = |w_a| * |v|  (|d| = |e| = [1 0 1]); also the transposed correlation with |w_a|, which is symmetric"""
    v, n = v.abs(), (1.0, 0.0, 1.0)
    return torch.stack([_sobel(v, S3, S3, n), _sobel(v, S3, n, S3), _sobel(v, n, S3, S3)], -4)


def edge_ref(vol):
    """[B, C, Lz, Hy, Wx] -> E [B, Lz, Hy, Wx], g [B, C, 3, ...], m [B, C, ...]"""
    g = sobel_ref(vol)
    m = torch.sqrt((g * g).sum(2))
    return m.sum(1), g, m


def edge_scale(absvol):
    """S_E and K_c of a volume of magnitudes"""
    A = sobel_abs(absvol)
    K = torch.sqrt((A * A).sum(2))
    return K.sum(1), K


def cos_ref(p, z):
    return (p * z).sum(1) / (p.norm(dim=1).clamp_min(COS_EPS) * z.norm(dim=1).clamp_min(COS_EPS))


def contr_ref(p1, z2, p2, z1, w):
    return w * (-(cos_ref(p1, z2).mean() + cos_ref(p2, z1).mean()) * 0.5)


# =========================================================================== torch's own fp32 ops (the other half of e32)
def torch32_blur(vol, k):
    """the dense k (x) k (x) k conv3d of the reference's gaussian_filter.py with the taps the kernel is given"""
    k = torch.as_tensor(np.asarray(k), dtype=vol.dtype)
    k3 = torch.einsum('i,j,k->ijk', k, k, k)
    lead = vol.shape[:-3]
    return F.conv3d(vol.reshape(-1, 1, *vol.shape[-3:]), k3[None, None], padding=len(k) // 2).reshape(*lead, *vol.shape[-3:])


def torch32_loss(pred, imgs, mask, Et, p, vol):
    """model/vit_autoenc.py:221-227 with torch's ops (oracle/mae_ref.py's building blocks), Et given -> recon, edge mse, Ep"""
    grid = tuple(n // p for n in vol)
    recon = (((pred - R.patchify(imgs, p)) ** 2).mean(dim=-1) * mask).sum() / mask.sum()
    Ep = R.sobel_magnitude(R.unpatchify(pred, p, grid))
    return recon, F.mse_loss(Ep, Et, reduction='mean'), Ep


# =========================================================================== metrics
def _ratio(num, den):
    """num / den with 0 / 0 = 0 and x / 0 = inf"""
    inf, zero = torch.full_like(num, float('inf')), torch.zeros_like(num)
    return torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num == 0, zero, inf))


def _cpu64(a):
    return a.detach().double().cpu()


def vox_err(a, ref, scale, where=None):
    """worst element of |a - ref| / scale -> (the figure, its flat index)"""
    r = _ratio((_cpu64(a) - _cpu64(ref)).abs(), _cpu64(scale))
    if where is not None:
        r = torch.where(where, r, torch.zeros_like(r))
    r = r.reshape(-1)
    i = int(torch.argmax(torch.nan_to_num(r, nan=float('inf'))))
    return float(r[i]), i


def rel_err64(a, ref):
    a, ref = float(a), float(ref)
    return 0.0 if a == ref else abs(a - ref) / abs(ref) if ref != 0 else float('inf')


def within(label, e, *e32s):
    """The bound of this file; prints the RATIO line."""
    e, e32 = (e[0] if isinstance(e, tuple) else e), max(x[0] if isinstance(x, tuple) else x for x in e32s)
    r = e / e32 if e32 > 0 else (0.0 if e == 0 else float('inf'))
    print(f'RATIO {label}: e={e:.3e} e32={e32:.3e} ratio={r:.2f}')
    assert e <= max(FACTOR * e32, FLOOR), (label, e, e32)
    return r


# =========================================================================== the launcher's plans, restated
def one_pass_plan(vol, B, target=256):
    """vitae_loss_fwd_bwd: NW = 8 waves = 6 output planes a z-tile, 60 output columns a row -> NS(xtiles, xo, zt, nseg, tys, pieces)"""
    Lz, Hy, Wx = vol
    xtiles = cdiv(Wx, 60)
    xo, zt = cdiv(Wx, xtiles), cdiv(Lz, 6)
    nseg = max(cdiv(target, xtiles * zt * B), 1)
    tys = min(max(cdiv(cdiv(Hy, nseg), 4) * 4, 8), Hy)
    return NS(xtiles=xtiles, xo=xo, zt=zt, nseg=cdiv(Hy, tys), tys=tys, pieces=xtiles * zt * B)


def target_plan(vol, B, target=256):
    """vitae_target_edge: 52 output columns a row, rows per segment >= 16"""
    Lz, Hy, Wx = vol
    xtiles = cdiv(Wx, 52)
    xo, zt = cdiv(Wx, xtiles), cdiv(Lz, 6)
    nseg = max(cdiv(target, xtiles * zt * B), 1)
    tys = min(max(cdiv(cdiv(Hy, nseg), 4) * 4, 16), Hy)
    return NS(xtiles=xtiles, xo=xo, zt=zt, nseg=cdiv(Hy, tys), tys=tys)


def seam_voxel(vol, B):
    """(z, y, x): the first voxel behind the first x-, y- and z-seam of the one-pass plan (the middle where an axis has no seam)"""
    pl = one_pass_plan(vol, B)
    Lz, Hy, Wx = vol
    return (6 if Lz > 6 else Lz // 2, pl.tys if pl.nseg > 1 else Hy // 2, pl.xo if pl.xtiles > 1 else Wx // 2)


def tiling_seam_voxel(vol):
    """(z, y, x): the first voxel behind the first z-, y- and x-seam of the 8 x 8 x 32 tiling (the middle where an axis has no seam)"""
    return tuple(t if n > t else n // 2 for n, t in zip(vol, (8, 8, 32)))


ONE_PASS_SHAPES = [((2, 2, 2), 2, 1), ((12, 24, 60), 4, 1), ((8, 16, 64), 8, 1), ((4, 8, 124), 4, 3), ((48, 40, 8), 8, 8), ((96, 8, 8), 8, 16)]


# =========================================================================== inputs
def gaussian_taps_host(sigma):
    from vit_ae_plus_plus_amd.engine import gaussian_taps_host as f
    return f(sigma)


def asym_taps(n, seed=5):
    """n positive taps, normalised, NOT symmetric (a reversed tap index shows)"""
    t = torch.rand(n, generator=torch.Generator().manual_seed(seed), dtype=F64) + 0.1 + torch.arange(n, dtype=F64) * 0.3 / n
    return (t / t.sum()).float().numpy()


def volumes(fam, B, C, vol, seed, at=None):
    """-> images [B, C, *vol], the prediction as a volume [B, C, *vol] (fp32); `at`: the outlier's voxel (default: the one-pass seam)"""
    g = torch.Generator().manual_seed(seed)
    shape = (B, C, *vol)
    z1, z2 = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    if fam in ('gauss', 'outlier'):
        imgs, pv = z1, 0.5 * z2
        if fam == 'outlier':
            pv = pv.clone()
            pv[B // 2, C // 2][at or seam_voxel(vol, B)] = 1e4
    elif fam == 'offset':
        imgs, pv = 50.0 + z1, 50.0 + z2
    elif fam == 'brain':
        inside = brain_inside(vol)
        noise = (torch.rand(shape, generator=g) * 0.8 + 0.1) * 1e-3 * (1 - 2 * torch.randint(0, 2, shape, generator=g)).float()
        imgs = torch.where(inside, 1.0 + z1.abs(), torch.zeros(()))
        pv = torch.where(inside, 0.8 * imgs + 0.1 * z2, noise)
    else:
        raise ValueError(fam)
    return imgs.float().contiguous(), pv.float().contiguous()


def brain_inside(vol):
    ax = [(torch.arange(n, dtype=F64) - (n - 1) / 2) / (0.4 * n + 0.5) for n in vol]
    return (ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2) <= 1.0


def make_mask(pat, B, vol, p):
    gl, gh, gw = (n // p for n in vol)
    L = gl * gh * gw
    if pat == 'ones':
        m = torch.ones(B, L)
    elif pat == 'one':
        m = torch.zeros(B, L)
        m[0, L // 2] = 1.0
    elif pat == 'checker':
        i = torch.arange(L)
        m = ((((i // (gh * gw)) + (i // gw) % gh + i % gw) % 2) == 0).float().expand(B, L).contiguous()
    else:
        raise ValueError(pat)
    return m


_CACHE = {}


@pytest.fixture(scope='module', autouse=True)
def _drop_case_cache():
    yield
    _CACHE.clear()


def loss_case(fam, vol, p, B, C=4, maskpat='ones', tiling=False):
    """Inputs and float64 references of one case, computed once and shared (read-only): the two gradient fields (of recon and of
    the edge MSE: dpred is linear in g_recon, g_edge), the rounding scales, the scalars.  `tiling`: the outlier sits on the seam
    voxel of the 8 x 8 x 32 tiling instead of the one-pass plan's."""
    key = (fam, vol, p, B, C, maskpat, tiling)
    if key in _CACHE:
        return _CACHE[key]
    seed = 100 + 7 * sum(vol) + 13 * p + B + 31 * FAMILIES.index(fam)
    imgs, pv = volumes(fam, B, C, vol, seed, tiling_seam_voxel(vol) if tiling else None)
    pred, mask = patchify_ref(pv, p).contiguous(), make_mask(maskpat, B, vol, p)
    taps = gaussian_taps_host(2.0)
    Et = edge_ref(blur_ref(imgs.double(), taps))[0].float()              # the target's edge map, an fp32 INPUT of every loss kernel
    V, L, P = vol[0] * vol[1] * vol[2], pred.shape[1], pred.shape[2]
    c = NS(fam=fam, vol=vol, p=p, B=B, C=C, V=V, L=L, P=P, imgs=imgs, pred=pred, mask=mask, Et=Et, msum=float(mask.sum()), taps=taps)
    pr = pred.double().requires_grad_(True)
    recon, rsum = recon_ref(pr, patchify_ref(imgs.double(), p), mask.double())
    Ep, g, m = edge_ref(unpatchify_ref(pr, p, vol, C))
    edge = ((Ep - Et.double()) ** 2).mean()
    c.d_recon, = torch.autograd.grad(recon, pr, retain_graph=True)
    c.d_edge, = torch.autograd.grad(edge, pr)
    c.recon, c.rsum, c.edge, c.esum = (float(t.detach()) for t in (recon, rsum, edge, ((Ep - Et.double()) ** 2).sum()))
    c.Ep, c.m = Ep.detach(), m.detach()
    with torch.no_grad():
        pv64 = pv.double()
        c.S_E, K = edge_scale(pv64)
        ga = g.detach().abs() / c.m[:, :, None]
        dE = (c.Ep - Et.double()).abs()[:, None, None]
        T = dE * (ga + (K / c.m)[:, :, None]) + c.S_E[:, None, None] * ga               # x coef below
        n = (1.0, 0.0, 1.0)
        back = _sobel(T[:, :, 0], S3, S3, n) + _sobel(T[:, :, 1], S3, n, S3) + _sobel(T[:, :, 2], n, S3, S3)
        c.edge_unit = patchify_ref(back, p) * (2.0 / (B * V))
        c.recon_unit = c.d_recon.abs()
    c.stmt = {}
    _CACHE[key] = c
    return c


def statements32(c, g_r, g_e):
    """dpred, Ep and the scalars of the two fp32 statements for one pair of upstream gradients (cached on the case)"""
    if (g_r, g_e) in c.stmt:
        return c.stmt[(g_r, g_e)]
    out = []
    for name in ('torch', 'formula'):
        pr = c.pred.clone().requires_grad_(True)
        if name == 'torch':
            recon, edge, Ep = torch32_loss(pr, c.imgs, c.mask, c.Et, c.p, c.vol)
            rsum = recon * c.msum
        else:
            recon, rsum = recon_ref(pr, patchify_ref(c.imgs, c.p), c.mask)
            Ep = edge_ref(unpatchify_ref(pr, c.p, c.vol, c.C))[0]
            edge = ((Ep - c.Et) ** 2).mean()
        (recon * g_r + edge * g_e).backward()
        out.append(NS(name=name, dpred=pr.grad, Ep=Ep.detach(), recon=float(recon.detach()), edge=float(edge.detach()), rsum=float(rsum.detach())))
    c.stmt[(g_r, g_e)] = out
    return out


def dpred_ref(c, g_r, g_e):
    """-> (float64 dpred, its rounding scale)"""
    return g_r * c.d_recon + g_e * c.d_edge, abs(g_r) * c.recon_unit + abs(g_e) * c.edge_unit


# =========================================================================== CPU tests: references, inputs, plans, e32
def test_references_are_the_oracle_in_float64():
    """corr1d-built float64 references == oracle/mae_ref.py (conv3d-built) evaluated in float64, forward and gradient: 1e-12."""
    close = lambda a, b, tol=1e-12: float((a - b).detach().abs().max()) <= tol * max(float(b.detach().abs().max()), 1e-300)
    for vol, p, B, C in (((4, 6, 8), 2, 2, 4), ((3, 3, 3), 1, 1, 1), ((6, 6, 12), 3, 1, 2)):
        g = torch.Generator().manual_seed(vol[2])
        imgs, pv = torch.randn(B, C, *vol, generator=g, dtype=F64), torch.randn(B, C, *vol, generator=g, dtype=F64)
        grid = tuple(n // p for n in vol)
        cfg = R.RefConfig(volume_size=vol, patch_size=p, in_chans=C, embed_dim=48, depth=1, num_heads=3, decoder_embed_dim=32,
                          decoder_depth=1, decoder_num_heads=2)
        L = grid[0] * grid[1] * grid[2]
        mask = (torch.rand(B, L, generator=g) < 0.6).double()
        mask[:, 0] = 1
        assert torch.equal(patchify_ref(pv, p), R.patchify(pv, p)) and torch.equal(unpatchify_ref(R.patchify(pv, p), p, vol, C), pv)
        # the index formula itself: element e of patch l
        pt = patchify_ref(pv, p)
        for (b, c_, z, y, x) in ((0, 0, 0, 0, 0), (B - 1, C - 1, vol[0] - 1, vol[1] - 1, vol[2] - 1), (0, C // 2, vol[0] // 2, 1, vol[2] - 2)):
            l = ((z // p) * grid[1] + y // p) * grid[2] + x // p
            e = (((z % p) * p + y % p) * p + x % p) * C + c_
            assert float(pt[b, l, e]) == float(pv[b, c_, z, y, x])
        # blur: the oracle takes its taps from a float32 linspace and renormalises the dense kernel; the same taps, normalised
        k = R.gaussian_taps(2).double()
        assert close(blur_ref(imgs, k / k.sum()), R.gaussian_blur3d(imgs, 2), 1e-12)
        assert close(torch32_blur(imgs, (k / k.sum()).numpy()), R.gaussian_blur3d(imgs, 2), 1e-12)
        assert close(edge_ref(pv)[0], R.sobel_magnitude(pv))
        pr1, pr2 = (patchify_ref(pv, p).clone().requires_grad_(True) for _ in range(2))
        want = R.loss_terms(imgs, pr1, mask, cfg, 0.37)
        want[0].backward()
        Et = R.sobel_magnitude(R.gaussian_blur3d(imgs, 2))
        recon, _ = recon_ref(pr2, patchify_ref(imgs, p), mask)
        Ep = edge_ref(unpatchify_ref(pr2, p, vol, C))[0]
        edge = ((Ep - Et) ** 2).mean()
        (recon + 0.37 * edge).backward()
        assert close(recon, want[2]) and close(edge, want[1]) and close(pr2.grad, pr1.grad)
        t_recon, t_edge, t_Ep = torch32_loss(pr2.detach(), imgs, mask, Et, p, vol)
        assert close(t_recon, want[2]) and close(t_edge, want[1]) and close(t_Ep, Ep)
    # cosine: values everywhere; gradients of rows at and above the clamp
    p1, z2, p2, z1 = cos_rows(9, 40, 1, F64)
    a, b = (p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)), (p1.clone().requires_grad_(True), p2.clone().requires_grad_(True))
    want, got = R.contrastive_loss(a[0], a[1], z1, z2, 0.3), contr_ref(b[0], z2, b[1], z1, 0.3)
    want.backward(); got.backward()
    assert abs(float(want.detach()) - float(got.detach())) <= 1e-12 * abs(float(want.detach()))
    keep = torch.ones(9, dtype=torch.bool)
    keep[4] = False
    for x, y in zip(a, b):
        assert close(y.grad[keep], x.grad[keep])
    # ... and below it torch differentiates another function (the clamp happens in place, outside autograd): not the reference
    assert 1e-4 < float((a[0].grad[4] - b[0].grad[4]).abs().max() / b[0].grad[4].abs().max()) < 1e-1
    # the formula's derivative there has no p term at all
    coef = 0.3 * -0.5 / 9
    assert close(b[0].grad[4], coef * z2[4] / (COS_EPS * z2[4].norm()))


def test_sobel_known_answer():
    """x = arange(27) as a 3^3 volume: centre components (-32, 96, 288), |g| = 305.26056."""
    x = torch.arange(27, dtype=F64).reshape(1, 1, 3, 3, 3)
    E, g, m = edge_ref(x)
    assert [float(t) for t in g[0, 0, :, 1, 1, 1]] == [-32.0, 96.0, 288.0]
    assert float(E[0, 1, 1, 1]) == 93184.0 ** 0.5 and f'{float(np.float32(float(E[0, 1, 1, 1]))):.5f}' == '305.26056'      # (the survey's figure is the fp32 one)


def test_corr1d_is_a_zero_padded_cross_correlation():
    v = torch.tensor([1.0, 10.0, 100.0, 1000.0], dtype=F64)
    assert corr1d(v, (1.0, 2.0, 4.0), 0).tolist() == [2 + 40, 1 + 20 + 400, 10 + 200 + 4000, 100 + 2000]
    assert corr1d(v, D3, 0).tolist() == [-10.0, 1 - 100.0, 10 - 1000.0, 100.0]


@pytest.mark.parametrize('fam', FAMILIES)
def test_input_families_have_the_claimed_properties(fam):
    shapes = [(vol, p, B, 4, False) for vol, p, B in ONE_PASS_SHAPES] + [(vol, p, 2, C, True) for _, vol, p, C, _ in TWO_KERNEL_CASES[:4]]
    for vol, p, B, C, tiling in shapes:
        c = loss_case(fam, vol, p, B, C, tiling=tiling)
        pv = unpatchify_ref(c.pred, p, vol, C).double()
        assert float(c.m.min()) > 0                                       # no 0 / 0 in float64 ...
        for s in statements32(c, 0.5, 0.185):
            assert bool(torch.isfinite(s.dpred).all()), s.name            # ... nor in either fp32 statement
        m32 = edge_ref(pv.float())[1:]
        assert float(m32[1].min()) > 0
        tol = lambda t: max(t, 4.0 / pv.numel() ** 0.5)                   # (four deviations of a mean of n unit samples, for the small shapes)
        if fam == 'gauss':
            assert abs(float(c.imgs.mean())) < tol(0.05) and abs(float(pv.std()) - 0.5) < tol(0.05)
        elif fam == 'offset':
            assert abs(float(pv.mean()) - 50) < tol(0.1) and abs(float(pv.std()) - 1) < tol(0.1)
            if min(vol) >= 3:
                inner = (slice(None), slice(None), slice(1, -1), slice(1, -1), slice(1, -1))
                assert float((c.m / edge_scale(pv)[1])[inner].max()) < 0.05      # the differences cancel
        elif fam == 'brain':
            out = ~brain_inside(vol)
            assert 0.2 < float(out.double().mean()) < 0.8 or vol == (2, 2, 2)      # (eight voxels: all inside)
            assert bool((c.imgs[:, :, out] == 0).all()) and bool((c.imgs[:, :, ~out] >= 1).all())
            assert not bool(out.any()) or 0 < float(pv[:, :, out].abs().min()) and float(pv[:, :, out].abs().max()) < 1e-3
        elif fam == 'outlier':
            z, y, x = tiling_seam_voxel(vol) if tiling else seam_voxel(vol, B)
            assert int((pv == 1e4).sum()) == 1 and float(pv[B // 2, C // 2, z, y, x]) == 1e4 and float(pv.abs().max()) == 1e4
    for pat in MASKS:
        m = make_mask(pat, 2, (8, 16, 64), 8)
        assert set(m.unique().tolist()) <= {0.0, 1.0} and float(m.sum()) == {'ones': 32, 'one': 1, 'checker': 16}[pat]
    m = make_mask('checker', 1, (8, 8, 16), 4).reshape(2, 2, 4)
    assert bool((m[:, :, :-1] != m[:, :, 1:]).all()) and bool((m[:, :-1] != m[:, 1:]).all()) and bool((m[:-1] != m[1:]).all())


def test_plans_of_the_tested_shapes():
    """The shapes reach what the module docstring says (the launchers' formulas, restated)."""
    pl = [one_pass_plan(v, B) for v, p, B in ONE_PASS_SHAPES]
    assert (pl[0].xtiles, pl[0].zt, pl[0].nseg, pl[0].tys) == (1, 1, 1, 2)                    # all boundary, Hy < 8
    assert (pl[1].xtiles, pl[1].xo, pl[1].zt, pl[1].nseg, pl[1].tys) == (1, 60, 2, 3, 8) and 12 % 6 == 0
    assert (pl[2].xtiles, pl[2].xo, pl[2].zt, pl[2].nseg, pl[2].tys) == (2, 32, 2, 2, 8) and 8 % 6 == 2
    assert (pl[3].xtiles, pl[3].xo, pl[3].zt, pl[3].nseg) == (3, 42, 1, 1) and 124 - 2 * 42 == 40
    assert (pl[4].pieces, pl[4].tys, pl[4].nseg) == (64, 12, 4) and 40 - 3 * 12 == 4
    assert (pl[5].pieces, pl[5].tys, pl[5].nseg) == (256, 8, 1)
    assert [tiling_seam_voxel(t[1]) for t in TWO_KERNEL_CASES] == [(8, 8, 32), (4, 4, 32), (8, 8, 32), (8, 8, 32), (4, 4, 32)]
    assert seam_voxel((8, 16, 64), 1) == (6, 8, 32)                                          # x-seam, z-seam and y-segment boundary at once
    # the training shapes run tys = 12 .. 48 with a ragged last segment: (48, 40, 8) x 8 is that form
    big = one_pass_plan((96, 96, 96), 4)
    assert big.tys in range(12, 49)
    tp = {v: target_plan(v, 2) for v in TARGET_SHAPES}
    assert (tp[(1, 1, 1)].xtiles, tp[(1, 1, 1)].tys) == (1, 1)
    assert (tp[(7, 17, 53)].xtiles, tp[(7, 17, 53)].xo, tp[(7, 17, 53)].zt, tp[(7, 17, 53)].nseg, tp[(7, 17, 53)].tys) == (2, 27, 2, 2, 16)
    assert (tp[(13, 33, 105)].xtiles, tp[(13, 33, 105)].xo, tp[(13, 33, 105)].zt, tp[(13, 33, 105)].nseg) == (3, 35, 3, 3)
    assert (tp[(6, 16, 52)].xtiles, tp[(6, 16, 52)].xo, tp[(6, 16, 52)].zt, tp[(6, 16, 52)].nseg) == (1, 52, 1, 1)
    # blur_xy_kernel's dynamic LDS: 32 (2 Wp + 12) 4 bytes
    lds = lambda Wx: 32 * (2 * cdiv(Wx, 4) * 4 + 12) * 4
    assert lds(33) < 65536 < lds(252) < lds(384) == 99840 and lds(248) <= 65536


@pytest.mark.parametrize('fam', FAMILIES)
def test_loss_e32_of_every_family(fam):
    """e32 itself, printed: both fp32 statements stay within a few 1e-6 of float64 in this file's units."""
    for vol, p, B in (((12, 24, 60), 4, 1), ((8, 16, 64), 8, 1), ((9, 16, 33), 1, 2)):
        c = loss_case(fam, vol, p, B, 4, 'checker')
        for g_r, g_e in ((0.5, 0.185), (0.5, 0.0)):
            d64, unit = dpred_ref(c, g_r, g_e)
            for s in statements32(c, g_r, g_e):
                ed, eE = vox_err(s.dpred, d64, unit)[0], vox_err(s.Ep, c.Ep, c.S_E)[0]
                er, ee = rel_err64(s.recon, c.recon), rel_err64(s.edge, c.edge)
                print(f'E32 loss {fam} {vol} p={p} g_edge={g_e} {s.name}: dpred={ed:.2e} Ep={eE:.2e} recon={er:.2e} edge={ee:.2e}')
                assert max(ed, eE, er, ee) < 2e-5


@pytest.mark.parametrize('fam', ['gauss', 'offset', 'brain'])
def test_blur_and_target_edge_e32_of_every_family(fam):
    for vol in ((3, 4, 5), (7, 17, 53)):
        imgs, _ = volumes(fam, 1, 4, vol, 3)
        for taps in (gaussian_taps_host(2.0), asym_taps(11), gaussian_taps_host(1.0)):
            b64, S = blur_ref(imgs.double(), taps), blur_abs(imgs.double(), taps)
            e_t, e_f = vox_err(torch32_blur(imgs, taps), b64, S)[0], vox_err(blur_ref(imgs, taps), b64, S)[0]
            E64, U = edge_ref(b64)[0], edge_scale(S)[0]
            e_e = max(vox_err(R.sobel_magnitude(torch32_blur(imgs, taps)), E64, U)[0], vox_err(edge_ref(blur_ref(imgs, taps))[0], E64, U)[0])
            print(f'E32 blur {fam} {vol} taps={len(taps)}: torch={e_t:.2e} formula={e_f:.2e} edge={e_e:.2e}')
            assert max(e_f, e_e) < 2e-6 and e_t < 1e-5               # (the dense conv3d adds up 1331 products a voxel: 2 - 3e-6)


def cos_rows(Rr, D, seed, dt=F32):
    """p1, z2, p2, z1 [Rr, D]: N(0, 1) rows; row 1 x 1e3, row 2 x 1e-3, row 3 of p exactly zero, row 4 of p with norm 1e-10 (below the
    clamp of 1e-8) — as far as Rr has them; in the second pair the same rows of z are scaled instead (the zero row stays p's)."""
    g = torch.Generator().manual_seed(seed)
    p1, z2, p2, z1 = (torch.randn(Rr, D, generator=g, dtype=F64) for _ in range(4))
    for p, z in ((p1, z2), (z1, p2)):
        if Rr > 1:
            p[1] *= 1e3
        if Rr > 2:
            z[2] *= 1e-3
    for p, z in ((p1, z2), (p2, z1)):
        if Rr > 3:
            p[3] = 0.0
        if Rr > 4:
            p[4] = z[4] + 0.5 * p[4]                                  # cos ~ 0.9: the p term the clamp removes would be 1e-4 of the gradient
            p[4] *= 1e-10 / p[4].norm()
    return [t.to(dt).contiguous() for t in (p1, z2, p2, z1)]


def cos_refs(ops, w, g):
    """float64: the scalar, its unit, sum of cosines, dp1 / dp2 and their per-row units; the fp32 statements' figures"""
    Rr = ops[0].shape[0]
    o64 = [t.double() for t in ops]
    a, b = o64[0].clone().requires_grad_(True), o64[2].clone().requires_grad_(True)
    val = contr_ref(a, o64[1], b, o64[3], w)
    (val * (g / w)).backward()                                       # hp[G_CONTR] = g multiplies the mean-cosine term, w included
    c1, c2 = cos_ref(o64[0], o64[1]), cos_ref(o64[2], o64[3])
    coef = abs(g) * 0.5 / Rr

    def unit(p, z, c):
        n_p, n_z = p.norm(dim=1).clamp_min(COS_EPS), z.norm(dim=1).clamp_min(COS_EPS)
        return coef * (z.abs().amax(1) / (n_p * n_z) + c.abs() * p.abs().amax(1) / n_p ** 2)

    r = NS(val=float(val.detach()), val_unit=float(w * (c1.abs().sum() + c2.abs().sum()) / (2 * Rr)), csum=float(c1.sum() + c2.sum()),
           csum_unit=float(c1.abs().sum() + c2.abs().sum()), d1=a.grad, d2=b.grad, u1=unit(o64[0], o64[1], c1), u2=unit(o64[2], o64[3], c2))
    above = [(t.double().norm(dim=1) >= COS_EPS) | (t.double().norm(dim=1) == 0) for t in (ops[0], ops[2])]   # torch counts there
    r.e32_d, r.e32_val = [], 0.0
    for name in ('torch', 'formula'):
        a32, b32 = ops[0].clone().requires_grad_(True), ops[2].clone().requires_grad_(True)
        v32 = R.contrastive_loss(a32, b32, ops[3], ops[1], w) if name == 'torch' else contr_ref(a32, ops[1], b32, ops[3], w)
        (v32 * (g / w)).backward()
        r.e32_val = max(r.e32_val, abs(float(v32.detach()) - r.val) / r.val_unit)
        for i, (got, want, u) in enumerate(((a32.grad, r.d1, r.u1), (b32.grad, r.d2, r.u2))):
            e = _ratio((got.double() - want).abs().amax(1), u)
            if name == 'torch':
                e = torch.where(above[i], e, torch.zeros_like(e))
            r.e32_d.append(float(e.max()))
    r.e32_d = max(r.e32_d)
    return r


@pytest.mark.parametrize('D', [7, 320, 768])
def test_cosine_e32_and_rows(D):
    ops = cos_rows(5, D, 3)
    n = [t.double().norm(dim=1) for t in ops]
    assert float(n[0][3]) == 0 and 0 < float(n[0][4]) < 0.02 * COS_EPS and float(n[0][1] / n[0][0]) > 100 and float(n[1][2] / n[1][0]) < 0.01
    r = cos_refs(ops, 0.001, 0.0005)
    print(f'E32 cosine D={D}: dp={r.e32_d:.2e} scalar={r.e32_val:.2e}')
    assert r.e32_d < 2e-6 and r.e32_val < 2e-6
    # the row below the clamp: the form that keeps the p term is 1e-5 .. 1e-3 of the unit away, far outside 3 e32
    p, z = ops[0].double()[4], ops[1].double()[4]
    n_p, n_z = COS_EPS, z.norm()
    wrong = -(0.0005 * 0.5 / 5) * (z / (n_p * n_z) - (p @ z) / (n_p * n_z) * p / n_p ** 2)
    assert float((wrong - r.d1[4]).abs().max() / r.u1[4]) > 100 * max(FACTOR * r.e32_d, FLOOR)


# =========================================================================== launches (GPU)
gpu = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    from vit_ae_plus_plus_amd._abi import lib as L
    L.load()
    return L


@pytest.fixture(scope='module')
def K():
    from vit_ae_plus_plus_amd import _abi
    return _abi.CONSTS


@pytest.fixture(scope='module')
def VitaeError():
    from vit_ae_plus_plus_amd._abi import VitaeError as E
    return E


def st():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


class Buf:
    """A device array of `shape` inside a flat buffer with `off` sentinel elements in front of it and max(GUARD, one row) behind.
    The array starts as `init`, else as `inner` everywhere (NaN for outputs: an element nobody wrote shows)."""

    def __init__(self, shape, init=None, dtype=F32, inner=float('nan'), off=0, keep=False):
        shape = tuple(shape)
        n = int(np.prod(shape))
        buf = torch.full((off + n + max(GUARD, shape[-1]),), SENT, dtype=dtype)
        buf[off:off + n] = init.reshape(-1).to(dtype) if init is not None else inner
        self.orig = buf.clone() if keep else None
        self.buf, self.n, self.off = buf.cuda(), n, off
        self.t = self.buf[off:off + n].view(shape)
        self.ptr = self.t.data_ptr()
        assert self.buf.data_ptr() % 16 == 0

    def intact(self):
        return bool((self.buf[:self.off] == SENT).all()) and bool((self.buf[self.off + self.n:] == SENT).all())

    def untouched(self):
        return torch.equal(_bits(self.buf).cpu(), _bits(self.orig))


def ptr(b):
    return None if b is None else b.ptr


def all_intact(*bufs):
    torch.cuda.synchronize()
    return all(b is None or b.intact() for b in bufs)


def make_hp(K, g_r=0.0, g_e=0.0, edge_w=0.0, g_c=0.0, contr_w=0.0):
    hp = torch.zeros(K['VITAE_HP_COUNT'])
    hp[K['VITAE_HP_G_RECON']], hp[K['VITAE_HP_G_EDGE']], hp[K['VITAE_HP_EDGE_W']] = g_r, g_e, edge_w
    hp[K['VITAE_HP_G_CONTR']], hp[K['VITAE_HP_CONTR_W']] = g_c, contr_w
    return hp.cuda()


def make_acc(K):
    return torch.zeros(K['VITAE_ACC_COUNT'], dtype=F64, device='cuda')


class Rows:
    """The decoder output / its gradient as the kernels address them: [B, L (+ 1 cls row in front), P], the cls rows sentinels."""

    def __init__(self, c, cls, dtype=F32, init=None, off=0):
        rows = c.L + cls
        full = torch.full((c.B, rows, c.P), SENT if cls else float('nan'), dtype=dtype)
        full[:, cls:] = init.to(dtype) if init is not None else float('nan')
        self.b = Buf((c.B, rows, c.P), full, dtype=dtype, off=off)
        self.cls, self.bstride = cls, rows * c.P
        self.ptr = self.b.ptr + cls * c.P * self.b.t.element_size()
        self.t = self.b.t[:, cls:]

    def ok(self):
        """guards intact, cls rows untouched"""
        torch.cuda.synchronize()
        return self.b.intact() and (not self.cls or bool((self.b.t[:, 0] == SENT).all()))


def one_pass_gpu(lib, K, c, dev, hp, cls, want='both'):
    d = Rows(c, cls) if want in ('both', 'f32') else None
    d16 = Rows(c, cls, BF16) if want in ('both', 'bf16') else None
    acc, flag = make_acc(K), Buf((1,), torch.zeros(1))
    lib.vitae_loss_fwd_bwd(dev.pred.ptr, dev.pred.bstride, dev.imgs.data_ptr(), dev.mask.data_ptr(), dev.Et.data_ptr(), hp.data_ptr(), ptr(d), ptr(d16),
                           flag.ptr, acc.data_ptr(), c.msum, c.B, 4, *c.vol, c.p, st())
    assert all(r is None or r.ok() for r in (d, d16)) and all_intact(flag)
    return NS(d=None if d is None else d.t, d16=None if d16 is None else d16.t, acc=acc, flag=flag.t)


def to_dev(c, cls, off=0):
    return NS(pred=Rows(c, cls, init=c.pred, off=off), imgs=c.imgs.cuda(), mask=c.mask.cuda(), Et=c.Et.cuda())


def where_of(c, i):
    """flat index of dpred [B, L, P] -> (b, channel, z, y, x)"""
    e, l, b = i % c.P, (i // c.P) % c.L, i // (c.P * c.L)
    p, (gl, gh, gw) = c.p, (n // c.p for n in c.vol)
    ch, q, s, r = e % c.C, (e // c.C) % p, (e // (c.C * p)) % p, e // (c.C * p * p)
    return b, ch, (l // (gh * gw)) * p + r, ((l // gw) % gh) * p + s, (l % gw) * p + q


def check_dpred(label, c, got, g_r, g_e):
    d64, unit = dpred_ref(c, g_r, g_e)
    assert bool(torch.isfinite(got).all()), label
    e, i = vox_err(got, d64, unit)
    within(f'{label} dpred@{where_of(c, i)}', e, *[vox_err(s.dpred, d64, unit) for s in statements32(c, g_r, g_e)])


def check_sums(label, c, acc, K, g_r, g_e):
    s32 = statements32(c, g_r, g_e)
    a = acc.cpu()
    within(f'{label} acc[recon]', rel_err64(a[K['VITAE_ACC_RECON']], c.rsum), *[rel_err64(s.rsum, c.rsum) for s in s32])
    within(f'{label} acc[edge]', rel_err64(a[K['VITAE_ACC_EDGE']], c.esum), *[rel_err64(s.edge, c.edge) for s in s32])


def _case_options(i):
    """mask pattern, edge weight, cls row: all three take every value over consecutive cases"""
    return MASKS[i % 3], (0.37, 0.0)[(i // 3) % 2], (1, 0)[(i // 2) % 2]


@gpu
@pytest.mark.parametrize('fam', FAMILIES)
@pytest.mark.parametrize('vol,p,B', ONE_PASS_SHAPES)
def test_one_pass_loss(lib, K, monkeypatch, vol, p, B, fam):
    """vitae_loss_fwd_bwd (both outputs, the bf16 copy alone, both piece maps), vitae_loss_finalize, and the two-kernel path
    vitae_loss_fwd_fused + vitae_loss_bwd_fused on the same inputs: dpred per voxel, the cls row, both sums, the four scalars."""
    i = ONE_PASS_SHAPES.index((vol, p, B)) * len(FAMILIES) + FAMILIES.index(fam)
    for k in (i, i + 7):
        maskpat, edge_w, cls = _case_options(k)
        c = loss_case(fam, vol, p, B, 4, maskpat)
        g_up = 0.5
        g_r, g_e = g_up, edge_w * g_up
        label = f'one_pass {fam} {vol} p={p} B={B} mask={maskpat} edge_w={edge_w} cls={cls}'
        assert lib.vitae_loss_fwd_bwd_supported(4, *vol, p) == 1
        dev, hp = to_dev(c, cls), make_hp(K, g_r, g_e, edge_w)
        monkeypatch.setenv('VITAE_LOSS_XCD', '1')
        o = one_pass_gpu(lib, K, c, dev, hp, cls)
        check_dpred(label, c, o.d, g_r, g_e)
        check_sums(label, c, o.acc, K, g_r, g_e)
        assert torch.equal(o.d16, o.d.to(BF16)) and float(o.flag) == 0.0
        # the scalars
        out4 = Buf((4,))
        lib.vitae_loss_finalize(o.acc.data_ptr(), hp.data_ptr(), out4.ptr, c.msum, B * c.V, st())
        assert all_intact(out4)
        got, s32 = out4.t.cpu(), statements32(c, g_r, g_e)
        within(f'{label} out[recon]', rel_err64(got[2], c.recon), *[rel_err64(s.recon, c.recon) for s in s32])
        within(f'{label} out[edge]', rel_err64(got[1], c.edge), *[rel_err64(s.edge, c.edge) for s in s32])
        tot = edge_w * c.edge + c.recon
        within(f'{label} out[loss]', abs(float(got[0]) - tot) / (abs(edge_w * c.edge) + c.recon),
               *[abs(float(np.float32(edge_w) * np.float32(s.edge) + np.float32(s.recon)) - tot) / (abs(edge_w * c.edge) + c.recon) for s in s32])
        assert float(got[3]) == 0.0
        # bf16 only: the same bits, the same sums
        o16 = one_pass_gpu(lib, K, c, dev, hp, cls, 'bf16')
        assert torch.equal(_bits(o16.d16), _bits(o.d16)) and float(o16.flag) == 0.0
        check_sums(label + ' bf16-only', c, o16.acc, K, g_r, g_e)
        # the identity piece map: the gradient bit for bit
        monkeypatch.setenv('VITAE_LOSS_XCD', '0')
        o0 = one_pass_gpu(lib, K, c, dev, hp, cls)
        assert torch.equal(_bits(o0.d), _bits(o.d)) and torch.equal(_bits(o0.d16), _bits(o.d16))
        check_sums(label + ' xcd=0', c, o0.acc, K, g_r, g_e)
        monkeypatch.setenv('VITAE_LOSS_XCD', '1')
        two_kernel_gpu(lib, K, label.replace('one_pass', 'two_kernel'), c, dev, hp, cls, g_r, g_e)


def two_kernel_gpu(lib, K, label, c, dev, hp, cls, g_r, g_e, d_off=0, dG=True):
    """vitae_loss_fwd_fused then vitae_loss_bwd_fused (whatever kernels the geometry and the alignment pick)"""
    B, C, vol, p = c.B, c.C, c.vol, c.p
    pv, Ep, acc = Buf((B, C, *vol)), Buf((B, *vol)), make_acc(K)
    lib.vitae_loss_fwd_fused(dev.pred.ptr, dev.pred.bstride, dev.imgs.data_ptr(), dev.mask.data_ptr(), dev.Et.data_ptr(), pv.ptr, Ep.ptr, acc.data_ptr(),
                             B, C, *vol, p, st())
    assert all_intact(pv, Ep)
    assert torch.equal(pv.t.cpu(), unpatchify_ref(c.pred, p, vol, C))
    s32 = statements32(c, g_r, g_e)
    within(f'{label} Ep', vox_err(Ep.t, c.Ep, c.S_E), *[vox_err(s.Ep, c.Ep, c.S_E) for s in s32])
    check_sums(label + ' fwd', c, acc, K, g_r, g_e)
    d, d16, flag = Rows(c, cls, off=d_off), Rows(c, cls, BF16), Buf((1,), torch.zeros(1))
    ws = Buf((B * C * 3 * c.V,)) if dG else None
    lib.vitae_loss_bwd_fused(dev.pred.ptr, pv.ptr, dev.imgs.data_ptr(), dev.mask.data_ptr(), Ep.ptr, dev.Et.data_ptr(), hp.data_ptr(), ptr(ws), d.ptr, d16.ptr,
                             flag.ptr, d.bstride, c.msum, B, C, *vol, p, st())
    assert d.ok() and d16.ok() and all_intact(ws, flag)
    check_dpred(label, c, d.t, g_r, g_e)
    assert torch.equal(d16.t, d.t.to(BF16)) and float(flag.t) == 0.0
    return d


TWO_KERNEL_CASES = [('row16-false C=1', (9, 9, 33), 3, 1, 0), ('row16-true C=1', (8, 8, 36), 4, 1, 0), ('row16-false C=4', (9, 16, 33), 1, 4, 0),
                    ('three-kernel C=2', (10, 12, 34), 2, 2, 0), ('unaligned C=4', (8, 8, 36), 4, 4, 1)]


@gpu
@pytest.mark.parametrize('fam', FAMILIES)
@pytest.mark.parametrize('name,vol,p,C,off', TWO_KERNEL_CASES)
def test_two_kernel_path(lib, K, name, vol, p, C, off, fam):
    """The 8 x 8 x 32 tiling: ragged tiles in all three axes, ROW16 false (Wx % 4 != 0) and true, one and four channels; the
    three-kernel path for another channel count, and for C = 4 with pred and dpred 4 bytes off 16 (forward and backward)."""
    B = 2
    i = FAMILIES.index(fam) + [t[0] for t in TWO_KERNEL_CASES].index(name)
    for k in (i, i + 4):
        maskpat, edge_w, cls = _case_options(k)
        c = loss_case(fam, vol, p, B, C, maskpat, tiling=True)
        g_r, g_e = 0.5, edge_w * 0.5
        two_kernel_gpu(lib, K, f'two_kernel {name} {fam} {vol} p={p} mask={maskpat} edge_w={edge_w} cls={cls}', c, to_dev(c, cls, off), make_hp(K, g_r, g_e, edge_w),
                       cls, g_r, g_e, d_off=off)


@gpu
def test_three_kernel_backward_alone(lib, K):
    """vitae_recon_loss_fwd / _bwd + vitae_sobel_edge_fwd / _bwd called one by one: the same contract."""
    c = loss_case('gauss', (10, 12, 34), 2, 2, 2, 'checker')
    g_r, g_e, cls = 0.5, 0.185, 1
    dev, hp = to_dev(c, cls), make_hp(K, g_r, g_e, 0.37)
    pv, Ep, acc = Buf((c.B, c.C, *c.vol)), Buf((c.B, *c.vol)), make_acc(K)
    lib.vitae_recon_loss_fwd(dev.pred.ptr, dev.pred.bstride, dev.imgs.data_ptr(), dev.mask.data_ptr(), acc.data_ptr(), c.B, c.C, *c.vol, c.p, st())
    lib.vitae_unpatchify(dev.pred.ptr, dev.pred.bstride, pv.ptr, c.B, c.C, *c.vol, c.p, st())
    lib.vitae_sobel_edge_fwd(pv.ptr, Ep.ptr, dev.Et.data_ptr(), acc.data_ptr(), c.B, c.C, *c.vol, st())
    assert all_intact(pv, Ep) and torch.equal(pv.t.cpu(), unpatchify_ref(c.pred, c.p, c.vol, c.C))
    check_sums('three_kernel alone', c, acc, K, g_r, g_e)
    d, d16, ws = Rows(c, cls), Rows(c, cls, BF16), Buf((c.B * c.C * 3 * c.V,))
    lib.vitae_recon_loss_bwd(dev.pred.ptr, dev.pred.bstride, dev.imgs.data_ptr(), dev.mask.data_ptr(), hp.data_ptr(), d.ptr, c.msum, c.B, c.C, *c.vol, c.p, st())
    lib.vitae_sobel_edge_bwd(pv.ptr, Ep.ptr, dev.Et.data_ptr(), hp.data_ptr(), ws.ptr, d.ptr, d16.ptr, d.bstride, c.B, c.C, *c.vol, c.p, st())
    assert d.ok() and d16.ok() and all_intact(ws)
    check_dpred('three_kernel alone', c, d.t, g_r, g_e)
    assert torch.equal(d16.t, d.t.to(BF16))


@gpu
@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
def test_non_finite_prediction(lib, K, bad):
    """One NaN / +Inf in the prediction on the voxel that is behind an x-seam, a z-seam and a y-segment boundary at once: dpred is
    non-finite exactly where the float64 autograd gradient is, every other voxel stays inside the bound, the flag becomes NaN.
    With the all-ones mask, and with the checkerboard, where the voxel's patch is NOT masked: no reconstruction term carries the
    bad value there, the edge term alone has to."""
    vol, p, B = (8, 16, 64), 8, 1
    z, y, x = seam_voxel(vol, B)
    for maskpat in ('ones', 'checker'):
        base = loss_case('gauss', vol, p, B, 4, maskpat)
        patch = ((z // p) * (vol[1] // p) + y // p) * (vol[2] // p) + x // p
        assert float(base.mask[0, patch]) == (1.0 if maskpat == 'ones' else 0.0)
        pv = unpatchify_ref(base.pred, p, vol, 4).clone()
        pv[0, 1, z, y, x] = bad
        c = NS(**{k: v for k, v in vars(base).items() if k != 'stmt'})
        c.pred = patchify_ref(pv, p).contiguous()
        g_r, g_e = 0.5, 0.185
        pr = c.pred.double().requires_grad_(True)
        recon, _ = recon_ref(pr, patchify_ref(c.imgs.double(), p), c.mask.double())
        Ep = edge_ref(unpatchify_ref(pr, p, vol, 4))[0]
        (g_r * recon + g_e * ((Ep - c.Et.double()) ** 2).mean()).backward()
        d64 = pr.grad
        fin = torch.isfinite(d64)
        assert 27 <= int((~fin).sum()) <= 4 * 125 and int(fin.sum()) >= fin.numel() - 500
        # away from the bad voxel the clean case's gradient and scale hold (the stencils reach two voxels)
        far = torch.ones(vol, dtype=torch.bool)
        far[max(z - 2, 0):z + 3, max(y - 2, 0):y + 3, max(x - 2, 0):x + 3] = False
        far = patchify_ref(far.expand(1, 4, *vol), p)
        assert bool((fin | ~far).all()) and bool(((~fin) <= ~far).all())
        dref, unit = dpred_ref(base, g_r, g_e)
        assert float((d64 - dref)[far].abs().max()) <= 1e-12 * float(dref.abs().max())
        s32 = statements32(base, g_r, g_e)
        dev, hp = to_dev(c, 1), make_hp(K, g_r, g_e, 0.37)
        o = one_pass_gpu(lib, K, c, dev, hp, 1)
        pvb, Epb = Buf((B, 4, *vol)), Buf((B, *vol))
        lib.vitae_loss_fwd_fused(dev.pred.ptr, dev.pred.bstride, dev.imgs.data_ptr(), dev.mask.data_ptr(), dev.Et.data_ptr(), pvb.ptr, Epb.ptr, make_acc(K).data_ptr(),
                                 B, 4, *vol, p, st())
        d2, flag2 = Rows(c, 1), Buf((1,), torch.zeros(1))
        lib.vitae_loss_bwd_fused(dev.pred.ptr, pvb.ptr, dev.imgs.data_ptr(), dev.mask.data_ptr(), Epb.ptr, dev.Et.data_ptr(), hp.data_ptr(), None, d2.ptr, None,
                                 flag2.ptr, d2.bstride, c.msum, B, 4, *vol, p, st())
        assert d2.ok() and all_intact(pvb, Epb, flag2)
        for name, got, flag in (('one_pass', o.d, o.flag), ('two_kernel', d2.t, flag2.t)):
            got = got.cpu()
            assert torch.equal(torch.isfinite(got), fin), (name, maskpat)
            assert bool(torch.isnan(flag).all()), (name, maskpat)
            within(f'non_finite {bad} mask={maskpat} {name} dpred elsewhere', vox_err(got, dref, unit, far), *[vox_err(s.dpred, dref, unit, far) for s in s32])
        assert torch.equal(_bits(o.d16.float().nan_to_num(1.0, 2.0, 3.0)), _bits(o.d.to(BF16).float().nan_to_num(1.0, 2.0, 3.0)))


# ---- the target's edge map
TARGET_SHAPES = [(1, 1, 1), (3, 4, 5), (7, 17, 53), (13, 33, 105), (6, 16, 52)]


def target_refs(fam, vol, B, taps):
    key = ('target', fam, vol, B, taps.tobytes())
    if key not in _CACHE:
        imgs, _ = volumes(fam, B, 4, vol, 50 + sum(vol))
        b64, S = blur_ref(imgs.double(), taps), blur_abs(imgs.double(), taps)
        E64, U = edge_ref(b64)[0], edge_scale(S)[0]
        b32 = [torch32_blur(imgs, taps), blur_ref(imgs, taps)]
        E32 = [R.sobel_magnitude(b32[0]), edge_ref(b32[1])[0]]
        _CACHE[key] = NS(imgs=imgs, b64=b64, S=S, E64=E64, U=U, b32=b32, E32=E32, S_Eb=edge_scale(b64)[0])
    return _CACHE[key]


@gpu
@pytest.mark.parametrize('fam', ['gauss', 'offset', 'brain'])
@pytest.mark.parametrize('vol', TARGET_SHAPES)
def test_target_edge(lib, monkeypatch, vol, fam):
    """vitae_target_edge against float64 and against vitae_gauss_blur_fwd + vitae_sobel_edge_fwd, symmetric and asymmetric taps,
    both piece maps bit for bit."""
    B = 2
    for taps in (gaussian_taps_host(2.0), asym_taps(11)):
        r = target_refs(fam, vol, B, taps)
        assert lib.vitae_target_edge_supported(4, 11, *vol) == 1
        im = r.imgs.cuda()
        outs = []
        for xcd in ('1', '0'):
            monkeypatch.setenv('VITAE_TARGET_XCD', xcd)
            et = Buf((B, *vol))
            lib.vitae_target_edge(im.data_ptr(), et.ptr, taps.ctypes.data, 11, B, 4, *vol, st())
            assert all_intact(et)
            outs.append(et.t)
        assert torch.equal(_bits(outs[0]), _bits(outs[1]))
        label = f'target_edge {fam} {vol} {"sym" if taps[0] == taps[-1] else "asym"}'
        within(label, vox_err(outs[0], r.E64, r.U), *[vox_err(e, r.E64, r.U) for e in r.E32])
        tmp, bl, e2 = Buf((B, 4, *vol)), Buf((B, 4, *vol)), Buf((B, *vol))
        lib.vitae_gauss_blur_fwd(im.data_ptr(), tmp.ptr, bl.ptr, taps.ctypes.data, 11, B * 4, *vol, st())
        lib.vitae_sobel_edge_fwd(bl.ptr, e2.ptr, None, None, B, 4, *vol, st())
        assert all_intact(tmp, bl, e2)
        within(label + ' blur', vox_err(bl.t, r.b64, r.S), *[vox_err(b, r.b64, r.S) for b in r.b32])
        within(label + ' blur+sobel', vox_err(e2.t, r.E64, r.U), *[vox_err(e, r.E64, r.U) for e in r.E32])
        # the two ways against each other: both within the bound of float64, so at most twice the bound apart
        e32 = max(vox_err(e, r.E64, r.U)[0] for e in r.E32)
        assert vox_err(outs[0], e2.t, r.U)[0] <= 2 * max(FACTOR * e32, FLOOR)


# ---- blur
def blur_gpu(lib, label, imgs, taps):
    BC, vol = imgs.shape[0], tuple(imgs.shape[1:])
    b64, S = blur_ref(imgs.double(), taps), blur_abs(imgs.double(), taps)
    im, tmp, out = imgs.cuda(), Buf(imgs.shape), Buf(imgs.shape)
    lib.vitae_gauss_blur_fwd(im.data_ptr(), tmp.ptr, out.ptr, taps.ctypes.data, len(taps), BC, *vol, st())
    assert all_intact(tmp, out)
    dense = [vox_err(torch32_blur(imgs, taps), b64, S)] if len(taps) ** 3 * imgs.numel() < 1e8 else []
    within(label, vox_err(out.t, b64, S), vox_err(blur_ref(imgs, taps), b64, S), *dense)


BLUR11_SHAPES = [(2, 22, 9), (2, 23, 9), (2, 45, 9), (32, 3, 5), (33, 3, 5), (2, 3, 5), (2, 3, 33), (2, 3, 252), (2, 3, 384)]


@gpu
@pytest.mark.parametrize('fam', ['gauss', 'offset', 'brain'])
@pytest.mark.parametrize('vol', BLUR11_SHAPES)
def test_gauss_blur_11_taps(lib, vol, fam):
    """blur_xy_kernel (bands of 22 rows: Hy = 22, 23, 45; Wx = 5 .. 384, the last two past 64 KB of dynamic LDS) + blur_z_kernel
    (chunks of 32 planes: Lz = 32, 33)."""
    imgs = volumes(fam, 3, 1, vol, 7)[0][:, 0].contiguous()
    for taps in (gaussian_taps_host(2.0), asym_taps(11)):
        blur_gpu(lib, f'blur11 {fam} {vol} {"sym" if taps[0] == taps[-1] else "asym"}', imgs, taps)


@gpu
@pytest.mark.parametrize('fam', ['gauss', 'offset', 'brain'])
@pytest.mark.parametrize('ntaps,vol', [(5, (6, 7, 9)), (15, (6, 7, 9)), (15, (16, 17, 19)), (33, (5, 6, 40)), (33, (34, 35, 3)), (11, (2, 3, 388))])
def test_gauss_blur_generic_path(lib, ntaps, vol, fam):
    """blur_axis_kernel: every tap count but 11 (sigma 1 -> 5 taps, sigma 3 -> 15, the 33 VITAE_MAX_TAPS admits: wider than the
    volume and narrower), and 11 taps at Wx = 388 > 384."""
    imgs = volumes(fam, 2, 1, vol, 8)[0][:, 0].contiguous()
    sym = {5: gaussian_taps_host(1.0), 15: gaussian_taps_host(3.0), 33: gaussian_taps_host(6.6), 11: gaussian_taps_host(2.0)}[ntaps]
    assert len(sym) == ntaps
    for taps in (sym, asym_taps(ntaps)):
        blur_gpu(lib, f'blur_generic {fam} {vol} taps={ntaps} {"sym" if taps[0] == taps[-1] else "asym"}', imgs, taps)


# ---- cosine
def cosine_gpu(lib, K, label, Rr, D, off=0):
    w, g = 0.001, 0.0005
    ops = cos_rows(Rr, D, 17 * Rr + D)
    r = cos_refs(ops, w, g)
    dv = [Buf((Rr, D), t, off=off if i == 0 else 0) for i, t in enumerate(ops)]
    hp, acc, out = make_hp(K, g_c=g, contr_w=w), make_acc(K), Buf((1,))
    lib.vitae_cosine_loss_fwd(*(t.ptr for t in dv), acc.data_ptr(), hp.data_ptr(), out.ptr, Rr, D, st())
    assert all_intact(out)
    within(f'{label} scalar', abs(float(out.t) - r.val) / r.val_unit, r.e32_val)
    within(f'{label} acc[cos]', abs(float(acc[K['VITAE_ACC_COS']]) - r.csum) / r.csum_unit, r.e32_val)
    assert int(acc.view(torch.int32)[2 * K['VITAE_ACC_TICKET_C']]) == 0                       # the ticket is back at zero
    d1, d2 = Buf((Rr, D)), Buf((Rr, D))
    lib.vitae_cosine_loss_bwd(*(t.ptr for t in dv), hp.data_ptr(), d1.ptr, d2.ptr, Rr, D, st())
    assert all_intact(d1, d2)
    for name, got, want, u in (('dp1', d1.t, r.d1, r.u1), ('dp2', d2.t, r.d2, r.u2)):
        e = _ratio((_cpu64(got) - want).abs().amax(1), u)
        i = int(torch.argmax(torch.nan_to_num(e, nan=float('inf'))))
        within(f'{label} {name}@row{i}', float(e[i]), r.e32_d)
    for with_f32 in (True, False):
        f1, f2 = (Buf((Rr, D)), Buf((Rr, D))) if with_f32 else (None, None)
        h1, h2 = Buf((Rr, D), dtype=BF16), Buf((Rr, D), dtype=BF16)
        lib.vitae_cosine_loss_bwd_bf16(*(t.ptr for t in dv), hp.data_ptr(), ptr(f1), ptr(f2), h1.ptr, h2.ptr, Rr, D, st())
        assert all_intact(f1, f2, h1, h2)
        assert torch.equal(h1.t, d1.t.to(BF16)) and torch.equal(h2.t, d2.t.to(BF16))
        if with_f32:
            assert torch.equal(_bits(f1.t), _bits(d1.t)) and torch.equal(_bits(f2.t), _bits(d2.t))
    # a second forward on the same block (sum slot cleared, nothing else): the same scalar
    first = float(out.t)
    acc[K['VITAE_ACC_COS']] = 0
    lib.vitae_cosine_loss_fwd(*(t.ptr for t in dv), acc.data_ptr(), hp.data_ptr(), out.ptr, Rr, D, st())
    assert abs(float(out.t) - first) <= 2 * FLOOR * r.val_unit


@gpu
@pytest.mark.parametrize('Rr', [1, 4, 5, 1030])
@pytest.mark.parametrize('D', [256, 512, 768, 1024, 320, 7])
def test_cosine(lib, K, D, Rr):
    """Vector forward (D = 256 NV) and the scalar one; rows 1e3 x and 1e-3 x, a row of zeros, a row below the clamp (Rr >= 5);
    Rr = 1030: more rows than 1024 workgroups x ... cover in one pass of the forward."""
    cosine_gpu(lib, K, f'cosine R={Rr} D={D}', Rr, D)


@gpu
@pytest.mark.parametrize('D', [768, 256])
def test_cosine_unaligned_operand_takes_the_two_launch_path(lib, K, D):
    cosine_gpu(lib, K, f'cosine unaligned R=5 D={D}', 5, D, off=1)


# ---- refusals: judged before anything is launched
def _refused(VitaeError, fn, args, outs, code='VITAE_ERR_INVALID_ARG'):
    with pytest.raises(VitaeError, match=code):
        fn(*args)
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs)


def _with(args, **kw):
    a = dict(args)
    a.update(kw)
    return a


@gpu
def test_refusals_of_the_volume_launchers(lib, K, VitaeError):
    """NULL required pointers, p <= 0, extents p does not divide, non-positive extents, mask_sum <= 0, B > 65535 — every launcher of
    the chain, the outputs bit for bit what they were.  (Read from the launchers first: every guard below stands in front of the
    first launch; none of these calls reaches a kernel.)"""
    B, C, vol, p = 2, 4, (4, 4, 8), 2
    V, L, P = 128, 16, 32
    z = lambda *s: torch.zeros(*s).cuda()
    pred, imgs, mask, Et, hp = torch.randn(B, L, P, generator=torch.Generator().manual_seed(1)).cuda(), z(B, C, *vol), z(B, L) + 1, z(B, *vol), make_hp(K, 1, 1, 1)
    o = NS(acc=Buf((K['VITAE_ACC_COUNT'],), torch.zeros(K['VITAE_ACC_COUNT']), dtype=F64, keep=True), d=Buf((B, L, P), keep=True),
           d16=Buf((B, L, P), dtype=BF16, keep=True), pv=Buf((B, C, *vol), keep=True), Ep=Buf((B, *vol), keep=True),
           ws=Buf((B * C * 3 * V,), keep=True), tmp=Buf((B, C, *vol), keep=True), flag=Buf((1,), torch.zeros(1), keep=True), out4=Buf((4,), keep=True))
    outs = list(vars(o).values())
    taps = gaussian_taps_host(2.0)
    g = dict(pred=pred.data_ptr(), bs=L * P, imgs=imgs.data_ptr(), mask=mask.data_ptr(), Et=Et.data_ptr(), hp=hp.data_ptr(), acc=o.acc.ptr, d=o.d.ptr,
             d16=o.d16.ptr, pv=o.pv.ptr, Ep=o.Ep.ptr, ws=o.ws.ptr, tmp=o.tmp.ptr, flag=o.flag.ptr, msum=32.0, B=B, C=C, Lz=vol[0], Hy=vol[1], Wx=vol[2], p=p,
             taps=taps.ctypes.data, nt=11, out4=o.out4.ptr, count=B * V)
    dims = lambda a: (a['B'], a['C'], a['Lz'], a['Hy'], a['Wx'])
    forms = {
        'vitae_recon_loss_fwd': (lambda a: (a['pred'], a['bs'], a['imgs'], a['mask'], a['acc'], *dims(a), a['p'], st()), ('pred', 'imgs', 'mask', 'acc')),
        'vitae_recon_loss_bwd': (lambda a: (a['pred'], a['bs'], a['imgs'], a['mask'], a['hp'], a['d'], a['msum'], *dims(a), a['p'], st()),
                                 ('pred', 'imgs', 'mask', 'hp', 'd')),
        'vitae_unpatchify': (lambda a: (a['pred'], a['bs'], a['pv'], *dims(a), a['p'], st()), ('pred', 'pv')),
        'vitae_sobel_edge_bwd': (lambda a: (a['pv'], a['Ep'], a['Et'], a['hp'], a['ws'], a['d'], a['d16'], a['bs'], *dims(a), a['p'], st()),
                                 ('pv', 'Ep', 'Et', 'hp', 'ws', 'd')),
        'vitae_loss_fwd_fused': (lambda a: (a['pred'], a['bs'], a['imgs'], a['mask'], a['Et'], a['pv'], a['Ep'], a['acc'], *dims(a), a['p'], st()),
                                 ('pred', 'imgs', 'mask', 'Et', 'pv', 'Ep', 'acc')),
        'vitae_loss_bwd_fused': (lambda a: (a['pred'], a['pv'], a['imgs'], a['mask'], a['Ep'], a['Et'], a['hp'], a['ws'], a['d'], a['d16'], a['flag'], a['bs'],
                                            a['msum'], *dims(a), a['p'], st()), ('pred', 'pv', 'imgs', 'mask', 'Ep', 'Et', 'hp', 'd')),
        'vitae_loss_fwd_bwd': (lambda a: (a['pred'], a['bs'], a['imgs'], a['mask'], a['Et'], a['hp'], a['d'], a['d16'], a['flag'], a['acc'], a['msum'], *dims(a),
                                          a['p'], st()), ('pred', 'imgs', 'mask', 'Et', 'hp', 'acc')),
    }
    for name, (form, required) in forms.items():
        fn = getattr(lib, name)
        for r in required:
            _refused(VitaeError, fn, form(_with(g, **{r: None})), outs)
        for kw in (dict(p=0), dict(p=-2), dict(p=3), dict(Lz=5), dict(Hy=6, p=4), dict(Wx=9), dict(Lz=0), dict(Hy=0), dict(Wx=-8), dict(B=0), dict(B=-1),
                   dict(C=0), dict(B=65536)):
            if name == 'vitae_sobel_edge_bwd' and kw == dict(B=65536):
                continue                                               # its grids are strided: any B is served
            _refused(VitaeError, fn, form(_with(g, **kw)), outs)
        if name in ('vitae_recon_loss_bwd', 'vitae_loss_bwd_fused', 'vitae_loss_fwd_bwd'):
            for ms in (0.0, -1.0, float('nan')):
                _refused(VitaeError, fn, form(_with(g, msum=ms)), outs)
    _refused(VitaeError, lib.vitae_loss_fwd_bwd, forms['vitae_loss_fwd_bwd'][0](_with(g, d=None, d16=None)), outs)
    _refused(VitaeError, lib.vitae_loss_bwd_fused, forms['vitae_loss_bwd_fused'][0](_with(g, C=2, ws=None)), outs)    # (the scratch is required off C = 1, 4)
    # one-pass: what it does not serve is UNSUPPORTED, not invalid
    _refused(VitaeError, lib.vitae_loss_fwd_bwd, forms['vitae_loss_fwd_bwd'][0](_with(g, C=2)), outs, 'VITAE_ERR_UNSUPPORTED_SHAPE')
    _refused(VitaeError, lib.vitae_loss_fwd_bwd, forms['vitae_loss_fwd_bwd'][0](_with(g, pred=g['pred'] + 4)), outs, 'VITAE_ERR_UNSUPPORTED_SHAPE')
    assert lib.vitae_loss_fwd_bwd_supported(4, 4, 4, 8, 0) == 0 and lib.vitae_loss_fwd_bwd_supported(4, 4, 4, 9, 2) == 0
    # blur, Sobel forward, the target's edge map, the scalars
    blur = lambda a: (a['imgs'], a['tmp'], a['pv'], a['taps'], a['nt'], a['B'] * 4, a['Lz'], a['Hy'], a['Wx'], st())
    for kw in (dict(imgs=None), dict(tmp=None), dict(pv=None), dict(taps=None), dict(nt=0), dict(nt=10), dict(nt=2), dict(nt=35), dict(nt=K['VITAE_MAX_TAPS'] + 1),
               dict(nt=-1), dict(B=0), dict(Lz=0), dict(Hy=-3), dict(Wx=0)):
        _refused(VitaeError, lib.vitae_gauss_blur_fwd, blur(_with(g, **kw)), outs)
    sob = lambda a: (a['pv'], a['Ep'], a['Et'], a['acc'], a['B'], a['C'], a['Lz'], a['Hy'], a['Wx'], st())
    for kw in (dict(pv=None), dict(Ep=None), dict(acc=None), dict(B=0), dict(C=0), dict(Lz=0), dict(Hy=0), dict(Wx=-1)):
        _refused(VitaeError, lib.vitae_sobel_edge_fwd, sob(_with(g, **kw)), outs)
    tgt = lambda a: (a['imgs'], a['Ep'], a['taps'], a['nt'], a['B'], a['C'], a['Lz'], a['Hy'], a['Wx'], st())
    for kw in (dict(imgs=None), dict(Ep=None), dict(taps=None), dict(B=0), dict(B=65536), dict(Lz=0), dict(Hy=0), dict(Wx=0)):
        _refused(VitaeError, lib.vitae_target_edge, tgt(_with(g, **kw)), outs)
    for kw in (dict(C=2), dict(nt=9)):
        _refused(VitaeError, lib.vitae_target_edge, tgt(_with(g, **kw)), outs, 'VITAE_ERR_UNSUPPORTED_SHAPE')
    fin = lambda a: (a['acc'], a['hp'], a['out4'], a['msum'], a['count'], st())
    for kw in (dict(acc=None), dict(hp=None), dict(out4=None), dict(msum=0.0), dict(msum=-2.0), dict(count=0), dict(count=-5)):
        _refused(VitaeError, lib.vitae_loss_finalize, fin(_with(g, **kw)), outs)
    # and the good calls go through
    lib.vitae_loss_fwd_bwd(*forms['vitae_loss_fwd_bwd'][0](g))
    lib.vitae_loss_finalize(*fin(g))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o.d.t).all()) and o.d.intact() and bool(torch.isfinite(o.out4.t).all())


@gpu
def test_refusals_of_the_cosine_launchers(lib, K, VitaeError):
    Rr, D = 5, 64
    ops = [torch.ones(Rr, D).cuda() for _ in range(4)]
    hp = make_hp(K, g_c=1.0, contr_w=1.0)
    o = NS(acc=Buf((K['VITAE_ACC_COUNT'],), torch.zeros(K['VITAE_ACC_COUNT']), dtype=F64, keep=True), out=Buf((1,), keep=True), d1=Buf((Rr, D), keep=True),
           d2=Buf((Rr, D), keep=True), h1=Buf((Rr, D), dtype=BF16, keep=True), h2=Buf((Rr, D), dtype=BF16, keep=True))
    outs = list(vars(o).values())
    base = [t.data_ptr() for t in ops]
    for drop in range(7):
        a = base + [o.acc.ptr, hp.data_ptr(), o.out.ptr]
        a[drop] = None
        _refused(VitaeError, lib.vitae_cosine_loss_fwd, (*a, Rr, D, st()), outs)
        a = base + [hp.data_ptr(), o.d1.ptr, o.d2.ptr]
        a[drop] = None
        _refused(VitaeError, lib.vitae_cosine_loss_bwd, (*a, Rr, D, st()), outs)
    for r_, d_ in ((0, D), (-1, D), (Rr, 0), (Rr, -4)):
        _refused(VitaeError, lib.vitae_cosine_loss_fwd, (*base, o.acc.ptr, hp.data_ptr(), o.out.ptr, r_, d_, st()), outs)
        _refused(VitaeError, lib.vitae_cosine_loss_bwd, (*base, hp.data_ptr(), o.d1.ptr, o.d2.ptr, r_, d_, st()), outs)
        _refused(VitaeError, lib.vitae_cosine_loss_bwd_bf16, (*base, hp.data_ptr(), o.d1.ptr, o.d2.ptr, o.h1.ptr, o.h2.ptr, r_, d_, st()), outs)
    for a in ((o.d1.ptr, None, o.h1.ptr, o.h2.ptr), (None, o.d2.ptr, o.h1.ptr, o.h2.ptr), (o.d1.ptr, o.d2.ptr, None, o.h2.ptr), (o.d1.ptr, o.d2.ptr, o.h1.ptr, None)):
        _refused(VitaeError, lib.vitae_cosine_loss_bwd_bf16, (*base, hp.data_ptr(), *a, Rr, D, st()), outs)
