"""The data-side kernels — csrc/tokens.hip, csrc/input.hip, csrc/percep.hip — through the C ABI, element by element.

References (validated on the CPU, no GPU needed): every operation is written out by hand in torch and evaluated in float64 on the
fp32 inputs the kernel gets; each is checked against an independent torch formulation (stable argsort against Python's sort,
the patch gather against Tensor.unfold and the kernel's index formula, the assemblies against the cat / gather statement of the
model and its float64 autograd, the normalisations against oracle/input_ref.py, the affine against float64 grid_sample with border
padding, im2col / pooling against slicing loops).

Metric and bound per output:
  copies, gathers, one fp32 addition, bf16 casts, index outputs      bitwise, through an int16 / int32 / int64 view (NaN — as a NaN
                                                                     in that place, whatever its payload —, inf, -0.0, a denormal
                                                                     and the bf16 round-to-even ties in the inputs count)
  a bf16 output                                                      bitwise the fp32 output .to(bfloat16); a call that asks for one
                                                                     output alone gives the bits of the call that asks for both
  column sums (dcls, dmask_token, token mean, squared difference)    per column |s - s64| / sum |addends|, what the target held before
                                                                     being an addend; bitwise on integer-valued addends
  normalisation                                                      per group max |y - y64| / max |y64|
  affine resample, general matrices                                  per voxel |y - y64| / max |x over the eight taps|
  noise + gamma                                                      per element |y - y64| / |y64|
Bound: e <= max(FACTOR e32, 4 2^-24), FACTOR = 3 (tests/test_norm_kernels.py).  e32 is the same metric, on the same inputs, at run
time, of the plain fp32 statement: oracle/input_ref.py's formulas for z-score and min-max, the running sum ``seq_sum`` for column
sums, the reference formula in fp32 for the affine, torch's fp32 ``pow`` for gamma.  GAMMA_FACTOR replaces FACTOR for gamma != 1
only: the kernel raises through the hardware log2 / exp2 pair, whose error grows with |gamma log2 |v|| (see GAMMA_FACTOR below).

Input families (their claimed properties are CPU-tested):
  masking noise   distinct — equal — three (3 distinct values: ties across workgroups) — zeros (+0.0 / -0.0 / +-0.5 mixed; the two
                  zeros tie) — inf (+-inf present) — nan (NaN, and inf, present: torch's order is NaN last, ties by index)
  volumes         plain N(0.3, 2) — off100 / off1000 / offm1000: mean 100 / 1000 / -1000, std 1 — scales: a scale out of 1e-3 .. 1e3
                  per group — outlier: one 1e4 in N(0, 1) — ints: integers in -8 .. 8 (sum and sum of squares exact: the workspace
                  is compared exactly, min-max's two ends are exact)
  copies          N(0, 1) with NaN, +-inf, -0.0 and the bf16 ties 1 + 2^-8 (rounds down to even) and 1 + 3 2^-8 (rounds up)

Which sizes reach which path (from the launchers):
  vitae_random_masking     32 elements a workgroup, eight lanes an element, LDS filled 256 at a time: L = 1, 7, 8, 9 (lane rounds),
                           31, 32, 33, 63 (workgroups), 216, 257 (a second fill round), 1728; L = 15000 is the largest accepted.
  vitae_gather_patches     p = 12: the dividing decode; p = 4, 8, 16: shifts.  zsplit = min(cdiv(1024, rows), cdiv(P4, 256)), a thread
                           takes elements i0 + u 256 zsplit (u < 4) per trip: P4 = 432 -> zsplit 2, one trip with a clamped tail;
                           P4 = 1296 with 1024 rows -> zsplit 1, two trips; P4 = 4096 (p = 16, C = 4) with 1024 rows -> four trips;
                           P4 = 16 -> zsplit 1 by the cap.  (1024 rows of p = 16, C = 4 are B = 8 samples of all L = 128 patches of a
                           64 x 64 x 128 volume: keep cannot exceed L.)
  assemblies               V (16 bytes a lane) iff D % 4 == 0 and every fp32 pointer 16-byte aligned: D = 48, 300, 1028 (a second
                           trip of the row loop: 257 > 256 lanes), 1032; scalar: D = 3, 50, or a pointer 4 bytes off.
                           dcls: batches of 8 then singly: B = 1, 3, 4, 7, 8, 9, 17.  dmask_token: col_blocks = cdiv(Dd, 256) (300:
                           a partial second block; 1028: five), 32 masked rows a workgroup, four in flight: B (L - keep) = 31, 32,
                           33, 65, and 0 (keep == L: no such workgroup).
  vitae_mean_pool_tokens   256 columns a workgroup (D = 1, 255, 256, 257, 768), four tokens a trip (counts 1 .. 5, 7, 216).
  vitae_normalize_volumes  the statistics pass reads 16 bytes a lane when the group starts 16-byte aligned (group g of n floats:
                           g n % 4 == 0) and its n % 4 tail singly, else singly; min(cdiv(n / 4, 256), 512) workgroups a group:
                           n = 524288 + 1031 is a second grid-stride trip plus a tail of 3.
  vitae_noise_gamma        16 bytes a lane iff n % 4 == 0 and x, y, noise aligned; else singly.
  vitae_percep_sqdiff      min(cdiv(n / 8, 256), 2048) workgroups: n = 2048 * 256 * 8 + 8 * 300 is a second trip for 300 lanes.

Every output lives in a buffer with >= 64 sentinel elements behind it (and one in front where a pointer is offset) that no launch
may touch, and starts as NaN / -1 so that an element nobody wrote shows.  Every GPU case prints ``RATIO`` lines (run with -s);
LABNOTES.md keeps the table."""
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_norm_kernels import FACTOR, FLOOR, Buf, _ratio, all_intact, int_grad, ptr, seq_sum, st, vec_err, within

from oracle import input_ref

F32, F64, BF16, I32, I64 = torch.float32, torch.float64, torch.bfloat16, torch.int32, torch.int64
NAN = float('nan')
NS = types.SimpleNamespace
gpu = pytest.mark.gpu
# gamma != 1: y = exp2(g log2 |v|) on the transcendental units.  log2 and the product g log2 |v| = E are each rounded to fp32, an
# absolute error of up to 1.5 ulp(E) in the exponent, i.e. a relative error of ln 2 * 1.5 * 2^-23 |E| in y (|E| <= 1.35 * 20 over
# 1e-6 .. 1e3: 3e-6 at worst), where powf keeps 1 ulp = 6e-8 whatever E.  The allowed factor over e32 is the one the MI355X run
# showed against float64 (LABNOTES.md, 'Data-side kernel parity') plus a margin of 2; seeds and shapes were fixed before that run.
GAMMA_FACTOR = 42.0


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    """the bit pattern; every NaN as the one quiet NaN (a NaN must sit where the reference has one, its payload is not compared:
    torch's own CPU cast to bf16 writes 0xffff from its vectorised loop and 0x7fc0 from its scalar one)"""
    t = t.detach().cpu().contiguous()
    if t.dtype.is_floating_point:
        t = torch.where(torch.isnan(t), torch.full_like(t, NAN), t)
    return t.view({1: torch.int8, 2: torch.int16, 4: I32, 8: I64}[t.element_size()])


def bitwise(label, got, want):
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (label, got.dtype, want.dtype, got.shape, want.shape)
    bad = int((bits(got) != bits(want)).sum())
    print(f'RATIO {label}: bitwise, {bad} of {want.numel()} elements differ')
    assert bad == 0, label


def with_specials(t, seed=0):
    """t with NaN, +-inf, -0.0 and the two kinds of bf16 tie scattered over it (every 13th element from `seed`)."""
    t = t.clone()
    sp = torch.tensor([NAN, math.inf, -math.inf, -0.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 2.0 ** -130])
    f = t.view(-1)
    idx = torch.arange(seed % 13, f.numel(), 13)
    f[idx] = sp[(idx // 13) % len(sp)]
    return t


# =========================================================================== tokens.hip: references
def masking_ref(noise, keep):
    """-> ids_shuffle, ids_restore, mask: torch's stable ascending argsort (NaN last), its inverse, rank >= keep"""
    sh = torch.argsort(noise, dim=1, stable=True)
    rs = torch.argsort(sh, dim=1, stable=True)
    return sh, rs, (rs >= keep).float()


MASK_FAMILIES = ['distinct', 'equal', 'three', 'zeros', 'inf', 'nan']
MASK_L = [1, 7, 8, 9, 31, 32, 33, 63, 216, 257, 1728]


def mask_noise(fam, B, L, seed):
    g = gen(seed)
    r = torch.rand(B, L, generator=g)
    pick = torch.randint(0, 20, (B, L), generator=g)
    if fam == 'distinct':
        return torch.stack([torch.randperm(L, generator=g) for _ in range(B)]).float() / L
    if fam == 'equal':
        return torch.full((B, L), 0.5)
    if fam == 'three':
        return (pick % 3).float() * 0.25
    if fam == 'zeros':
        x = torch.tensor([0.0, -0.0, 0.5, -0.5])[pick % 4]
        if L >= 2:
            x[:, 0], x[:, L - 1] = 0.0, -0.0
        return x
    if fam == 'inf':
        r[pick == 0], r[pick == 1] = math.inf, -math.inf
        r[:, 0] = math.inf
        r[:, L // 2] = -math.inf
        return r
    if fam == 'nan':
        r[pick < 4], r[pick == 4], r[pick == 5] = NAN, math.inf, -math.inf
        r[:, L // 2] = NAN
        return r
    raise ValueError(fam)


def keeps_of(L):
    return sorted({0, 1, L - 1, L} & set(range(L + 1)))


def patches_of(x, p):
    """[B, C, Lz, Hy, Wx] -> [B, L, C p^3]: every patch as the Conv3d weight's (C, p, p, p) flattening"""
    B, C, Lz, Hy, Wx = x.shape
    g = (Lz // p, Hy // p, Wx // p)
    return x.reshape(B, C, g[0], p, g[1], p, g[2], p).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B, g[0] * g[1] * g[2], C * p ** 3)


def gather_ref(x, ids, p, keep):
    pat = patches_of(x, p)
    B, L, P = pat.shape
    return torch.gather(pat, 1, ids[:, :keep].long().unsqueeze(-1).expand(-1, -1, P)).reshape(B * keep, P)


def perm_ids(B, L, seed):
    return masking_ref(torch.rand(B, L, generator=gen(seed)), 0)[0].int()


def enc_fwd_ref(tok, cls, pos, ids, keep, dt=F32):
    B, D = ids.shape[0], tok.shape[1]
    tok, cls, pos = tok.to(dt), cls.to(dt), pos.to(dt)
    x = torch.empty(B, keep + 1, D, dtype=dt)
    x[:, 0] = cls + pos[0]
    x[:, 1:] = tok.view(B, keep, D) + pos[1 + ids[:, :keep].long()]
    return x


def dec_fwd_ref(e, mt, dpos, rs, keep, dt=F32):
    B, L = rs.shape
    e, mt, dpos, rs = e.to(dt), mt.to(dt), dpos.to(dt), rs.long()
    kept = e[:, 1:][torch.arange(B)[:, None], rs.clamp_max(max(keep - 1, 0))]
    src = torch.where((rs < keep)[..., None], kept, mt.expand(B, L, -1))
    return torch.cat([e[:, :1] + dpos[0], src + dpos[1:]], 1)


def dec_bwd_ref(dxd, sh, keep):
    """-> de (a copy of rows), the addends of dmask_token in (sample, masked rank) order"""
    B, L = sh.shape
    rows = dxd[:, 1:][torch.arange(B)[:, None], sh.long()]          # [B, L, Dd] in shuffled order
    return torch.cat([dxd[:, :1], rows[:, :keep]], 1), rows[:, keep:].reshape(B * (L - keep), dxd.shape[-1])


def mean_pool_emul(x, first):
    """The kernel's statement in fp32: four strided partial sums over the tokens, ((s0 + s1) + (s2 + s3)) / count"""
    xs = x[:, first:]
    B, cnt, D = xs.shape
    s = [torch.zeros(B, D) for _ in range(4)]
    n4 = cnt // 4 * 4
    for n in range(0, n4, 4):
        for k in range(4):
            s[k] = s[k] + xs[:, n + k]
    for n in range(n4, cnt):
        s[0] = s[0] + xs[:, n]
    t = (s[0] + s[1]) + (s[2] + s[3])
    return torch.div(t, torch.full_like(t, float(cnt)))


def colsum_check(label, got, terms, i0=None, exact=False):
    """got [D] against the float64 sum of `terms` [rows, D] (+ i0) at the bound; bitwise where the addends are integers"""
    t64 = terms.double()
    want = t64.sum(0) + (0 if i0 is None else i0.double())
    scale = t64.abs().sum(0) + (0 if i0 is None else i0.double().abs())
    r = within(label, vec_err(got, want, scale), vec_err(seq_sum(terms, i0) if terms.shape[0] else i0, want, scale))
    if exact:
        bitwise(label + ' integers', got.cpu(), want.float())
    return r


# =========================================================================== input.hip: references
NORM_MODES = {'zscore': 0, 'pm1': 1, '01': 2}
NORM_FAMILIES = ['plain', 'off100', 'off1000', 'offm1000', 'scales', 'outlier', 'ints']
# (groups, n): aligned vector path with n % 4 = 0, 1, 3; n = 4098: groups 0, 2 vector and 1, 3 scalar (group 1 = a copy of group 0's
# data); n = 4097: only groups 0 and 4 are aligned (group 4 = a copy of group 3's data); tiny; grid-stride
NORM_SHAPES = [(1, 4096), (1, 4097), (1, 4099), (4, 4098), (5, 4097), (3, 2), (3, 3), (3, 5), (2, 524288 + 1031)]
NORM_TWINS = {(4, 4098): (0, 1), (5, 4097): (3, 4)}


def norm_family(fam, G, n, seed):
    g = gen(seed)
    z = torch.randn(G, n, generator=g)
    if fam == 'plain':
        x = z * 2 + 0.3
    elif fam in ('off100', 'off1000', 'offm1000'):
        x = z + {'off100': 100.0, 'off1000': 1000.0, 'offm1000': -1000.0}[fam]
    elif fam == 'scales':
        x = z * (10.0 ** (torch.rand(G, 1, generator=g) * 6 - 3))
    elif fam == 'outlier':
        x = z.clone()
        x[torch.arange(G), (torch.arange(G) * 7 + 1) % n] = 1e4
    elif fam == 'ints':
        x = torch.randint(-8, 9, (G, n), generator=g).float()
        x[:, 0], x[:, n - 1] = -8.0, 8.0
    else:
        raise ValueError(fam)
    x = x.float().contiguous()
    if (G, n) in NORM_TWINS:
        a, b = NORM_TWINS[(G, n)]
        x[b] = x[a]
    return x


def norm_ref(x, mode, dt):
    """x [G, n]: the statements of dataset/*/: z-score with the unbiased variance, min-max to [-1, 1] or [0, 1]"""
    x = x.to(dt)
    if mode == 'zscore':
        return (x - x.mean(1, keepdim=True)) / torch.sqrt(x.var(1, keepdim=True))
    mx, mn = x.amax(1, keepdim=True), x.amin(1, keepdim=True)
    q = (x - mn) / (mx - mn)
    return 2 * q - 1 if mode == 'pm1' else q


def norm_oracle32(x, mode):
    """e32's statement: oracle/input_ref.py on the fp32 input, group by group"""
    if mode == 'zscore':
        return input_ref.normalize_data(x.view(x.shape[0], 1, 1, -1), True, per_channel=True).view_as(x)
    fn = (lambda v: input_ref.normalize_data(v, False)) if mode == 'pm1' else input_ref.min_max_normalize_data
    return torch.stack([fn(v) for v in x])


def group_err(y, ref):
    """[G, n] -> per group max |y - ref| / max |ref|"""
    y, ref = y.detach().double().cpu(), ref.detach().double().cpu()
    return _ratio((y - ref).abs().amax(1), ref.abs().amax(1))


def affine_ref(x, mats, pad, dt, levels=None):
    """x [B, C, Lz, Hy, Wx], mats [B, 12] (rows of the 3 x 4 index map output -> source), pad [B]: linear interpolation at
    s = A (l, h, w, 1); inside iff -0.5 <= s_d < n_d - 0.5 on every axis, else the pad value; both neighbours clamped to the volume.
    levels: a list that receives every intermediate (coordinates, weights, the three lerp levels)."""
    B, C, Lz, Hy, Wx = x.shape
    x, A = x.to(dt), mats.to(dt).view(B, 3, 4)
    o = torch.stack(torch.meshgrid(torch.arange(Lz), torch.arange(Hy), torch.arange(Wx), indexing='ij'), 0).to(dt)   # [3, Lz, Hy, Wx]
    a = lambda i, j: A[:, i, j].view(B, 1, 1, 1)
    s = [((a(i, 0) * o[0] + a(i, 1) * o[1]) + a(i, 2) * o[2]) + a(i, 3) for i in range(3)]                         # [B, Lz, Hy, Wx] each
    inside = torch.ones_like(s[0], dtype=torch.bool)
    for d, n in enumerate((Lz, Hy, Wx)):
        inside &= (s[d] >= -0.5) & (s[d] < n - 0.5)
    base = [torch.floor(v) for v in s]
    t = [(v - b).unsqueeze(1) for v, b in zip(s, base)]
    i0 = [b.long().clamp(0, n - 1) for b, n in zip(base, (Lz, Hy, Wx))]
    i1 = [(b.long() + 1).clamp(0, n - 1) for b, n in zip(base, (Lz, Hy, Wx))]
    bi = torch.arange(B).view(B, 1, 1, 1, 1)
    ci = torch.arange(C).view(1, C, 1, 1, 1)
    tap = lambda il, ih, iw: x[bi, ci, il.unsqueeze(1), ih.unsqueeze(1), iw.unsqueeze(1)]
    p = {(u, v, w): tap((i0, i1)[u][0], (i0, i1)[v][1], (i0, i1)[w][2]) for u in (0, 1) for v in (0, 1) for w in (0, 1)}
    lerp = lambda p0, p1, tt: p0 + tt * (p1 - p0)
    a00, a01 = lerp(p[0, 0, 0], p[0, 0, 1], t[2]), lerp(p[0, 1, 0], p[0, 1, 1], t[2])
    a10, a11 = lerp(p[1, 0, 0], p[1, 0, 1], t[2]), lerp(p[1, 1, 0], p[1, 1, 1], t[2])
    a0, a1 = lerp(a00, a01, t[1]), lerp(a10, a11, t[1])
    y = lerp(a0, a1, t[0])
    if levels is not None:
        levels.extend(s + t + [t[2] * (p[0, 0, 1] - p[0, 0, 0]), t[2] * (p[1, 1, 1] - p[1, 1, 0]), a00, a01, a10, a11,
                               t[1] * (a01 - a00), t[1] * (a11 - a10), a0, a1, t[0] * (a1 - a0), y])
    padv = torch.as_tensor(pad, dtype=dt).expand(B).view(B, 1, 1, 1, 1)
    y = torch.where(inside.unsqueeze(1), y, padv.expand_as(y))
    tapmax = torch.stack([v.abs() for v in p.values()]).amax(0)
    return y, NS(s=s, inside=inside, tapmax=tapmax)


AFFINE_EXTENTS = [(1, 5, 7), (5, 1, 3), (13, 11, 9), (16, 16, 16)]
SHIFTS = (-0.5, 0.5, -1.0, 1.0, 2.125)


def dyadic_matrices(ext):
    """name -> 3 x 4 matrix with entries and translations that are multiples of 1/8"""
    eye = torch.eye(3, 4)
    m = {'id': eye.clone(), 'perm': torch.tensor([[0., 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0]]),
         'scale': torch.tensor([[0.5, 0, 0, 0], [0, 0.75, 0, 0], [0, 0, 2.0, 0]])}
    for d in range(3):
        f = eye.clone()
        f[d, d], f[d, 3] = -1.0, float(ext[d] - 1)
        m[f'flip{d}'] = f
        for sh in SHIFTS:
            t = eye.clone()
            t[d, 3] = sh
            m[f'shift{d}{sh:+g}'] = t
    return m


def int_volume(B, C, ext, seed):
    """integers in -1024 .. 1024; channel c of sample b has the minimum -(1000 + c + 3 b) at a place of its own, so the minimum over
    the sample is channel C - 1's"""
    x = torch.randint(-900, 1025, (B, C, *ext), generator=gen(seed)).float()
    V = ext[0] * ext[1] * ext[2]
    for b in range(B):
        for c in range(C):
            x[b, c].view(-1)[(5 * c + b) % V] = -(1000.0 + c + 3 * b)
    return x


def rotations(B, ext, seed):
    """small random rotations about the volume's centre with a scale near 1 and a shift of a voxel or two, as fp32 matrices"""
    g = gen(seed)
    out = []
    for _ in range(B):
        ang = (torch.rand(3, generator=g, dtype=F64) - 0.5) * 0.5
        R = torch.eye(3, dtype=F64)
        for ax, th in enumerate(ang):
            c, s_ = math.cos(th), math.sin(th)
            i, j = [(1, 2), (0, 2), (0, 1)][ax]
            Q = torch.eye(3, dtype=F64)
            Q[i, i], Q[i, j], Q[j, i], Q[j, j] = c, -s_, s_, c
            R = R @ Q
        R = R * (0.9 + 0.2 * torch.rand(3, generator=g, dtype=F64))
        ctr = (torch.tensor(ext, dtype=F64) - 1) / 2
        tr = ctr - R @ ctr + (torch.rand(3, generator=g, dtype=F64) - 0.5) * 3
        out.append(torch.cat([R, tr[:, None]], 1).reshape(12))
    return torch.stack(out).float()


def affine_excluded(info, ext, eps=1e-4):
    """voxels whose float64 source coordinate is within eps of an inside boundary or of an integer (where fp32 may take the other
    branch)"""
    ex = torch.zeros_like(info.inside)
    for d, n in enumerate(ext):
        s = info.s[d]
        ex |= ((s + 0.5).abs() < eps) | ((s - (n - 0.5)).abs() < eps) | ((s - torch.round(s)).abs() < eps)
    return ex


def gamma_ref(x, noise, stds, gammas, dt):
    """[B, n]: v = x + std_b noise, then sign(v) |v|^gamma_b; gamma_b == 1 passes v through"""
    v = x.to(dt)
    if noise is not None:
        v = v + stds.to(dt)[:, None] * noise.to(dt)
    if gammas is None:
        return v
    g = gammas.to(dt)[:, None].expand_as(v)
    return torch.where(g == 1, v, torch.copysign(torch.pow(v.abs(), g), v))


def gamma_values(B, n, seed):
    """magnitudes log-uniform over 1e-6 .. 1e3, both signs, +0.0 and -0.0 among them"""
    g = gen(seed)
    x = 10.0 ** (torch.rand(B, n, generator=g) * 9 - 6) * (1 - 2 * torch.randint(0, 2, (B, n), generator=g)).float()
    if n >= 3:
        x[:, 1], x[:, 2] = 0.0, -0.0
    return x.float()


# =========================================================================== percep.hip: references
def im2col_first_ref(pred, target, ch, img0, n_img):
    """-> [2 n_img H W, 64] bf16: the 3 x 3 neighbourhood (zero padded) of every pixel of images img0 .. of channel ch, pred then
    target; columns 9 .. 63 zero"""
    B, C, Z, H, W = pred.shape
    rows = []
    for vol in (pred, target):
        im = vol[:, ch].reshape(B * Z, 1, H, W)[img0:img0 + n_img].to(BF16).float()
        rows.append(F.unfold(im, 3, padding=1).transpose(1, 2).reshape(n_img * H * W, 9))
    A = torch.zeros(2 * n_img * H * W, 64)
    A[:, :9] = torch.cat(rows)
    return A.to(BF16)


def im2col_ref(x):
    """x [n, H, W, C] bf16 -> [n H W, 9 C]: A[(n, y, x), (ky, kx, c)]"""
    n, H, W, C = x.shape
    u = F.unfold(x.float().permute(0, 3, 1, 2), 3, padding=1).view(n, C, 9, H * W)
    return u.permute(0, 3, 2, 1).reshape(n * H * W, 9 * C).to(BF16)


def maxpool_ref(x, drop_nan):
    """x [n, H, W, C] bf16 -> [n, H/2, W/2, C].  drop_nan: what the kernel's fmaxf chain does — a NaN loses against any number, a
    window of four NaN stays NaN; else torch's max_pool2d, which propagates NaN."""
    xf = x.float().permute(0, 3, 1, 2)
    if not drop_nan:
        return F.max_pool2d(xf, 2).permute(0, 2, 3, 1).contiguous().to(BF16)
    nan = torch.isnan(xf)
    m = F.max_pool2d(torch.where(nan, torch.full_like(xf, -math.inf), xf), 2)
    allnan = F.max_pool2d((~nan).float(), 2) == 0
    return torch.where(allnan, torch.full_like(m, NAN), m).permute(0, 2, 3, 1).contiguous().to(BF16)


def bf16_image(shape, seed, specials=True):
    x = torch.randn(*shape, generator=gen(seed))
    return (with_specials(x, seed) if specials else x).to(BF16)


# =========================================================================== CPU tests: references, inputs, claimed properties
def test_masking_reference_is_the_stable_sort_with_nan_last():
    for fam in MASK_FAMILIES:
        for L in (1, 9, 33, 257):
            noise = mask_noise(fam, 3, L, 5 + L)
            for keep in keeps_of(L):
                sh, rs, mask = masking_ref(noise, keep)
                for b in range(3):
                    v = noise[b].tolist()
                    order = sorted(range(L), key=lambda i: (math.isnan(v[i]), 0.0 if math.isnan(v[i]) or v[i] == 0 else v[i], i))
                    assert sh[b].tolist() == order, (fam, L)
                    assert sorted(sh[b].tolist()) == list(range(L))                     # a permutation, NaN or not
                    assert all(rs[b, order[k]] == k for k in range(L))
                assert float(mask.sum()) == 3 * (L - keep) and bool((mask == (rs >= keep)).all())


def test_masking_noise_families_have_the_claimed_properties():
    for L in MASK_L + [15000]:
        B = 1 if L > 2000 else 3
        x = mask_noise('distinct', B, L, 1)
        assert all(len(set(r.tolist())) == L for r in x)
        assert len(set(mask_noise('equal', B, L, 1).view(-1).tolist())) == 1
        if L >= 33:
            t = mask_noise('three', B, L, 1)
            assert all(len(set(r.tolist())) == 3 for r in t)
            z = mask_noise('zeros', B, L, 1)
            zb = bits(z)
            assert bool(((zb == 0).sum(1) > 0).all()) and bool(((zb == -2 ** 31).sum(1) > 0).all())
            i = mask_noise('inf', B, L, 1)
            assert bool(((i == math.inf).sum(1) > 0).all()) and bool(((i == -math.inf).sum(1) > 0).all()) and not bool(torch.isnan(i).any())
            n = mask_noise('nan', B, L, 1)
            assert bool((torch.isnan(n).sum(1) > 1).all()) and bool((~torch.isnan(n)).any())
    assert 15000 * 4 <= 60000 < 15001 * 4                                              # the launcher's LDS limit


def test_gather_reference_is_unfold_and_the_index_formula():
    for (B, C, ext, p, keep) in ((2, 3, (24, 12, 36), 12, 4), (2, 2, (48, 24, 40), 8, 22), (2, 1, (8, 4, 12), 4, 3)):
        x = with_specials(torch.randn(B, C, *ext, generator=gen(1)), 3)
        g = tuple(e // p for e in ext)
        L = g[0] * g[1] * g[2]
        ids = perm_ids(B, L, 2)
        ref = gather_ref(x, ids, p, keep)
        unf = x.unfold(2, p, p).unfold(3, p, p).unfold(4, p, p).permute(0, 2, 3, 4, 1, 5, 6, 7).reshape(B, L, C * p ** 3)
        assert torch.equal(bits(patches_of(x, p)), bits(unf))
        rng = np.random.default_rng(0)
        for _ in range(200):                                # out[(b keep + j), c p^3 + r p^2 + s p + q] = vol[b, c, gl p + r, gh p + s, gw p + q]
            b, j, c, r, s, q = (int(rng.integers(0, hi)) for hi in (B, keep, C, p, p, p))
            l = int(ids[b, j])
            gl, gh, gw = l // (g[1] * g[2]), (l // g[2]) % g[1], l % g[2]
            a, w = ref[b * keep + j, ((c * p + r) * p + s) * p + q], x[b, c, gl * p + r, gh * p + s, gw * p + q]
            assert torch.equal(bits(a.reshape(1)), bits(w.reshape(1)))
    t = with_specials(torch.zeros(128)).to(BF16).float()                               # the ties round to even, a denormal survives
    assert float(t[4 * 13]) == 1.0 and float(t[5 * 13]) == 1 + 2.0 ** -6 and math.isnan(float(t[0])) and float(t[7 * 13]) == 2.0 ** -130
    assert bits(with_specials(torch.ones(64)))[3 * 13] == -2 ** 31                     # -0.0


def _assemble_inputs(B, L, keep, D, seed, integer=False):
    g = gen(seed)
    sh, rs, _ = masking_ref(torch.rand(B, L, generator=g), keep)
    r = lambda *s: torch.randn(*s, generator=g)
    c = NS(B=B, L=L, keep=keep, D=D, sh=sh.int(), rs=rs.int())
    c.tok, c.cls, c.pos = r(B * keep, D), r(D), r(L + 1, D)
    c.e, c.mt, c.dpos = r(B, keep + 1, D), r(D), r(L + 1, D)
    if D * B * keep >= 16:
        c.tok.view(-1)[::7] = torch.tensor([math.inf, -0.0, -math.inf])[torch.arange(c.tok.view(-1)[::7].numel()) % 3]
        c.e.view(-1)[::11] = torch.tensor([-0.0, math.inf])[torch.arange(c.e.view(-1)[::11].numel()) % 2]
    # gradients: NaN, inf, -0.0 and bf16 ties in the rows that are copied, finite values in the rows that are summed
    c.dx = with_specials(r(B, keep + 1, D), seed)
    c.dx[:, 0] = int_grad((B, D), seed + 1) if integer else r(B, D)
    c.dxd = with_specials(r(B, L + 1, D), seed + 2)
    fin = int_grad((B, L - keep, D), seed + 3) if integer else r(B, L - keep, D)
    c.dxd[torch.arange(B)[:, None], 1 + sh[:, keep:]] = fin
    i = torch.randint(1, 6, (D,), generator=g).float() * (1 - 2 * torch.randint(0, 2, (D,), generator=g)).float()
    c.dcls0, c.dmask0 = (i, i.flip(0)) if integer else (r(D) * 0.5, r(D) * 0.5)
    return c


def test_assembly_references_are_the_models_statement_and_its_autograd():
    for (B, L, keep, D) in ((3, 12, 3, 50), (1, 12, 12, 48), (4, 12, 1, 3), (2, 9, 8, 300)):
        c = _assemble_inputs(B, L, keep, D, 7)
        ids_keep = c.sh[:, :keep].long()
        x = torch.cat([(c.cls + c.pos[0]).expand(B, 1, D), c.tok.reshape(B, keep, D) + c.pos[1:][ids_keep]], 1)
        assert torch.equal(bits(enc_fwd_ref(c.tok, c.cls, c.pos, c.sh, keep)), bits(x))
        # decoder: vit_autoenc.py's cat / repeat / gather, and its gradient
        e, mt, dxd = (torch.nan_to_num(t, 0.0, 1.0, -1.0).double() for t in (c.e, c.mt, c.dxd))
        er, mtr = e.clone().requires_grad_(True), mt.clone().requires_grad_(True)
        x_ = torch.cat([er[:, 1:], mtr.reshape(1, 1, D).repeat(B, L - keep, 1)], 1)
        x_ = torch.gather(x_, 1, c.rs.long().unsqueeze(-1).repeat(1, 1, D))
        full = torch.cat([er[:, :1], x_], 1) + c.dpos.double()
        assert torch.equal(dec_fwd_ref(e, mt, c.dpos, c.rs, keep, F64), full.detach())
        full.backward(dxd)
        de, terms = dec_bwd_ref(dxd, c.sh, keep)
        assert torch.equal(de, er.grad) and terms.shape[0] == B * (L - keep)
        assert float((terms.sum(0) - mtr.grad).abs().max()) <= 1e-12 * max(1.0, float(terms.abs().sum(0).max()))
        assert torch.equal(bits(dec_fwd_ref(c.e, c.mt, c.dpos, c.rs, keep)[:, 0]), bits(c.e[:, 0] + c.dpos[0]))
        assert bool(torch.isfinite(c.dx[:, 0]).all()) and bool(torch.isfinite(dec_bwd_ref(c.dxd, c.sh, keep)[1]).all())
        assert D < 48 or not bool(torch.isfinite(dec_bwd_ref(c.dxd, c.sh, keep)[0]).all())                      # the copied rows carry the special values
    ci = _assemble_inputs(17, 12, 3, 48, 9, integer=True)
    t = dec_bwd_ref(ci.dxd, ci.sh, 3)[1]
    assert bool((t == t.round()).all()) and bool((ci.dmask0 == ci.dmask0.round()).all()) and bool((ci.dcls0 != 0).all())
    for B, L, keep, total in DEC_TOTALS:
        assert B * (L - keep) == total
    assert [B * (L - k) for B, L, k, _ in DEC_TOTALS] == [31, 32, 33, 65]


def test_mean_pool_emulation_is_the_mean():
    for first in (0, 1):
        for cnt in (1, 2, 3, 4, 5, 7, 216):
            x = torch.randn(2, first + cnt, 5, generator=gen(cnt))
            m64 = x[:, first:].double().mean(1)
            assert float((mean_pool_emul(x, first).double() - m64).abs().max()) < 1e-6
            xi = int_grad((2, first + cnt, 5), cnt) * cnt                               # integer sums divisible by the count: exact
            assert torch.equal(mean_pool_emul(xi, first).double(), xi[:, first:].double().mean(1))


def test_normalisation_reference_is_the_oracles_and_the_families_are_what_they_claim():
    for fam in NORM_FAMILIES:
        x = norm_family(fam, 4, 4098, 3)
        x64 = x.double()
        for mode in NORM_MODES:
            o = norm_oracle32(x64, mode)
            assert float((norm_ref(x, mode, F64) - o).abs().max()) <= 1e-12 * float(o.abs().max())
            e32 = group_err(norm_oracle32(x, mode), norm_ref(x, mode, F64))
            print(f'E32 normalize {fam} {mode}: {float(e32.max()):.2e}')
            assert float(e32.max()) < 1e-4
        mean, std = x64.mean(1), x64.std(1)
        assert torch.equal(x[0], x[1])
        if fam.startswith('off'):
            off = {'off100': 100.0, 'off1000': 1000.0, 'offm1000': -1000.0}[fam]
            assert bool(((mean - off).abs() < 0.1).all()) and bool(((std - 1).abs() < 0.05).all())
        elif fam == 'outlier':
            assert bool(((x == 1e4).sum(1) == 1).all())
        elif fam == 'ints':
            assert bool((x == x.round()).all()) and float(x.max()) == 8 and float(x.min()) == -8 and 64 * (524288 + 1031) < 2 ** 53
            for mode, lo in (('pm1', -1.0), ('01', 0.0)):
                y = norm_oracle32(x, mode)
                assert bool((y[x == -8] == lo).all()) and bool((y[x == 8] == 1.0).all())
    sc = torch.cat([norm_family('scales', 5, 4097, s).double().std(1) for s in range(8)])
    assert float(sc.max() / sc.min()) > 1e3 and float(sc.min()) > 5e-4 and float(sc.max()) < 2e3
    for G, n in NORM_SHAPES:                                            # which groups start 16-byte aligned
        vec = [g for g in range(G) if (g * n) % 4 == 0]
        assert 0 in vec and (len(vec) < G or G == 1)
    assert [g for g in range(4) if (g * 4098) % 4 == 0] == [0, 2] and [g for g in range(5) if (g * 4097) % 4 == 0] == [0, 4]
    n = 524288 + 1031
    assert (n // 4 + 255) // 256 > 512 and n % 4 == 3


def test_the_fp32_sum_of_four_squares_is_what_broke_the_zscore():
    """The statistics pass as it was (four squares added in fp32, then widened) against the one that widens first, in numpy: the
    variance's sum_q - sum * mean amplifies the fp32 rounding by (mean / std)^2."""
    for off, n, least in ((100.0, 4096, 1.0), (1000.0, 4096, 10.0), (-1000.0, 64, 30.0), (1000.0, 64, 30.0), (10000.0, 4096, 100.0)):
        x = (torch.randn(n, generator=gen(int(abs(off)) + n)) + off).float().numpy()
        y64 = norm_ref(torch.from_numpy(x)[None], 'zscore', F64)[0].numpy()
        out = {}
        for name in ('fp32 quads', 'widened'):
            q4 = x.reshape(-1, 4)
            sq = (q4 * q4).sum(1, dtype=np.float32).astype(np.float64).sum() if name == 'fp32 quads' else (q4.astype(np.float64) ** 2).sum()
            s = q4.astype(np.float64).sum()
            mean = s / n
            var = (sq - s * mean) / (n - 1)
            y = (x - np.float32(mean)) * np.float32(1.0 / np.sqrt(var))
            out[name] = np.abs(y - y64).max() / np.abs(y64).max()
        e32 = float(group_err(norm_oracle32(torch.from_numpy(x)[None], 'zscore'), torch.from_numpy(y64)[None]))
        print(f'E32 zscore offset {off} n {n}: fp32 quads {out["fp32 quads"] / e32:.0f}x, widened {out["widened"] / e32:.2f}x of e32 = {e32:.2e}')
        assert out['fp32 quads'] > least * e32 and out['widened'] <= max(FACTOR * e32, FLOOR)


def test_minmax_by_reciprocal_overshoots_and_by_division_does_not():
    """fl(d * fl(1 / d)) != 1 for about one d in seven; (x - lo) / (hi - lo) with a correctly rounded division stays in [0, 1]."""
    lo, hi, x = minmax_groups(4096, 37, 1)
    d = (hi - lo)
    assert 0.05 < float(((d * (1.0 / d)) != 1).float().mean()) < 0.3
    q = (x - lo[:, None]) / d[:, None]
    assert float(q.min()) == 0.0 and float(q.max()) == 1.0 and bool((q.amax(1) == 1).all()) and bool((q.amin(1) == 0).all())
    assert float((2 * q - 1).min()) == -1.0 and float((2 * q - 1).max()) == 1.0


def minmax_groups(G, n, seed):
    """-> lo [G], hi [G], x [G, n]: groups with ranges log-uniform over 1e-3 .. 1e3 at offsets up to +-100; lo and hi are attained"""
    g = gen(seed)
    rng = 10.0 ** (torch.rand(G, generator=g) * 6 - 3)
    off = (torch.rand(G, generator=g) - 0.5) * 200
    x = (off[:, None] + rng[:, None] * torch.rand(G, n, generator=g)).float()
    return x.amin(1), x.amax(1), x


def test_affine_reference_is_grid_sample_with_border_padding():
    for ext in AFFINE_EXTENTS:
        B, C = 3, 2
        x = torch.randn(B, C, *ext, generator=gen(1))
        mats = rotations(B, ext, 2)
        pad = torch.tensor([-7.0, 0.5, 3.0])
        y, info = affine_ref(x, mats, pad, F64)
        nrm = [(2 * s / (n - 1) - 1) if n > 1 else torch.zeros_like(s) for s, n in zip(info.s, ext)]
        grid = torch.stack([nrm[2], nrm[1], nrm[0]], -1)
        gs = F.grid_sample(x.double(), grid, mode='bilinear', padding_mode='border', align_corners=True)
        gs = torch.where(info.inside.unsqueeze(1), gs, pad.double().view(B, 1, 1, 1, 1).expand_as(gs))
        assert float((y - gs).abs().max()) <= 1e-9 * float(x.abs().max()), ext
        assert 0.02 < float(info.inside.float().mean()) <= 1.0


def test_dyadic_affine_cases_are_exact_in_fp32_with_or_without_fma():
    """Every coordinate, weight, product and lerp level of the exact cases is an fp32 number already in float64, so neither the
    rounding of a product nor its absence (FMA contraction) changes a bit; the fp32 evaluation is bitwise the float64 one."""
    for ext in AFFINE_EXTENTS:
        x = int_volume(3, 3, ext, 1)
        assert float(x.abs().max()) <= 1024 and bool((x == x.round()).all())
        mins = x.amin((2, 3, 4))
        assert bool((mins[:, 2] < mins[:, 1]).all()) and bool((mins[:, 1] < mins[:, 0]).all())     # per channel distinct, the last the lowest
        M = dyadic_matrices(ext)
        assert len(M) == 21 and all(bool((m * 8 == (m * 8).round()).all()) for m in M.values())
        names = list(M)
        for i in range(0, 21, 3):
            mats = torch.stack([M[k].reshape(12) for k in names[i:i + 3]])
            lv = []
            pad = x.amin((1, 2, 3, 4))
            y64, info = affine_ref(x, mats, pad, F64, lv)
            assert all(torch.equal(v.float().double(), v) for v in lv), (ext, names[i:i + 3])
            y32, _ = affine_ref(x, mats, pad, F32)
            assert torch.equal(bits(y32), bits(y64.float()))
            for b, k in enumerate(names[i:i + 3]):
                if k.startswith('shift'):
                    d, sh = int(k[5]), float(k[6:])
                    first, last = y64[b].select(d + 1, 0), y64[b].select(d + 1, ext[d] - 1)
                    if sh == -0.5:      # source -0.5: inside, both neighbours clamp to 0
                        assert torch.equal(first, x[b].double().select(d + 1, 0))
                    if sh == 0.5:       # source n - 0.5: outside
                        assert bool((last == pad[b]).all())


def test_general_affine_excludes_under_one_percent():
    for ext in ((13, 11, 9), (16, 16, 16)):
        for seed in range(4):
            _, info = affine_ref(torch.zeros(3, 1, *ext), rotations(3, ext, seed), 0.0, F64)
            share = float(affine_excluded(info, ext).float().mean())
            print(f'affine general {ext} seed {seed}: excluded {share:.4%}, inside {float(info.inside.float().mean()):.1%}')
            assert share < 0.01


def test_gamma_reference_and_values():
    x = gamma_values(2, 1028, 1)
    assert float(x.abs()[x != 0].min()) >= 1e-6 and float(x.abs().max()) <= 1e3 and bool((x > 0).any()) and bool((x < 0).any())
    assert int(bits(x)[0, 1]) == 0 and int(bits(x)[0, 2]) == -2 ** 31
    gm = torch.tensor([0.74, 1.35])
    y = gamma_ref(x, None, None, gm, F64)
    nz = x != 0
    assert float((y[nz].abs().log() / x.double()[nz].abs().log() - gm.double()[:, None].expand_as(y)[nz]).abs().max()) < 1e-9
    assert bool((torch.sign(y) == torch.sign(x.double())).all())
    assert torch.equal(bits(gamma_ref(x, None, None, gm, F32)[:, 1:3]), bits(x[:, 1:3]))          # +-0 stays +-0
    assert torch.equal(bits(gamma_ref(x, None, None, torch.ones(2), F32)), bits(x))
    e32 = vec_err(gamma_ref(x, None, None, gm, F32), y)
    print(f'E32 gamma: {e32:.2e}')
    assert e32 < 3e-7


def test_percep_references_against_slicing():
    pred, target = (with_specials(torch.randn(2, 3, 3, 3, 5, generator=gen(s)), s) for s in (1, 2))
    A = im2col_first_ref(pred, target, 2, 1, 4)
    assert A.shape == (2 * 4 * 15, 64) and bool((bits(A[:, 9:]) == 0).all())
    for v, vol in enumerate((pred, target)):
        im = F.pad(vol[:, 2].reshape(6, 3, 5)[1:5].to(BF16), (1, 1, 1, 1))
        for ky in range(3):
            for kx in range(3):
                want = im[:, ky:ky + 3, kx:kx + 5].reshape(-1)
                assert torch.equal(bits(A[v * 60:(v + 1) * 60, ky * 3 + kx]), bits(want))
    x = bf16_image((2, 3, 5, 8), 3)
    A = im2col_ref(x).view(2, 3, 5, 9, 8)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    for ky in range(3):
        for kx in range(3):
            assert torch.equal(bits(A[:, :, :, ky * 3 + kx]), bits(xp[:, ky:ky + 3, kx:kx + 5]))
    x = bf16_image((2, 4, 6, 8), 4, specials=False)
    want = torch.stack([x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]]).float().amax(0).to(BF16)
    assert torch.equal(maxpool_ref(x, True), want) and torch.equal(maxpool_ref(x, False), want)
    xs = pool_nan_image()
    a, b = maxpool_ref(xs, True), maxpool_ref(xs, False)
    assert math.isnan(float(b[0, 0, 0, 0])) and float(a[0, 0, 0, 0]) == 5.0              # one NaN in the window: dropped / propagated
    assert math.isnan(float(a[0, 0, 1, 0])) and math.isnan(float(b[0, 0, 1, 0]))        # four NaN: NaN either way
    assert float(a[0, 0, 0, 1]) == math.inf and float(a[0, 0, 1, 1]) == -0.5


def pool_nan_image():
    x = torch.full((1, 2, 4, 8), -1.0)
    x[0, :, :2, 0] = torch.tensor([[NAN, 5.0], [2.0, 3.0]])
    x[0, :, 2:, 0] = NAN
    x[0, :, :2, 1] = torch.tensor([[math.inf, 1.0], [-math.inf, 0.0]])
    x[0, 0, 2, 1] = -0.5
    return x.to(BF16)


def test_sqdiff_integer_inputs_stay_below_2_to_24():
    a, b = sqdiff_ints(SQDIFF_BIG, 1)
    d = a.float() - b.float()
    assert bool((d.abs() <= 1).all()) and float((d * d).double().sum()) < 2 ** 24 and bool((a.float() == a.float().round()).all())
    assert SQDIFF_BIG == 2048 * 256 * 8 + 8 * 300 and (SQDIFF_BIG // 8 + 255) // 256 > 2048


SQDIFF_BIG = 2048 * 256 * 8 + 8 * 300


def sqdiff_ints(n, seed):
    g = gen(seed)
    a = torch.randint(-3, 4, (n,), generator=g).float()
    return a.to(BF16), (a + torch.randint(-1, 2, (n,), generator=g).float()).to(BF16)


# =========================================================================== launches (GPU)
@pytest.fixture(scope='module')
def lib():
    from vit_ae_plus_plus_amd._abi import lib as L
    L.load()
    return L


@pytest.fixture(scope='module')
def VitaeError():
    from vit_ae_plus_plus_amd._abi import VitaeError as E
    return E


def cu(t):
    t = t.contiguous().cuda()
    assert t.data_ptr() % 16 == 0
    return t


def refused(VitaeError, fn, args, outs):
    with pytest.raises(VitaeError):
        fn(*args)
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs)


# ---- vitae_random_masking
def masking_gpu(lib, noise, keep, want64):
    B, L = noise.shape
    nd = cu(noise)
    sh, rs, mk = Buf((B, L), dtype=I32, inner=-1), Buf((B, L), dtype=I32, inner=-1), Buf((B, L), inner=NAN)
    rs64 = Buf((B, L), dtype=I64, inner=-1) if want64 else None
    lib.vitae_random_masking(nd.data_ptr(), sh.ptr, rs.ptr, mk.ptr, ptr(rs64), B, L, keep, st())
    assert all_intact(sh, rs, mk, rs64)
    return NS(sh=sh.t.cpu(), rs=rs.t.cpu(), mask=mk.t.cpu(), rs64=None if rs64 is None else rs64.t.cpu())


def check_masking(label, noise, keep, out):
    sh, rs, mask = masking_ref(noise, keep)
    bad = sum(int((a != b).sum()) for a, b in ((out.sh, sh.int()), (out.rs, rs.int())) ) + int((bits(out.mask) != bits(mask)).sum())
    if out.rs64 is not None:
        bad += int((out.rs64 != rs).sum())
    print(f'RATIO {label}: bitwise, {bad} of {(3 + (out.rs64 is not None)) * noise.numel()} elements differ')
    assert bad == 0, label
    assert bool((out.sh.long().sort(1).values == torch.arange(noise.shape[1])).all())


@gpu
@pytest.mark.parametrize('fam', MASK_FAMILIES[:-1])
@pytest.mark.parametrize('L', MASK_L)
def test_random_masking(lib, L, fam):
    for k, keep in enumerate(keeps_of(L)):
        noise = mask_noise(fam, 3, L, 100 + L + k)
        check_masking(f'random_masking {fam} L={L} keep={keep} i64={(k + L) % 2}', noise, keep, masking_gpu(lib, noise, keep, (k + L) % 2))


@gpu
@pytest.mark.parametrize('L', MASK_L)
def test_random_masking_nan_sorts_last_and_ranks_stay_a_permutation(lib, L):
    """NaN in the noise: torch's order (NaN behind every number, ties by index).  The masking kernel alone: nothing of this goes
    into a gather."""
    for k, keep in enumerate(keeps_of(L)):
        noise = mask_noise('nan', 3, L, 200 + L + k)
        check_masking(f'random_masking nan L={L} keep={keep}', noise, keep, masking_gpu(lib, noise, keep, k % 2))
    allnan = torch.full((2, L), NAN)
    check_masking(f'random_masking all-nan L={L}', allnan, L // 2, masking_gpu(lib, allnan, L // 2, 1))


@gpu
def test_random_masking_largest_row_and_refusals(lib, VitaeError):
    noise = mask_noise('three', 1, 15000, 1)
    noise[0, ::5] = torch.rand(3000, generator=gen(2))
    check_masking('random_masking three L=15000 keep=3750', noise, 3750, masking_gpu(lib, noise, 3750, 1))
    nd = cu(torch.zeros(2, 15001))
    outs = [Buf((2, 15001), dtype=I32, keep=True), Buf((2, 15001), dtype=I32, keep=True), Buf((2, 15001), keep=True), Buf((2, 15001), dtype=I64, keep=True)]
    p = [o.ptr for o in outs]
    refused(VitaeError, lib.vitae_random_masking, (nd.data_ptr(), *p, 1, 15001, 5, st()), outs)
    refused(VitaeError, lib.vitae_random_masking, (nd.data_ptr(), *p, 1, 16, 17, st()), outs)        # keep > L
    refused(VitaeError, lib.vitae_random_masking, (nd.data_ptr(), *p, 1, 16, -1, st()), outs)
    refused(VitaeError, lib.vitae_random_masking, (nd.data_ptr(), *p, 0, 16, 4, st()), outs)
    refused(VitaeError, lib.vitae_random_masking, (nd.data_ptr(), p[0], None, p[2], p[3], 1, 16, 4, st()), outs)
    refused(VitaeError, lib.vitae_random_masking, (None, *p, 1, 16, 4, st()), outs)


# ---- vitae_gather_patches / _2views
def gather_gpu(lib, x, ids, p, keep, want, x2=None):
    """one view: x [B, ...], ids [B, L]; two views: x, x2 [B, ...] each, ids [2 B, L]"""
    B, C, Lz, Hy, Wx = x.shape
    rows, P = ids.shape[0] * keep, C * p ** 3
    xd, idd = cu(x), cu(ids)
    out = Buf((rows, P), inner=NAN) if want in ('both', 'out') else None
    out16 = Buf((rows, P), dtype=BF16, inner=NAN) if want in ('both', 'out16') else None
    if x2 is None:
        lib.vitae_gather_patches(xd.data_ptr(), idd.data_ptr(), ptr(out), ptr(out16), B, C, Lz, Hy, Wx, p, keep, st())
    else:
        x2d = cu(x2)
        lib.vitae_gather_patches_2views(xd.data_ptr(), x2d.data_ptr(), idd.data_ptr(), ptr(out), ptr(out16), B, C, Lz, Hy, Wx, p, keep, st())
    assert all_intact(out, out16)
    return NS(out=None if out is None else out.t.cpu(), out16=None if out16 is None else out16.t.cpu())


def gather_zsplit_trips(rows, C, p):
    """the launcher's plan: -> (zsplit, trips of the U * stride loop)"""
    cdiv = lambda a, b: (a + b - 1) // b
    P4 = C * p * p * (p // 4)
    z = min(cdiv(1024, rows) if rows < 1024 else 1, cdiv(P4, 256))
    return z, cdiv(P4, 4 * 256 * z)


GATHER_SMALL = [  # B, C, extents, p, keep
    (2, 1, (24, 12, 36), 12, 4), (2, 3, (24, 12, 36), 12, 6), (2, 1, (8, 4, 12), 4, 3), (2, 2, (48, 24, 40), 8, 22), (3, 4, (32, 32, 32), 16, 4)]


def test_gather_plans_of_the_tested_shapes():
    assert gather_zsplit_trips(8, 1, 12) == (2, 1) and gather_zsplit_trips(12, 3, 12) == (6, 1)        # capped by cdiv(P4, 256)
    assert gather_zsplit_trips(6, 1, 4) == (1, 1)
    assert gather_zsplit_trips(1024, 3, 12) == (1, 2) and gather_zsplit_trips(1024, 4, 16) == (1, 4)
    assert gather_zsplit_trips(44, 2, 8) == (1, 1) and gather_zsplit_trips(24, 4, 16)[0] == 16


@gpu
@pytest.mark.parametrize('B,C,ext,p,keep', GATHER_SMALL)
def test_gather_patches(lib, B, C, ext, p, keep):
    L = (ext[0] // p) * (ext[1] // p) * (ext[2] // p)
    x = with_specials(torch.randn(B, C, *ext, generator=gen(p + C)), C)
    for kp in sorted({1, keep, L}):
        ids = perm_ids(B, L, 10 + kp)
        ref = gather_ref(x, ids, p, kp)
        both = gather_gpu(lib, x, ids, p, kp, 'both')
        label = f'gather_patches p={p} C={C} {ext} keep={kp} zsplit,trips={gather_zsplit_trips(B * kp, C, p)}'
        bitwise(label + ' fp32', both.out, ref)
        bitwise(label + ' bf16', both.out16, ref.to(BF16))
        for want in ('out', 'out16'):
            alone = gather_gpu(lib, x, ids, p, kp, want)
            bitwise(f'{label} {want} alone', getattr(alone, want), getattr(both, want))


@gpu
@pytest.mark.parametrize('B,C,ext,p', [(16, 3, (48, 48, 48), 12), (8, 4, (64, 64, 128), 16)])
def test_gather_patches_1024_rows_one_zsplit_several_trips(lib, B, C, ext, p):
    L = (ext[0] // p) * (ext[1] // p) * (ext[2] // p)
    assert B * L == 1024
    x = with_specials(torch.randn(B, C, *ext, generator=gen(p)), 5)
    ids = perm_ids(B, L, 3)
    ref = gather_ref(x, ids, p, L)
    got = gather_gpu(lib, x, ids, p, L, 'both')
    label = f'gather_patches p={p} C={C} {ext} rows=1024 zsplit,trips={gather_zsplit_trips(1024, C, p)}'
    bitwise(label + ' fp32', got.out, ref)
    bitwise(label + ' bf16', got.out16, ref.to(BF16))


@gpu
@pytest.mark.parametrize('B,C,ext,p,keep', GATHER_SMALL[1:4])
def test_gather_patches_2views(lib, B, C, ext, p, keep):
    """two different volumes: rows [0, B keep) from the first with ids[:B], the rest from the second with ids[B:]; and the same
    rows as two single-view calls"""
    L = (ext[0] // p) * (ext[1] // p) * (ext[2] // p)
    x1 = with_specials(torch.randn(B, C, *ext, generator=gen(1)), 1)
    x2 = with_specials(torch.randn(B, C, *ext, generator=gen(2)), 2) + 100.0
    ids = perm_ids(2 * B, L, 4)
    ref = torch.cat([gather_ref(x1, ids[:B], p, keep), gather_ref(x2, ids[B:], p, keep)])
    label = f'gather_patches_2views p={p} C={C} {ext} keep={keep}'
    both = gather_gpu(lib, x1, ids, p, keep, 'both', x2)
    bitwise(label + ' fp32', both.out, ref)
    bitwise(label + ' bf16', both.out16, ref.to(BF16))
    for want in ('out', 'out16'):
        bitwise(f'{label} {want} alone', getattr(gather_gpu(lib, x1, ids, p, keep, want, x2), want), getattr(both, want))
    one = torch.cat([gather_gpu(lib, x1, ids[:B].contiguous(), p, keep, 'out').out, gather_gpu(lib, x2, ids[B:].contiguous(), p, keep, 'out').out])
    bitwise(label + ' = two single views', both.out, one)


@gpu
def test_gather_patches_refusals(lib, VitaeError):
    ids = cu(perm_ids(2, 64, 1))
    out, out16 = Buf((8, 4096), keep=True), Buf((8, 4096), dtype=BF16, keep=True)
    xa, xo = Buf((2, 1, 24, 24, 24), torch.zeros(2 * 24 ** 3)), Buf((2, 1, 24, 24, 24), torch.zeros(2 * 24 ** 3), off=1)
    one = lambda x, *shape: (x.ptr, ids.data_ptr(), out.ptr, out16.ptr, 2, 1, *shape, st())
    two = lambda a, b, *shape: (a.ptr, b.ptr, ids.data_ptr(), out.ptr, out16.ptr, 1, 1, *shape, st())
    for shape in ((24, 24, 24, 6, 4), (24, 24, 20, 8, 4), (20, 24, 24, 8, 4), (24, 20, 24, 8, 4), (24, 24, 24, 8, 0)):
        refused(VitaeError, lib.vitae_gather_patches, one(xa, *shape), [out, out16])
        refused(VitaeError, lib.vitae_gather_patches_2views, two(xa, xa, *shape), [out, out16])
    refused(VitaeError, lib.vitae_gather_patches, one(xo, 24, 24, 24, 8, 4), [out, out16])                 # volume 4 bytes off
    refused(VitaeError, lib.vitae_gather_patches_2views, two(xo, xa, 24, 24, 24, 8, 4), [out, out16])
    refused(VitaeError, lib.vitae_gather_patches_2views, two(xa, xo, 24, 24, 24, 8, 4), [out, out16])
    refused(VitaeError, lib.vitae_gather_patches, (xa.ptr, ids.data_ptr(), None, None, 2, 1, 24, 24, 24, 8, 4, st()), [out, out16])


# ---- the four assemblies
ASM_D = [3, 48, 50, 300, 1028, 1032]
ASM_B = [1, 3, 4, 7, 8, 9, 17]
ASM_L = 12
DEC_TOTALS = [(1, 40, 9, 31), (4, 12, 4, 32), (3, 12, 1, 33), (5, 16, 3, 65)]       # B, L, keep, B (L - keep)


def asm_gpu(lib, c, want16='both', off=None):
    """all four assemblies on one case.  off: {operand name: 1} puts that operand one element off its alignment."""
    o = lambda k: (off or {}).get(k, 0)
    B, L, keep, D = c.B, c.L, c.keep, c.D
    sh, rs = cu(c.sh), cu(c.rs)
    I = lambda name, t: Buf(t.shape, t, off=o(name))
    tok, cls, pos, e, mt, dpos = I('tok', c.tok), I('cls', c.cls), I('pos', c.pos), I('e', c.e), I('mt', c.mt), I('dpos', c.dpos)
    dx, dxd = I('dx', c.dx), I('dxd', c.dxd)
    x, xd = Buf((B, keep + 1, D), inner=NAN, off=o('x')), Buf((B, L + 1, D), inner=NAN, off=o('xd'))
    lib.vitae_encoder_assemble_fwd(tok.ptr, cls.ptr, pos.ptr, sh.data_ptr(), x.ptr, B, L, keep, D, st())
    lib.vitae_decoder_assemble_fwd(e.ptr, mt.ptr, dpos.ptr, rs.data_ptr(), xd.ptr, B, L, keep, D, st())
    dtok = Buf((B * keep, D), inner=NAN, off=o('dtok')) if want16 in ('both', 'fp32') else None
    dtok16 = Buf((B * keep, D), dtype=BF16, inner=NAN, off=o('dtok16')) if want16 in ('both', 'bf16') else None
    dcls, dmask = Buf((D,), c.dcls0), Buf((D,), c.dmask0)
    lib.vitae_encoder_assemble_bwd(dx.ptr, ptr(dtok), ptr(dtok16), dcls.ptr, B, keep, D, st())
    de = Buf((B, keep + 1, D), inner=NAN, off=o('de'))
    de16 = Buf((B, keep + 1, D), dtype=BF16, inner=NAN, off=o('de16')) if want16 in ('both', 'bf16') else None
    lib.vitae_decoder_assemble_bwd(dxd.ptr, sh.data_ptr(), de.ptr, ptr(de16), dmask.ptr, B, L, keep, D, st())
    assert all_intact(x, xd, dtok, dtok16, dcls, dmask, de, de16, tok, cls, pos, e, mt, dpos, dx, dxd)
    g = lambda b: None if b is None else b.t.cpu()
    return NS(x=g(x), xd=g(xd), dtok=g(dtok), dtok16=g(dtok16), dcls=g(dcls), dmask=g(dmask), de=g(de), de16=g(de16))


def check_asm(label, c, out, integer=False):
    B, L, keep, D = c.B, c.L, c.keep, c.D
    bitwise(f'{label} encoder_fwd', out.x, enc_fwd_ref(c.tok, c.cls, c.pos, c.sh, keep))
    bitwise(f'{label} decoder_fwd', out.xd, dec_fwd_ref(c.e, c.mt, c.dpos, c.rs, keep))
    dtok = c.dx[:, 1:].reshape(B * keep, D)
    de, terms = dec_bwd_ref(c.dxd, c.sh, keep)
    if out.dtok is not None:
        bitwise(f'{label} dtok', out.dtok, dtok)
    if out.dtok16 is not None:
        bitwise(f'{label} dtok bf16', out.dtok16, dtok.to(BF16))
    bitwise(f'{label} de', out.de, de)
    if out.de16 is not None:
        bitwise(f'{label} de bf16', out.de16, de.to(BF16))
    colsum_check(f'{label} dcls', out.dcls, c.dx[:, 0], c.dcls0, exact=integer)
    if keep == L:
        bitwise(f'{label} dmask_token untouched', out.dmask, c.dmask0)
    else:
        colsum_check(f'{label} dmask_token', out.dmask, terms, c.dmask0, exact=integer)


@gpu
@pytest.mark.parametrize('D', ASM_D)
def test_assemblies(lib, D):
    """every B and keep at one width; real and integer-valued gradients take turns (dcls / dmask_token exact on the latter)"""
    k = 0
    for B in ASM_B:
        for keep in (1, ASM_L // 4, ASM_L - 1, ASM_L):
            k += 1
            c = _assemble_inputs(B, ASM_L, keep, D, 31 * D + k, integer=bool(k % 2))
            check_asm(f'assemble D={D} B={B} L={ASM_L} keep={keep}', c, asm_gpu(lib, c), integer=bool(k % 2))


@gpu
@pytest.mark.parametrize('B,L,keep,total', DEC_TOTALS)
@pytest.mark.parametrize('D', [48, 50, 300, 1028])
def test_decoder_bwd_mask_token_row_blocks(lib, D, B, L, keep, total):
    """B (L - keep) = 31, 32, 33, 65 masked rows: one short of, at, one past a workgroup's 32, and two workgroups plus one row"""
    for integer in (True, False):
        c = _assemble_inputs(B, L, keep, D, D + total, integer=integer)
        check_asm(f'assemble masked-rows={total} D={D} B={B} L={L} keep={keep}', c, asm_gpu(lib, c), integer=integer)


@gpu
@pytest.mark.parametrize('D', [48, 300, 1028])
def test_assemblies_one_output_alone(lib, D):
    c = _assemble_inputs(3, ASM_L, 5, D, D)
    both = asm_gpu(lib, c)
    check_asm(f'assemble D={D} both', c, both)
    for want, names in (('fp32', ('dtok', 'de')), ('bf16', ('dtok16', 'de', 'de16'))):
        alone = asm_gpu(lib, c, want)
        for n in names:
            bitwise(f'assemble D={D} {n} with {want} alone', getattr(alone, n), getattr(both, n))
        bitwise(f'assemble D={D} dcls with {want} alone', alone.dcls, both.dcls)


@gpu
@pytest.mark.parametrize('which', ['tok', 'cls', 'pos', 'x', 'e', 'mt', 'dpos', 'xd', 'dx', 'dtok', 'dtok16', 'dxd', 'de', 'de16'])
def test_assemblies_a_pointer_off_alignment_takes_the_scalar_rows(lib, which):
    """D % 4 == 0 with one operand 4 bytes (bf16: 2 bytes) off: the scalar row path, the same bits, nothing written in front"""
    for D in (48, 1028):
        c = _assemble_inputs(3, ASM_L, 5, D, 3 * D, integer=True)
        check_asm(f'assemble D={D} {which} off', c, asm_gpu(lib, c, off={which: 1}), integer=True)


# ---- vitae_mean_pool_tokens
@gpu
@pytest.mark.parametrize('D', [1, 255, 256, 257, 768])
def test_mean_pool_tokens(lib, VitaeError, D):
    for B in (1, 3):
        for first in (0, 1):
            for cnt in (1, 2, 3, 4, 5, 7, 216):
                N = first + cnt
                x = torch.randn(B, N, D, generator=gen(D + cnt)) + 0.5
                if first:
                    x[:, 0] = NAN                              # the cls row must not be read into the mean
                xd, out = cu(x), Buf((B, D), inner=NAN)
                lib.vitae_mean_pool_tokens(xd.data_ptr(), out.ptr, B, N, D, first, st())
                assert all_intact(out)
                label = f'mean_pool_tokens B={B} D={D} first={first} count={cnt}'
                bitwise(label, out.t.cpu(), mean_pool_emul(x, first))
                xs = x[:, first:].double()
                want, scale = xs.mean(1), xs.abs().mean(1)
                e32 = vec_err(torch.stack([seq_sum(v) for v in x[:, first:]]) / cnt, want, scale)
                within(label, vec_err(out.t, want, scale), e32)
    out = Buf((3, D), keep=True)
    xd = cu(torch.zeros(3, 4, D))
    for N, first in ((4, 4), (4, 5), (4, -1)):
        refused(VitaeError, lib.vitae_mean_pool_tokens, (xd.data_ptr(), out.ptr, 3, N, D, first, st()), [out])


# ---- vitae_normalize_volumes
def normalize_gpu(lib, x, mode):
    G, n = x.shape
    xd, y, ws = cu(x), Buf((G, n), inner=NAN), Buf((G, 3), dtype=F64, inner=NAN)
    lib.vitae_normalize_volumes(xd.data_ptr(), y.ptr, ws.ptr, G, n, NORM_MODES[mode], st())
    assert all_intact(y, ws)
    return y.t.cpu(), ws.t.cpu()


@gpu
@pytest.mark.parametrize('fam', NORM_FAMILIES)
@pytest.mark.parametrize('G,n', NORM_SHAPES)
def test_normalize_volumes(lib, G, n, fam):
    x = norm_family(fam, G, n, 17 * G + n)
    vec = [(g * n) % 4 == 0 for g in range(G)]
    for mode in NORM_MODES:
        y64 = norm_ref(x, mode, F64)
        e32 = group_err(norm_oracle32(x, mode), y64)
        y, ws = normalize_gpu(lib, x, mode)
        e = group_err(y, y64)
        for g in range(G):
            label = f'normalize_volumes {mode} {fam} n={n} group {g}/{G} {"vector" if vec[g] else "scalar"}'
            if n == 2 and mode != 'zscore':             # two voxels: the two ends of the interval, exactly
                bitwise(label, y[g], torch.where(x[g] == x[g].max(), 1.0, -1.0 if mode == 'pm1' else 0.0))
            within(label, float(e[g]), float(e32[g]))
        if (G, n) in NORM_TWINS:                              # the same data through the vector and the scalar statistics
            a, b = NORM_TWINS[(G, n)]
            assert vec[a] != vec[b]
            within(f'normalize_volumes {mode} {fam} n={n} vector against scalar group', float(group_err(y[a][None], y[b][None].double())), float(max(e32[a], e32[b])))
        if fam == 'ints':
            x64 = x.double()
            assert torch.equal(ws[:, 0], x64.sum(1)) and torch.equal(ws[:, 1], (x64 * x64).sum(1))       # exact sums: an exact mean
            if mode != 'zscore':
                lo = -1.0 if mode == 'pm1' else 0.0
                assert bool((y[x == -8] == lo).all()) and bool((y[x == 8] == 1.0).all())


@gpu
@pytest.mark.parametrize('mode', ['pm1', '01'])
def test_minmax_stays_inside_its_interval(lib, mode):
    """4096 groups of 37 with random ranges: every output inside the interval, the minimum exactly on the lower end, the maximum on
    the upper end within the bound; how many groups miss the upper end exactly is printed."""
    lo, hi, x = minmax_groups(4096, 37, 5)
    y, _ = normalize_gpu(lib, x, mode)
    a = -1.0 if mode == 'pm1' else 0.0
    assert bool((y >= a).all()) and bool((y <= 1.0).all()), (float(y.min()), float(y.max()))
    assert bool((y[x == lo[:, None]] == a).all())
    top = y[x == hi[:, None]]
    miss = int((top != 1.0).sum())
    e32 = float(group_err(norm_oracle32(x, mode), norm_ref(x, mode, F64)).max())
    print(f'ENDPOINT minmax {mode}: {miss} of {top.numel()} maxima are not exactly 1.0')
    within(f'normalize_volumes {mode} maximum of 4096 random groups', float((top.double() - 1).abs().max()), e32)
    within(f'normalize_volumes {mode} 4096 random groups', float(group_err(y, norm_ref(x, mode, F64)).max()), e32)


@gpu
@pytest.mark.parametrize('mode', list(NORM_MODES))
def test_normalize_constant_and_nan_groups(lib, VitaeError, mode):
    """A constant group is 0 / 0 = NaN in every mode; a NaN voxel makes its whole group NaN (torch.min / max / mean propagate it) and
    leaves the other groups alone."""
    for n in (5, 4096, 4099):
        x = norm_family('plain', 6, n, n)
        x[1], x[3] = 3.0, 0.1
        x[4, n // 2] = NAN
        x[5, n - 1] = NAN
        y, _ = normalize_gpu(lib, x, mode)
        bad = [1, 3, 4, 5]
        nans = int(torch.isnan(y[bad]).sum())
        print(f'RATIO normalize_volumes {mode} n={n} constant and NaN groups: {nans} of {4 * n} NaN')
        assert nans == 4 * n
        y64 = norm_ref(x, mode, F64)
        assert bool(torch.isnan(y64[bad]).all())
        for g in (0, 2):
            within(f'normalize_volumes {mode} n={n} group {g} beside NaN groups', float(group_err(y[g][None], y64[g][None])),
                   float(group_err(norm_oracle32(x[g][None], mode), y64[g][None])))
    xd, y, ws = cu(torch.randn(4, 8)), Buf((4, 8), keep=True), Buf((65536, 3), dtype=F64, keep=True)
    for args in ((4, 1, NORM_MODES[mode]), (4, 8, 3), (4, 8, -1), (65536, 8, NORM_MODES[mode]), (0, 8, NORM_MODES[mode])):
        refused(VitaeError, lib.vitae_normalize_volumes, (xd.data_ptr(), y.ptr, ws.ptr, *args, st()), [y, ws])
    refused(VitaeError, lib.vitae_normalize_volumes, (xd.data_ptr(), y.ptr, None, 4, 8, NORM_MODES[mode], st()), [y, ws])


# ---- vitae_volume_minmax + vitae_affine_resample
def affine_gpu(lib, x, mats, pad):
    """pad: a float (constant) or 'min' (the sample's minimum through vitae_volume_minmax)"""
    B, C, Lz, Hy, Wx = x.shape
    xd, md, y = cu(x), cu(mats), Buf(x.shape, inner=NAN)
    ws = None
    if pad == 'min':
        ws = Buf((B, 3), dtype=F64, inner=NAN)
        lib.vitae_volume_minmax(xd.data_ptr(), ws.ptr, B, C * Lz * Hy * Wx, st())
    lib.vitae_affine_resample(xd.data_ptr(), y.ptr, md.data_ptr(), ptr(ws), 0.0 if pad == 'min' else pad, B, C, Lz, Hy, Wx, st())
    assert all_intact(y, ws)
    return y.t.cpu()


@gpu
@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('ext', AFFINE_EXTENTS)
def test_affine_resample_dyadic_cases_are_exact(lib, ext, C):
    x = int_volume(3, C, ext, 7 + C)
    M = dyadic_matrices(ext)
    names = list(M)
    for i in range(0, 21, 3):
        mats = torch.stack([M[k].reshape(12) for k in names[i:i + 3]])
        for pad in (-2048.0, 'min'):
            padv = x.amin((1, 2, 3, 4)) if pad == 'min' else torch.full((3,), pad)
            y64, info = affine_ref(x, mats, padv, F64)
            y = affine_gpu(lib, x, mats, pad)
            bitwise(f'affine_resample {ext} C={C} {"/".join(names[i:i + 3])} pad={pad} (outside {1 - float(info.inside.float().mean()):.0%})', y, y64.float())
            for b, k in enumerate(names[i:i + 3]):
                if k.startswith('shift') and float(k[6:]) == -0.5:
                    assert torch.equal(y[b].select(int(k[5]) + 1, 0), x[b].select(int(k[5]) + 1, 0)), k
                if k.startswith('shift') and float(k[6:]) == 0.5:
                    assert bool((y[b].select(int(k[5]) + 1, ext[int(k[5])] - 1) == padv[b]).all()), k


@gpu
@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('ext', [(13, 11, 9), (16, 16, 16)])
def test_affine_resample_rotations(lib, VitaeError, ext, C):
    for seed in range(3):
        x = torch.randn(3, C, *ext, generator=gen(seed)) * 3 + 1
        mats = rotations(3, ext, seed)
        for pad in (0.25, 'min'):
            padv = x.amin((1, 2, 3, 4)) if pad == 'min' else torch.full((3,), pad)
            y64, info = affine_ref(x, mats, padv, F64)
            y32, _ = affine_ref(x, mats, padv, F32)
            ok = ~affine_excluded(info, ext).unsqueeze(1).expand_as(y64)
            assert float((~ok).float().mean()) < 0.01
            y = affine_gpu(lib, x, mats, pad)
            err = lambda t: float(_ratio((t.double() - y64).abs()[ok], info.tapmax[ok]).max())
            within(f'affine_resample rotations {ext} C={C} seed={seed} pad={pad} (outside {1 - float(info.inside.float().mean()):.0%})', err(y), err(y32))
            assert torch.equal(bits(y[~info.inside.unsqueeze(1).expand_as(y) & ok]), bits(padv.view(3, 1, 1, 1, 1).expand_as(y)[~info.inside.unsqueeze(1).expand_as(y) & ok]))
    xb = Buf((3, C, *ext), keep=True)
    md = cu(rotations(3, ext, 0))
    refused(VitaeError, lib.vitae_affine_resample, (xb.ptr, xb.ptr, md.data_ptr(), None, 0.0, 3, C, *ext, st()), [xb])
    refused(VitaeError, lib.vitae_affine_resample, (xb.ptr, None, md.data_ptr(), None, 0.0, 3, C, *ext, st()), [xb])
    ws = Buf((3, 3), dtype=F64, keep=True)
    refused(VitaeError, lib.vitae_volume_minmax, (xb.ptr, ws.ptr, 65536, 4, st()), [ws])
    refused(VitaeError, lib.vitae_volume_minmax, (xb.ptr, ws.ptr, 3, 0, st()), [ws])


# ---- vitae_noise_gamma
def noise_gamma_gpu(lib, x, noise, stds, gammas, off=None):
    o = lambda k: (off or {}).get(k, 0)
    B, n = x.shape
    xb = Buf((B, n), x, off=o('x'))
    nb = None if noise is None else Buf((B, n), noise, off=o('noise'))
    y = Buf((B, n), inner=NAN, off=o('y'))
    sd, gm = (None if t is None else cu(t) for t in (stds, gammas))
    lib.vitae_noise_gamma(xb.ptr, ptr(nb), y.ptr, None if sd is None else sd.data_ptr(), None if gm is None else gm.data_ptr(), B, n, st())
    assert all_intact(y, xb, nb)
    return y.t.cpu()


GAMMA_N = [1, 3, 4, 1023, 1024, 1028]


@gpu
@pytest.mark.parametrize('n', GAMMA_N)
def test_noise_gamma(lib, n):
    B = 2
    x, z = gamma_values(B, n, n), torch.randn(B, n, generator=gen(n + 1))
    sd, gm, one = torch.tensor([0.05, 0.2]), torch.tensor([0.74, 1.35]), torch.ones(B)
    label = f'noise_gamma n={n}'
    bitwise(f'{label} nothing to do', noise_gamma_gpu(lib, x, None, None, None), x)
    bitwise(f'{label} stds without noise, gamma = 1', noise_gamma_gpu(lib, x, None, sd, one), x)
    # noise alone: one product and one sum, contracted or not
    v64 = gamma_ref(x, z, sd, None, F64)
    scale = x.double().abs() + (sd.double()[:, None] * z.double()).abs()
    yn = noise_gamma_gpu(lib, x, z, sd, None)
    within(f'{label} noise', vec_err(yn, v64, scale), vec_err(gamma_ref(x, z, sd, None, F32), v64, scale))
    bitwise(f'{label} noise, gamma = 1 passes it through', noise_gamma_gpu(lib, x, z, sd, one), yn)
    # gamma alone
    y64 = gamma_ref(x, None, None, gm, F64)
    y = noise_gamma_gpu(lib, x, None, None, gm)
    gamma_within(f'{label} gamma', y, y64, gamma_ref(x, None, None, gm, F32))
    zero = x == 0
    assert torch.equal(bits(y[zero]), bits(x[zero]))                                                    # +-0 stays +-0
    assert bool((torch.sign(y) == torch.sign(x)).all())
    one_each = torch.tensor([1.0, 1.35])
    ym = noise_gamma_gpu(lib, x, None, None, one_each)
    bitwise(f'{label} gamma = 1 in sample 0 only', ym[0], x[0])
    bitwise(f'{label} gamma = 1.35 in sample 1 only', ym[1], y[1])
    # both: the reference raises the kernel's own noisy value (cancellation in x + std z is the noise case's business)
    yb = noise_gamma_gpu(lib, x, z, sd, gm)
    gamma_within(f'{label} noise + gamma', yb, gamma_ref(yn, None, None, gm, F64), gamma_ref(yn, None, None, gm, F32))


def gamma_within(label, y, y64, y32):
    e, e32 = vec_err(y, y64), vec_err(y32, y64)
    print(f'RATIO {label}: e={e:.3e} e32={e32:.3e} ratio={e / e32 if e32 > 0 else float(e > 0):.2f} (allowed {GAMMA_FACTOR})')
    assert e <= max(GAMMA_FACTOR * e32, FLOOR), (label, e, e32)


@gpu
@pytest.mark.parametrize('which', ['x', 'noise', 'y'])
def test_noise_gamma_a_pointer_off_alignment_gives_the_same_bits(lib, VitaeError, which):
    B, n = 2, 1028
    x, z = gamma_values(B, n, 3), torch.randn(B, n, generator=gen(4))
    sd, gm = torch.tensor([0.05, 0.2]), torch.tensor([0.74, 1.35])
    bitwise(f'noise_gamma n={n} {which} 4 bytes off', noise_gamma_gpu(lib, x, z, sd, gm, off={which: 1}), noise_gamma_gpu(lib, x, z, sd, gm))
    xb, nb, y = cu(x), cu(z), Buf((B, n), keep=True)
    g = cu(gm)
    refused(VitaeError, lib.vitae_noise_gamma, (xb.data_ptr(), nb.data_ptr(), y.ptr, None, g.data_ptr(), B, n, st()), [y])   # noise without stds
    refused(VitaeError, lib.vitae_noise_gamma, (xb.data_ptr(), None, y.ptr, None, g.data_ptr(), B, 0, st()), [y])
    refused(VitaeError, lib.vitae_noise_gamma, (None, None, y.ptr, None, g.data_ptr(), B, n, st()), [y])


# ---- percep.hip
@gpu
@pytest.mark.parametrize('H,W', [(2, 2), (3, 5), (16, 24)])
def test_percep_im2col_first(lib, VitaeError, H, W):
    B, C, Z = 2, 3, 3
    pred, target = (with_specials(torch.randn(B, C, Z, H, W, generator=gen(s)), s) for s in (1, 2))
    pd, td = cu(pred), cu(target)
    for ch in (0, C - 1):
        for img0, n_img in ((0, B * Z), (1, 4), (5, 1)):
            A = Buf((2 * n_img * H * W, 64), dtype=BF16, inner=NAN)
            lib.vitae_percep_im2col_first(pd.data_ptr(), td.data_ptr(), A.ptr, B, C, ch, Z, H, W, img0, n_img, st())
            assert all_intact(A)
            got = A.t.cpu()
            bitwise(f'percep_im2col_first {H}x{W} channel={ch} img0={img0} n_img={n_img}', got, im2col_first_ref(pred, target, ch, img0, n_img))
            assert bool((bits(got[:, 9:]) == 0).all())
    A = Buf((2 * H * W, 64), dtype=BF16, keep=True)
    for args in ((B, C, C, Z, H, W, 0, 1), (B, C, -1, Z, H, W, 0, 1), (B, C, 0, Z, H, W, B * Z, 1), (B, C, 0, Z, H, W, 0, 0), (B, C, 0, Z, H, W, -1, 1)):
        refused(VitaeError, lib.vitae_percep_im2col_first, (pd.data_ptr(), td.data_ptr(), A.ptr, *args, st()), [A])


@gpu
@pytest.mark.parametrize('Cin', [8, 64])
@pytest.mark.parametrize('H,W', [(2, 2), (3, 5), (16, 24)])
def test_percep_im2col_and_maxpool(lib, VitaeError, H, W, Cin):
    n = 3
    x = bf16_image((n, H, W, Cin), H + Cin)
    xd = cu(x)
    A = Buf((n * H * W, 9 * Cin), dtype=BF16, inner=NAN)
    lib.vitae_percep_im2col(xd.data_ptr(), A.ptr, n, H, W, Cin, st())
    assert all_intact(A)
    bitwise(f'percep_im2col {H}x{W} Cin={Cin}', A.t.cpu(), im2col_ref(x))
    keepA = Buf((n * H * W, 9 * Cin), dtype=BF16, keep=True)
    refused(VitaeError, lib.vitae_percep_im2col, (xd.data_ptr(), keepA.ptr, n, H, W, Cin + 4, st()), [keepA])
    refused(VitaeError, lib.vitae_percep_im2col, (xd.data_ptr(), keepA.ptr, 0, H, W, Cin, st()), [keepA])
    if H % 2 == 0:
        # no NaN in the values here: what the pool does with one is test_percep_maxpool_nan's business
        xp = torch.nan_to_num(x.float(), nan=0.375, posinf=math.inf, neginf=-math.inf).to(BF16)
        out = Buf((n, H // 2, W // 2, Cin), dtype=BF16, inner=NAN)
        xpd = cu(xp)
        lib.vitae_percep_maxpool2(xpd.data_ptr(), out.ptr, n, H, W, Cin, st())
        assert all_intact(out)
        bitwise(f'percep_maxpool2 {H}x{W} C={Cin}', out.t.cpu(), maxpool_ref(xp, False))
    else:
        keepO = Buf((n, 2, 3, Cin), dtype=BF16, keep=True)
        refused(VitaeError, lib.vitae_percep_maxpool2, (xd.data_ptr(), keepO.ptr, n, H, W, Cin, st()), [keepO])
        refused(VitaeError, lib.vitae_percep_maxpool2, (xd.data_ptr(), keepO.ptr, n, 2, 2, 12, st()), [keepO])


@gpu
def test_percep_maxpool_nan(lib):
    """Pinned difference to torch: the pool's fmaxf chain lets a NaN lose against any number of its window; only a
    window of four NaN gives NaN.  F.max_pool2d propagates every NaN."""
    x = torch.cat([pool_nan_image(), with_specials(torch.randn(1, 2, 4, 8, generator=gen(1)), 0).to(BF16)])
    out = Buf((2, 1, 2, 8), dtype=BF16, inner=NAN)
    xd = cu(x)
    lib.vitae_percep_maxpool2(xd.data_ptr(), out.ptr, 2, 2, 4, 8, st())
    assert all_intact(out)
    got = out.t.cpu()
    bitwise('percep_maxpool2 NaN loses against numbers', got, maxpool_ref(x, True))
    assert int(torch.isnan(maxpool_ref(x, False)).sum()) > int(torch.isnan(got).sum()) > 0


@gpu
@pytest.mark.parametrize('n', [8, SQDIFF_BIG])
def test_percep_sqdiff(lib, VitaeError, n):
    for integer in (True, False):
        if integer:
            a, b = sqdiff_ints(n, n % 97)
        else:
            a, b = (torch.randn(n, generator=gen(s)).to(BF16) for s in (1, 2))
        acc0 = 12345.0 if integer else 0.3
        acc = Buf((1,), torch.tensor([acc0], dtype=F64), dtype=F64)
        ad, bd = cu(a), cu(b)
        lib.vitae_percep_sqdiff(ad.data_ptr(), bd.data_ptr(), n, acc.ptr, st())
        assert all_intact(acc)
        d = a.double() - b.double()
        total = float((d * d).sum())
        got = float(acc.t.cpu()[0])
        d32 = a.float() - b.float()
        s32 = float(seq_sum((d32 * d32)[:, None])[0]) if n <= 64 else float((d32 * d32).sum())
        label = f'percep_sqdiff n={n} {"integers" if integer else "real"} onto {acc0}'
        within(label, abs(got - (acc0 + total)) / (acc0 + total), abs(s32 - total) / (acc0 + total))
        if integer:
            assert got == acc0 + total, (got, acc0 + total)
    keep = Buf((1,), torch.tensor([1.5], dtype=F64), dtype=F64, keep=True)
    refused(VitaeError, lib.vitae_percep_sqdiff, (ad.data_ptr(), ad.data_ptr(), 12, keep.ptr, st()), [keep])
    refused(VitaeError, lib.vitae_percep_sqdiff, (ad.data_ptr(), ad.data_ptr(), 0, keep.ptr, st()), [keep])
    refused(VitaeError, lib.vitae_percep_sqdiff, (ad.data_ptr(), None, 8, keep.ptr, st()), [keep])
    refused(VitaeError, lib.vitae_percep_sqdiff, (ad.data_ptr(), ad.data_ptr(), 8, None, st()), [keep])
