"""The kernels of csrc/norm.hip — LayerNorm, BatchNorm1d + ReLU, column sums — against float64, row by row and column by column.

References (validated on the CPU, no GPU needed): every operation is written out by hand in torch (``ln_fwd_ref``, ``ln_bwd_ref``,
``bn_fwd_ref``, ``bn_bwd_ref``, ``bn_eval_ref``) with two-pass statistics and evaluated in float64 on the fp32 inputs the kernel gets
(eps and momentum as the floats the launcher receives).  On plain inputs they equal float64 ``F.layer_norm`` / ``nn.BatchNorm1d``
autograd to 1e-12.  nn.BatchNorm1d in float64 is NOT the reference at ReLU's edge: a constant column with zero bias gives it a
pre-activation that is float64 round-off noise, hence a mask of random signs; the hand-written form yields an exact zero there.

The backward kernels take mean / rstd (and BatchNorm's y) as inputs and are tested twice: 'chain' — fed by the forward kernel's own
outputs, reference end to end from x; 'isolated' — fed the float64 statistics rounded to fp32, reference computed from those same
rounded numbers.  BatchNorm's ReLU mask is ``y > 0`` of the y array the kernel is given (its contract), in the reference too.

Metric: the error in units of what is being subtracted, per row or per column, then the worst row / column:
  LayerNorm y      per row      max_c |y - y64| / max_c |y64|
  LayerNorm dx     per row      max_c |dx - dx64| / (rstd64 max_c |dy w|)       (|dx| itself is round-off where the terms cancel)
  BatchNorm y      per column   max_r |y - y64| / max_r |y64|                   (absolute where the column is all zero)
  BatchNorm dx     per column   max_r |dx - dx64| / (|w| rstd64 max_r |g|)      g = dy where y > 0
  column sums      per column   |s - s64| / sum of the |addends|                dw, db, dx_colsum, colsum_accum, running statistics;
                                                                                what the target held before is an addend
  mean             |mean - mean64| / (|mean64| + std64);   rstd: relative.
A zero denominator demands a zero numerator.

Bound: e <= max(FACTOR e32, 4 2^-24) with FACTOR = 3 (test_optimizer_kernels.FACTOR: margin for FMA contraction and summation order).
e32 is the same metric, on the same inputs, at run time, of the plain fp32 statement — the larger of torch's own fp32 op on the CPU
and the reference formula evaluated in fp32 (its column sums as the running sum `out += term` the formula states, ``seq_sum``).  The floor is there because e32 is exactly zero on some of the inputs below.
bf16 copies are bitwise ``fp32 output .to(bfloat16)``; a call that asks for the bf16 output alone gives the bf16 output of the call
that asks for both.  Integer-valued gradients make every pure column sum exact in any order: db, colsum_accum and the record sums
of vitae_ln_grad_reduce are then compared bitwise (a dropped or doubled row / workgroup / record shows as a whole number).

Input families (``ln_family`` / ``bn_family``; their claimed properties are CPU-tested): plain N(0.3, 2) — offset: row (column)
means +-1000, std 1 — tiny: std 1e-4 (variance 1e-8 << eps 1e-6) / a BatchNorm column of std 1e-3 (variance 1e-6 against eps 1e-5) —
scales: per-row (column) scales log-uniform over 1e-3 .. 1e3 — const: every third row (columns 0 and 1) a small integer constant, so
sum and mean are exact in any order: mean == c, LayerNorm y == b bitwise, BatchNorm y == relu(b), and with bias exactly 0 (column 0)
y == 0, dx == 0 and the column adds 0 to dw and db — outlier: one 1e4 in N(0, 1) — ramp (BatchNorm): column 0 = 0.25 row, split means
far apart (the n_i (mean_i - mean)^2 term of the Chan merge is nearly all of M2).

Which sizes reach which path (from the launchers; VITAE_LN_VEC / VITAE_LN_BWD_BLOCKS / VITAE_LN_PART_BLOCKS are read once per process
and are not touched):
  vitae_layernorm_fwd   vec<NV> iff D = 256 NV (NV 1..4) and x, w, b, y 16-byte / y_bf16 8-byte aligned; else the scalar kernel, a
                        lane owning columns lane + 64 i: D = 63 / 64 / 65 are one short of, at, and one past the first lane round;
                        769 .. 1023 need i >= 12; 4 rows a workgroup, so M = 1, 5, 33 are a partial, 1 + partial and 8 + partial.
  vitae_layernorm_bwd   D in {256, 512, 768} aligned: rows_vec<2, NV> on min(cdiv(M, 8), 128) workgroups — M = 1027 gives 129 row
                        groups, so workgroup 0 takes a second one (the grid-stride loop); D <= 768 otherwise (or unaligned):
                        rows_kernel<2>, 8 rows a workgroup (M = 7, 8, 9: partial, full, one over); D > 768: the generic kernel on
                        min(cdiv(M, 4), 256) workgroups = 1024 waves, a second row per wave from M = 1025 (M = 1027).
  vitae_layernorm_bwd_part   min(cdiv(M, 8), 256) records; a workgroup takes groups blockIdx, + G, + 2 G .. with two register sets:
                        M = 2047 / 2049 / 4097 / 6145 are 1 / 2 / 3 / 4 groups for workgroup 0 (1, 2 for the others).
  vitae_ln_grad_reduce  lane j of 16 sums records j, j + 16, ..: the 8x-unrolled loop runs while g + 112 < G (G >= 113), the tail
                        loop takes the rest (G = 113, 129, 200, 300: both; 128, 256: unrolled only for lanes 0 ..; <= 112: tail only);
                        LN_RED_MAX = 48 instances a launch: n = 49 and 97 take a second and a third launch.
  vitae_colsum_accum    256 columns x 32 rows a workgroup: N = 255, 256, 257 and M = 31, 32, 33, 65.
  vitae_bn1d_relu_fwd / _bwd   64 columns a workgroup (D = 60, 64, 68, 100: partial, full, 1 + partial), 16 row groups, the forward's
                        statistics 4x unrolled while r + 48 < R (R >= 64 for row group 15), the backward 2x: R = 2, 15 leave row
                        groups without a row, 16 / 17 / 63 / 64 / 65 / 130 walk the remainder and the unrolled loops.
  vitae_bn1d_relu_*_split   ``bn_split_plan`` below restates the launcher's plan: (R, D) = (2, 4) one split; (100, 64) four even
                        splits; (97, 64) an uneven last; (1000, 4) a last split of 8 rows < 16 row groups; (12289, 4) RS = 373 < rs = 384.

Every output lives in a buffer with >= 64 sentinel elements (one extra row for matrices) behind it that no launch may touch;
partial-record and workspace buffers start as NaN so that an element nobody wrote shows.  Every GPU case prints ``RATIO`` lines
(run with -s); LABNOTES.md keeps the table."""
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

EPS_LN, EPS_BN = 1e-6, 1e-5
GUARD, SENT = 64, 7.25           # SENT is exact in bf16
FACTOR, FLOOR = 3.0, 4.0 * 2.0 ** -24
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
LN_FAMILIES = ['plain', 'offset', 'tiny', 'scales', 'const', 'outlier']
BN_FAMILIES = ['plain', 'offset', 'tiny', 'scales', 'const', 'outlier', 'ramp']
# what e32 itself may be (CPU sanity check of references and inputs): values of size 1000 (1e4) in units of a deviation of 1 round
# at 1000 x 2^-24 = 6e-5 (6e-4) each, and torch's one-pass CPU statistics lose a little more; on a constant row (rstd = eps^-1/2 =
# 1000) torch's LayerNorm backward carries a mean one ulp off into d(gamma): 1.5e-4 where the two-pass formula has 1e-7
E32_SANE = dict({f: 1e-4 for f in BN_FAMILIES}, offset=5e-3, outlier=5e-3, const=1e-3)


def f32(x):
    return float(np.float32(x))


# =========================================================================== references (any dtype; float64 is THE reference)
def ln_fwd_ref(x, w, b, eps, dt):
    x, w, b = x.to(dt), w.to(dt), b.to(dt)
    mean = x.mean(1, keepdim=True)
    d = x - mean
    rstd = ((d * d).mean(1, keepdim=True) + eps).rsqrt()
    return d * rstd * w + b, mean[:, 0], rstd[:, 0]


def ln_bwd_ref(dy, x, w, mean, rstd, dt, base=None):
    """-> dx (+ base), the addends of dw, the addends of db"""
    dy, x, w, mean, rstd = dy.to(dt), x.to(dt), w.to(dt), mean.to(dt)[:, None], rstd.to(dt)[:, None]
    xh = (x - mean) * rstd
    g = dy * w
    dx = rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    if base is not None:
        dx = dx + base.to(dt)
    return dx, dy * xh, dy


def bn_fwd_ref(x, w, b, eps, dt):
    """-> y, mean, rstd, unbiased variance"""
    x, w, b = x.to(dt), w.to(dt), b.to(dt)
    R = x.shape[0]
    mean = x.mean(0)
    d = x - mean
    q = (d * d).sum(0)
    rstd = (q / R + eps).rsqrt()
    return (d * (rstd * w) + b).clamp_min(0), mean, rstd, q / max(R - 1, 1)


def bn_bwd_ref(dy, x, y_given, w, mean, rstd, dt):
    """-> dx, the addends of dw, the addends of db; the mask is y_given > 0"""
    dy, x, w, mean, rstd = dy.to(dt), x.to(dt), w.to(dt), mean.to(dt), rstd.to(dt)
    R = x.shape[0]
    g = dy * (y_given > 0).to(dt)
    xh = (x - mean) * rstd
    dx = w * rstd * (g - g.sum(0) / R - xh * ((g * xh).sum(0) / R))
    return dx, g * xh, g


def bn_eval_ref(x, w, b, rm, rv, eps, dt):
    x, w, b, rm, rv = (t.to(dt) for t in (x, w, b, rm, rv))
    return ((x - rm) * (rv + eps).rsqrt() * w + b).clamp_min(0)


def running_ref(r0, stat, mom, dt):
    """-> new running statistic, the sum of its absolute addends"""
    r0, stat = r0.to(dt), stat.to(dt)
    m = torch.tensor(mom, dtype=dt)
    return (1 - m) * r0 + m * stat, (1 - m) * r0.abs() + m * stat.abs()


def bn_split_plan(R, D):
    """The launcher's row-split plan: -> (RS, rows per split, rs before the rounding)."""
    cdiv = lambda a, b: (a + b - 1) // b
    rs = max(1, min(cdiv(384, cdiv(D, 64)), cdiv(R, 32)))
    rps = cdiv(R, rs)
    return cdiv(R, rps), rps, rs


# =========================================================================== torch's own fp32 ops (the other half of e32)
def torch_ln_fwd(x, w, b, eps):
    var, mean = torch.var_mean(x, 1, unbiased=False)
    return F.layer_norm(x, (x.shape[1],), w, b, eps), mean, (var + eps).rsqrt()


def torch_ln_bwd(dy, x, w, eps, base=None):
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), torch.zeros_like(w).requires_grad_(True)
    F.layer_norm(xr, (x.shape[1],), wr, br, eps).backward(dy)
    return (xr.grad if base is None else xr.grad + base), wr.grad, br.grad


def torch_bn_fwd(x, w, b, eps, rm=None, rv=None, mom=0.1):
    rm, rv = (None, None) if rm is None else (rm.clone(), rv.clone())
    y = F.relu(F.batch_norm(x, rm, rv, w, b, True, mom, eps))
    var, mean = torch.var_mean(x, 0, unbiased=False)
    return y, mean, (var + eps).rsqrt(), rm, rv


def torch_bn_bwd(g, x, w, eps):
    """autograd through torch's fp32 batch_norm fed the masked gradient g (the mask is the caller's: the kernel's contract)"""
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), torch.zeros_like(w).requires_grad_(True)
    F.batch_norm(xr, None, None, wr, br, True, 0.1, eps).backward(g)
    return xr.grad, wr.grad, br.grad


# =========================================================================== metrics
def seq_sum(t, i0=None):
    """A column sum the way the kernels' formula states it, `out[c] += t[m, c]` row after row, out starting as i0: the running
    fp32 sum from what the target held (torch's own ops keep torch's pairwise order and add i0 last)."""
    acc = torch.zeros_like(t[0]) if i0 is None else i0.to(t.dtype).clone()
    for row in t:                       # a loop on purpose: torch.cumsum accumulates fp32 in double on the CPU
        acc = acc + row
    return acc


def _ratio(num, den):
    """num / den with 0 / 0 = 0 and x / 0 = inf"""
    inf, zero = torch.full_like(num, float('inf')), torch.zeros_like(num)
    return torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num == 0, zero, inf))


def _cpu64(a):
    return a.detach().double().cpu()


def row_err(a, ref, scale=None):
    """[M, D]: worst row of max_c |a - ref| / scale_row (default max_c |ref|)"""
    a, ref = _cpu64(a), _cpu64(ref)
    return float(_ratio((a - ref).abs().amax(1), ref.abs().amax(1) if scale is None else _cpu64(scale)).max())


def col_err(a, ref, scale=None):
    """[R, D]: worst column of max_r |a - ref| / scale_col (default max_r |ref|, absolute where that is zero)"""
    a, ref = _cpu64(a), _cpu64(ref)
    if scale is None:
        scale = ref.abs().amax(0)
        scale = torch.where(scale > 0, scale, torch.ones_like(scale))
    return float(_ratio((a - ref).abs().amax(0), _cpu64(scale)).max())


def vec_err(a, ref, scale=None):
    """element-wise |a - ref| / scale (default |ref|), the worst element"""
    a, ref = _cpu64(a), _cpu64(ref)
    return float(_ratio((a - ref).abs(), ref.abs() if scale is None else _cpu64(scale)).max())


def within(label, e, *e32s):
    """The bound of this file; prints the RATIO line."""
    e32 = max(e32s)
    r = e / e32 if e32 > 0 else (0.0 if e == 0 else float('inf'))
    print(f'RATIO {label}: e={e:.3e} e32={e32:.3e} ratio={r:.2f}')
    assert e <= max(FACTOR * e32, FLOOR), (label, e, e32)
    return r


# =========================================================================== inputs
def ln_family(fam, M, D, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(M, D, generator=g)
    r = torch.arange(M)
    if fam == 'plain':
        x = z * 2 + 0.3
    elif fam == 'offset':
        x = z + (1000.0 * (1 - 2 * (r % 2)).float())[:, None]
    elif fam == 'tiny':
        x = z * 1e-4
    elif fam == 'scales':
        x = z * (10.0 ** (torch.rand(M, generator=g) * 6 - 3))[:, None]
    elif fam == 'const':
        x = z * 2 + 0.3
        x[::3] = ln_const_values(M)[::3, None]
    elif fam == 'outlier':
        x = z.clone()
        x[r, (r * 7) % D] = 1e4
    else:
        raise ValueError(fam)
    return x.float().contiguous()


def ln_const_values(M):
    """the constant of row r (rows 0, 3, 6, .. of the const family): an integer in -3 .. 3, D |c| < 2^24 for every D <= 1024"""
    return ((torch.arange(M) // 3) % 7 - 3).float()


def ln_params(D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(D, generator=g) + 1.0, torch.randn(D, generator=g)


def bn_family(fam, R, D, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(R, D, generator=g)
    c = torch.arange(D)
    x = z * 2 + 0.5
    if fam == 'plain':
        pass
    elif fam == 'offset':
        x = z + 1000.0 * (1 - 2 * (c % 2)).float()
    elif fam == 'tiny':
        x[:, 0] = 0.5 + 1e-3 * z[:, 0]
    elif fam == 'scales':
        x = z * 10.0 ** (torch.rand(D, generator=g) * 6 - 3)
    elif fam == 'const':
        x[:, 0], x[:, 1] = 3.0, -2.0
    elif fam == 'outlier':
        x = z.clone()
        x[(c[::4] * 5) % R, c[::4]] = 1e4
    elif fam == 'ramp':
        x[:, 0] = 0.25 * torch.arange(R).float()
    else:
        raise ValueError(fam)
    return x.float().contiguous()


def bn_params(fam, D, seed, bias=None):
    """weight N(1, 1), bias 0.1 N(0, 1); const: column 0 has bias EXACTLY 0, column 1 a bias of 0.75; bias=: every bias that value"""
    g = torch.Generator().manual_seed(seed)
    w, b = torch.randn(D, generator=g) + 1.0, torch.randn(D, generator=g) * 0.1
    if fam == 'const':
        b[0], b[1] = 0.0, 0.75
    if bias is not None:
        b[:] = bias
    return w, b


def int_grad(shape, seed, lim=8):
    """integer-valued gradient in -lim .. lim: any sum of fewer than 2^24 / lim of them is exact in fp32 in any order"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


def real_grad(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# =========================================================================== CPU tests: references, inputs, e32
def test_references_are_float64_autograd():
    """The hand-written float64 forms against float64 F.layer_norm / nn.BatchNorm1d autograd on plain inputs: 1e-12."""
    close = lambda a, b: float((a - b).detach().abs().max()) <= 1e-12 * float(b.detach().abs().max())
    for M, D in ((33, 48), (9, 768), (5, 1000), (3, 1)):
        x, (w, b), dy = ln_family('plain', M, D, 1).double(), [t.double() for t in ln_params(D, 2)], real_grad((M, D), 3).double()
        xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        ref = F.layer_norm(xr, (D,), wr, br, EPS_LN)
        ref.backward(dy)
        y, mean, rstd = ln_fwd_ref(x, w, b, EPS_LN, F64)
        dx, tw, tb = ln_bwd_ref(dy, x, w, mean, rstd, F64)
        assert close(y, ref) and close(tb.sum(0), br.grad) and close(tw.sum(0), wr.grad)
        assert float((dx - xr.grad).abs().max()) <= 1e-12 * float((rstd[:, None] * (dy * w).abs()).max())
    for R, D in ((130, 100), (17, 4), (2, 8)):
        for mom in (0.1, 0.3):
            x, dy = bn_family('plain', R, D, 4).double(), real_grad((R, D), 5).double()
            w, b = [t.double() for t in bn_params('plain', D, 6)]
            bn = torch.nn.BatchNorm1d(D, eps=EPS_BN, momentum=mom).double()
            rm0, rv0 = torch.randn(D, dtype=F64), torch.rand(D, dtype=F64) + 0.5
            with torch.no_grad():
                bn.weight.copy_(w); bn.bias.copy_(b); bn.running_mean.copy_(rm0); bn.running_var.copy_(rv0)
            xr = x.clone().requires_grad_(True)
            ref = F.relu(bn(xr))
            ref.backward(dy)
            y, mean, rstd, uvar = bn_fwd_ref(x, w, b, EPS_BN, F64)
            dx, tw, tb = bn_bwd_ref(dy, x, y, w, mean, rstd, F64)
            assert close(y, ref) and close(dx, xr.grad) and close(tw.sum(0), bn.weight.grad) and close(tb.sum(0), bn.bias.grad)
            assert close(running_ref(rm0, mean, mom, F64)[0], bn.running_mean) and close(running_ref(rv0, uvar, mom, F64)[0], bn.running_var)
            bn.eval()
            assert close(bn_eval_ref(x, w, b, bn.running_mean, bn.running_var, EPS_BN, F64), F.relu(bn(x)))


def test_float64_batchnorm_module_is_no_reference_at_relus_edge():
    """A constant column with zero bias: the hand-written reference gives exactly 0 before the ReLU whatever the weight; that is
    what the kernels are held to (nn.BatchNorm1d(...).double() was seen to leave round-off noise of either sign there)."""
    x, (w, b) = bn_family('const', 130, 8, 1), bn_params('const', 8, 2)
    y, mean, rstd, uvar = bn_fwd_ref(x, w, b, f32(EPS_BN), F64)
    assert float(mean[0]) == 3.0 and float(mean[1]) == -2.0 and float(uvar[0]) == 0.0
    assert bool((y[:, 0] == 0).all()) and bool((y[:, 1] == 0.75).all())
    dx, tw, tb = bn_bwd_ref(real_grad((130, 8), 3), x, y, w, mean, rstd, F64)
    assert bool((dx[:, 0] == 0).all()) and bool((tw[:, 0] == 0).all()) and bool((tb[:, 0] == 0).all())


def test_input_families_have_the_claimed_properties():
    M, D = 33, 768
    for fam in LN_FAMILIES:
        x = ln_family(fam, M, D, 7).double()
        mean, std = x.mean(1), x.std(1, unbiased=False)
        if fam == 'plain':
            assert abs(float(mean.mean()) - 0.3) < 0.1 and abs(float(std.mean()) - 2.0) < 0.1
        elif fam == 'offset':
            assert bool(((mean.abs() - 1000).abs() < 0.5).all()) and bool((mean[::2] > 0).all()) and bool((mean[1::2] < 0).all())
            assert bool(((std - 1).abs() < 0.2).all())
        elif fam == 'tiny':
            assert bool((std ** 2 < 0.02 * EPS_LN).all()) and bool((std > 0).all())
        elif fam == 'scales':
            assert float(std.max() / std.min()) > 1e4 and float(std.min()) > 5e-4 and float(std.max()) < 2e3
        elif fam == 'const':
            c = ln_const_values(M).double()
            assert bool((x[::3] == c[::3, None]).all()) and float(c.abs().max()) * 1024 < 2 ** 24 and bool((std[1::3] > 1).all())
            assert len(set(c[::3].tolist())) > 3 and 0.0 in c[::3].tolist()
        elif fam == 'outlier':
            assert bool(((x == 1e4).sum(1) == 1).all()) and bool((x.abs().amax(1) == 1e4).all())
    R, D = 130, 64
    for fam in BN_FAMILIES:
        x = bn_family(fam, R, D, 7).double()
        mean, std = x.mean(0), x.std(0, unbiased=False)
        if fam == 'offset':
            assert bool(((mean.abs() - 1000).abs() < 0.5).all()) and bool((mean[::2] > 0).all()) and bool((mean[1::2] < 0).all())
        elif fam == 'tiny':
            assert 0.2 * EPS_BN > float(std[0]) ** 2 > 0.02 * EPS_BN and bool((std[1:] > 1).all())
        elif fam == 'scales':
            assert float(std.max() / std.min()) > 1e3
        elif fam == 'const':
            assert bool((x[:, 0] == 3).all()) and bool((x[:, 1] == -2).all()) and 3 * 12289 < 2 ** 24
            w, b = bn_params('const', D, 1)
            assert float(b[0]) == 0.0 and float(b[1]) == 0.75
        elif fam == 'outlier':
            assert int((x == 1e4).sum()) == D // 4 and bool(((x == 1e4).sum(0) <= 1).all())
        elif fam == 'ramp':
            # four splits of 25 rows: the split means are 6.25 apart, the deviation inside a split is 1.8
            xs = bn_family(fam, 100, D, 7).double()[:, 0].view(4, 25)
            between = float((25 * (xs.mean(1) - xs.mean()) ** 2).sum())
            inside = float(((xs - xs.mean(1, keepdim=True)) ** 2).sum())
            assert between > 10 * inside
    g = int_grad((6145, 8), 1)
    assert bool((g == g.round()).all()) and float(g.abs().max()) == 8 and 8 * 12289 * 2 < 2 ** 24


def test_split_plans_of_the_tested_shapes():
    """The (R, D) of the split tests reach what the module docstring says."""
    assert bn_split_plan(2, 4)[0] == 1
    RS, rps, _ = bn_split_plan(100, 64)
    assert (RS, rps) == (4, 25)
    RS, rps, _ = bn_split_plan(97, 64)
    assert RS == 4 and 97 - 3 * rps == 22 != rps
    RS, rps, _ = bn_split_plan(1000, 4)
    assert RS > 1 and 0 < 1000 - (RS - 1) * rps < 16
    RS, rps, rs = bn_split_plan(12289, 4)
    assert rs == 384 and RS == 373 < rs
    RS, rps, rs = bn_split_plan(1760, 768)          # the predictor at batch 32
    assert RS == rs == 32 and rps == 55
    cdiv = lambda a, b: (a + b - 1) // b
    assert cdiv(1027, 8) == 129 > 128 and cdiv(1027, 4) > 256          # layernorm_bwd: both grid-stride loops
    for M, groups in ((2047, 1), (2049, 2), (4097, 3), (6145, 4)):     # layernorm_bwd_part: row groups of workgroup 0
        G = min(cdiv(M, 8), 256)
        assert len(range(0, cdiv(M, 8), G)) == groups


def _ln_e32(fam, M, D, seed=11):
    x, (w, b), dy = ln_family(fam, M, D, seed), ln_params(D, seed + 1), real_grad((M, D), seed + 2)
    eps = f32(EPS_LN)
    y64, m64, r64 = ln_fwd_ref(x, w, b, eps, F64)
    std64 = x.double().std(1, unbiased=False)
    fwd = {}
    for name, (y, m, r) in (('torch', torch_ln_fwd(x, w, b, eps)), ('formula', ln_fwd_ref(x, w, b, eps, F32))):
        fwd[name] = (row_err(y, y64), vec_err(m, m64, m64.abs() + std64), vec_err(r, r64), y, m, r)
    dx64, tw64, tb64 = ln_bwd_ref(dy, x, w, m64, r64, F64)
    sc = r64 * (dy.double() * w.double()).abs().amax(1)
    _, m32, r32 = ln_fwd_ref(x, w, b, eps, F32)
    dxf, twf, tbf = ln_bwd_ref(dy, x, w, m32, r32, F32)
    dxt, dwt, dbt = torch_ln_bwd(dy, x, w, eps)
    bwd = {'torch': (row_err(dxt, dx64, sc), vec_err(dwt, tw64.sum(0), tw64.abs().sum(0)), vec_err(dbt, tb64.sum(0), tb64.abs().sum(0))),
           'formula': (row_err(dxf, dx64, sc), vec_err(seq_sum(twf), tw64.sum(0), tw64.abs().sum(0)), vec_err(seq_sum(tbf), tb64.sum(0), tb64.abs().sum(0)))}
    return x, w, b, fwd, bwd


@pytest.mark.parametrize('fam', LN_FAMILIES)
def test_layernorm_e32_of_every_family(fam):
    """e32 itself, printed, for the LayerNorm metrics; both fp32 statements stay within a few 1e-6 of float64 in these units, and
    on the const family the fp32 formula meets the exact assertions the kernels are held to."""
    for M, D in ((33, 48), (33, 768), (9, 1000)):
        x, w, b, fwd, bwd = _ln_e32(fam, M, D)
        for name in ('torch', 'formula'):
            ey, em, er = fwd[name][:3]
            ex, ew, eb = bwd[name]
            print(f'E32 layernorm {fam} M={M} D={D} {name}: y={ey:.2e} mean={em:.2e} rstd={er:.2e} dx={ex:.2e} dw={ew:.2e} db={eb:.2e}')
            assert max(ey, em, er, ex, ew, eb) < E32_SANE[fam]
        if fam == 'const':
            _, _, _, y, m, r = fwd['formula']
            assert torch.equal(m[::3], ln_const_values(M)[::3]) and torch.equal(y[::3], b.expand(M, D)[::3])


def _bn_e32(fam, R, D, seed=21):
    x, (w, b), dy = bn_family(fam, R, D, seed), bn_params(fam, D, seed + 1), real_grad((R, D), seed + 2)
    eps = f32(EPS_BN)
    y64, m64, r64, u64 = bn_fwd_ref(x, w, b, eps, F64)
    std64 = x.double().std(0, unbiased=False)
    out = {}
    yt, mt, rt, _, _ = torch_bn_fwd(x, w, b, eps)
    yf, mf, rf, uf = bn_fwd_ref(x, w, b, eps, F32)
    for name, (y, m, r) in (('torch', (yt, mt, rt)), ('formula', (yf, mf, rf))):
        g = dy * (y > 0)
        dx64, tw64, tb64 = bn_bwd_ref(dy, x, y, w, m64, r64, F64)
        sc = w.double().abs() * r64 * g.double().abs().amax(0)
        if name == 'torch':
            dx, dw, db = torch_bn_bwd(g, x, w, eps)
        else:
            dx, tw, tb = bn_bwd_ref(dy, x, y, w, m, r, F32)
            dw, db = seq_sum(tw), seq_sum(tb)
        out[name] = (col_err(y, y64), vec_err(m, m64, m64.abs() + std64), vec_err(r, r64), col_err(dx, dx64, sc),
                     vec_err(dw, tw64.sum(0), tw64.abs().sum(0)), vec_err(db, tb64.sum(0), tb64.abs().sum(0)))
    return x, w, b, dy, out, (yf, mf, rf)


@pytest.mark.parametrize('fam', BN_FAMILIES)
def test_batchnorm_e32_of_every_family(fam):
    for R, D in ((2, 4), (17, 60), (130, 64), (1000, 4)):
        x, w, b, dy, out, (yf, mf, rf) = _bn_e32(fam, R, D)
        for name in ('torch', 'formula'):
            print(f'E32 batchnorm {fam} R={R} D={D} {name}: ' + ' '.join(f'{k}={v:.2e}' for k, v in zip(('y', 'mean', 'rstd', 'dx', 'dw', 'db'), out[name])))
            assert max(out[name]) < E32_SANE[fam]
        if fam == 'const':
            assert float(mf[0]) == 3.0 and float(mf[1]) == -2.0 and bool((yf[:, 0] == 0).all()) and bool((yf[:, 1] == 0.75).all())
            dx, tw, tb = bn_bwd_ref(dy, x, yf, w, mf, rf, F32)
            assert bool((dx[:, 0] == 0).all()) and float(tw.sum(0)[0]) == 0.0 and float(tb.sum(0)[0]) == 0.0


def test_integer_sums_are_exact_in_fp32_in_any_order():
    g = int_grad((6145, 16), 5)
    want = g.double().sum(0)
    perm = torch.randperm(6145, generator=torch.Generator().manual_seed(1))
    for s in (g.sum(0), g[perm].sum(0), g.flip(0).cumsum(0)[-1], g.view(5, 1229, 16).sum(1).sum(0)):
        assert torch.equal(s.double(), want)


# =========================================================================== launches (GPU)
gpu = pytest.mark.gpu
NS = types.SimpleNamespace


@pytest.fixture(scope='module')
def lib():
    from vit_ae_plus_plus_amd._abi import lib as L
    L.load()
    return L


@pytest.fixture(scope='module')
def VitaeError():
    from vit_ae_plus_plus_amd._abi import VitaeError as E
    return E


def st():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


class Buf:
    """A device array of `shape` inside a flat buffer with `off` sentinel elements in front of it (off = 1 takes a fresh 512-byte
    aligned allocation one element off) and max(GUARD, one row) sentinel elements behind.  The array starts as `init`, else as
    `inner` everywhere (the sentinel; NaN for records and workspaces)."""

    def __init__(self, shape, init=None, dtype=F32, inner=None, off=0, keep=False):
        shape = tuple(shape)
        n = int(np.prod(shape))
        self.sent = SENT if dtype.is_floating_point else 7
        buf = torch.full((off + n + max(GUARD, shape[-1]),), self.sent, dtype=dtype)
        if init is not None:
            buf[off:off + n] = init.reshape(-1).to(dtype)
        elif inner is not None:
            buf[off:off + n] = inner
        self.orig = buf.clone() if keep else None
        self.buf, self.n, self.off = buf.cuda(), n, off
        self.t = self.buf[off:off + n].view(shape)
        self.ptr = self.t.data_ptr()
        assert self.buf.data_ptr() % 16 == 0

    def intact(self):
        return bool((self.buf[:self.off] == self.sent).all()) and bool((self.buf[self.off + self.n:] == self.sent).all())

    def untouched(self):
        return torch.equal(_bits(self.buf).cpu(), _bits(self.orig))


def ptr(b):
    return None if b is None else b.ptr


def all_intact(*bufs):
    torch.cuda.synchronize()
    return all(b is None or b.intact() for b in bufs)


_CACHE = {}


@pytest.fixture(scope='module', autouse=True)
def _drop_case_cache():
    yield
    _CACHE.clear()


def ln_case(fam, M, D):
    """Inputs and the forward references of one (family, M, D), computed once and shared (read-only) by the tests that need them."""
    key = ('ln', fam, M, D)
    if key in _CACHE:
        return _CACHE[key]
    seed = 1000 + 7 * M + D
    x, (w, b), eps = ln_family(fam, M, D, seed), ln_params(D, seed + 1), f32(EPS_LN)
    c = NS(fam=fam, M=M, D=D, x=x, w=w, b=b, ref=ln_fwd_ref(x, w, b, eps, F64), t32=torch_ln_fwd(x, w, b, eps),
           f32=ln_fwd_ref(x, w, b, eps, F32), std64=x.double().std(1, unbiased=False))
    if M * D <= 1 << 20:
        _CACHE[key] = c
    return c


# ---- LayerNorm forward
def ln_fwd_gpu(lib, c, want='both', off=(0, 0, 0)):
    M, D = c.M, c.D
    xd, wd, bd = Buf((M, D), c.x, off=off[0]), Buf((D,), c.w), Buf((D,), c.b)
    y = Buf((M, D), off=off[1]) if want in ('both', 'y') else None
    y16 = Buf((M, D), dtype=BF16, off=off[2]) if want in ('both', 'y16') else None
    mean, rstd = Buf((M,)), Buf((M,))
    lib.vitae_layernorm_fwd(xd.ptr, wd.ptr, bd.ptr, ptr(y), ptr(y16), mean.ptr, rstd.ptr, M, D, EPS_LN, st())
    assert all_intact(y, y16, mean, rstd)
    return NS(y=None if y is None else y.t, y16=None if y16 is None else y16.t, mean=mean.t, rstd=rstd.t)


def check_ln_fwd(label, c, out):
    y64, m64, r64 = c.ref
    within(f'{label} y', row_err(out.y, y64), row_err(c.t32[0], y64), row_err(c.f32[0], y64))
    sc = m64.abs() + c.std64
    within(f'{label} mean', vec_err(out.mean, m64, sc), vec_err(c.t32[1], m64, sc), vec_err(c.f32[1], m64, sc))
    within(f'{label} rstd', vec_err(out.rstd, r64), vec_err(c.t32[2], r64), vec_err(c.f32[2], r64))
    if c.fam == 'const':
        assert torch.equal(out.mean.cpu()[::3], ln_const_values(c.M)[::3])
        assert torch.equal(out.y.cpu()[::3], c.b.expand(c.M, c.D)[::3])


def ln_fwd_all_outputs(lib, label, c, off=(0, 0, 0), alone=('y', 'y16')):
    """y and y_bf16, then each alone: the fp32 output within the bound, the bf16 one its bitwise rounding, the same bits (statistics
    included) from every combination; statistics asserted against float64."""
    both = ln_fwd_gpu(lib, c, 'both', off)
    check_ln_fwd(label, c, both)
    assert torch.equal(both.y16, both.y.to(BF16))
    for want in alone:
        o = ln_fwd_gpu(lib, c, want, off)
        assert torch.equal(_bits(getattr(o, want)), _bits(getattr(both, want))), want
        assert torch.equal(o.mean, both.mean) and torch.equal(o.rstd, both.rstd), want
    return both


LN_VEC_D, LN_SCALAR_D = [256, 512, 768, 1024], [1, 2, 63, 64, 65, 100, 700, 769, 1000, 1023]


@gpu
@pytest.mark.parametrize('fam', LN_FAMILIES)
@pytest.mark.parametrize('D', LN_VEC_D + LN_SCALAR_D)
def test_layernorm_fwd(lib, D, fam):
    for M in (1, 5, 33):
        ln_fwd_all_outputs(lib, f'layernorm_fwd {"vec" if D in LN_VEC_D else "scalar"} {fam} M={M} D={D}', ln_case(fam, M, D))


@gpu
@pytest.mark.parametrize('fam', ['plain', 'offset', 'const'])
@pytest.mark.parametrize('which', ['x', 'y', 'y16'])
@pytest.mark.parametrize('D', [768, 256])
def test_layernorm_fwd_unaligned_operands_take_the_scalar_kernel(lib, D, which, fam):
    """x or y one float off 16 bytes, y_bf16 one element off 8: same contract, nothing written in front of or behind the arrays."""
    off = {'x': (1, 0, 0), 'y': (0, 1, 0), 'y16': (0, 0, 1)}[which]
    alone = ('y', 'y16') if which == 'x' else (which,)         # a call without the unaligned output is the vector kernel's business
    ln_fwd_all_outputs(lib, f'layernorm_fwd unaligned-{which} {fam} M=5 D={D}', ln_case(fam, 5, D), off, alone)


# ---- LayerNorm backward
def reduce_gpu(lib, parts, dws, dbs, css, Gs, Ds):
    """vitae_ln_grad_reduce on lists of Buf (css: a list that may hold None, or None for a NULL array)"""
    u64 = lambda v: np.array(v, dtype=np.uint64)
    a_p, a_w, a_b = u64([p.ptr for p in parts]), u64([t.ptr for t in dws]), u64([t.ptr for t in dbs])
    a_c = None if css is None else u64([0 if t is None else t.ptr for t in css])
    a_g, a_d = np.array(Gs, dtype=np.int32), np.array(Ds, dtype=np.int32)
    lib.vitae_ln_grad_reduce(len(parts), a_p.ctypes.data, a_w.ctypes.data, a_b.ctypes.data, None if a_c is None else a_c.ctypes.data,
                             a_g.ctypes.data, a_d.ctypes.data, st())


def ln_bwd_gpu(lib, entry, c, dy, mean, rstd, base, accum, want16, want_cs, init, off=None):
    """entry 'bwd': vitae_layernorm_bwd; 'part': vitae_layernorm_bwd_part + vitae_ln_grad_reduce of its records (without a
    column-sum target the reduce gets a NULL dx_colsum ARRAY).  mean / rstd: fp32 tensors (CPU or device)."""
    M, D = c.M, c.D
    off = off or {}
    dyd, xd, wd = Buf((M, D), dy, off=off.get('dy', 0)), Buf((M, D), c.x, off=off.get('x', 0)), Buf((D,), c.w)
    md, rd = Buf((M,), mean), Buf((M,), rstd)
    dx = Buf((M, D), base if accum else None, off=off.get('dx', 0))
    dx16 = Buf((M, D), dtype=BF16, off=off.get('dx16', 0)) if want16 else None
    dw, db, cs = Buf((D,), init[0]), Buf((D,), init[1]), (Buf((D,), init[2]) if want_cs else None)
    part = None
    if entry == 'bwd':
        lib.vitae_layernorm_bwd(dyd.ptr, xd.ptr, wd.ptr, md.ptr, rd.ptr, dx.ptr, dw.ptr, db.ptr, ptr(dx16), ptr(cs), M, D, accum, st())
    else:
        G = lib.vitae_layernorm_bwd_part_records(M)
        assert G == min((M + 7) // 8, 256)
        part = Buf((G, 3 * D), inner=float('nan'))
        lib.vitae_layernorm_bwd_part(dyd.ptr, xd.ptr, wd.ptr, md.ptr, rd.ptr, dx.ptr, part.ptr, ptr(dx16), M, D, accum, st())
        reduce_gpu(lib, [part], [dw], [db], [cs] if want_cs else None, [G], [D])
    assert all_intact(dx, dx16, dw, db, cs, part)
    assert part is None or not bool(torch.isnan(part.t).any())            # every element of every record was written
    return NS(dx=dx.t, dx16=None if dx16 is None else dx16.t, dw=dw.t, db=db.t, cs=None if cs is None else cs.t,
              part=None if part is None else part.t)


def ln_bwd_init(D, seed):
    """what dw / db / dx_colsum hold before the launch (they receive +=): db's start is a non-zero integer (db stays exact under an
    integer dy)"""
    g = torch.Generator().manual_seed(seed)
    i = torch.randint(1, 6, (D,), generator=g).float() * (1 - 2 * torch.randint(0, 2, (D,), generator=g)).float()
    return torch.randn(D, generator=g) * 0.5, i, torch.randn(D, generator=g) * 0.5


def ln_dx_scale(c, dy):
    return c.ref[2] * (dy.double() * c.w.double()).abs().amax(1)


def check_ln_bwd(label, c, dy, out, base, accum, init, stats=None, int_dy=False):
    """stats None: the kernel was fed the forward kernel's statistics, the reference runs end to end from x; else the fp32 (mean,
    rstd) it was fed, which the reference and the fp32 formula use too (torch's own op is measured against the true result)."""
    eps, x, w = f32(EPS_LN), c.x, c.w
    b_ = base if accum else None
    true = ln_bwd_ref(dy, x, w, c.ref[1], c.ref[2], F64, b_)
    ref = true if stats is None else ln_bwd_ref(dy, x, w, stats[0], stats[1], F64, b_)
    m32, r32 = (c.f32[1], c.f32[2]) if stats is None else stats
    fm = ln_bwd_ref(dy, x, w, m32, r32, F32, b_)
    tc = torch_ln_bwd(dy, x, w, eps, b_)
    sc = ln_dx_scale(c, dy)
    assert bool(torch.isfinite(out.dx).all())
    within(f'{label} dx', row_err(out.dx, ref[0], sc), row_err(tc[0], true[0], sc), row_err(fm[0], ref[0], sc))
    sums = [('dw', out.dw, init[0], ref[1], true[1], tc[1], fm[1]), ('db', out.db, init[1], ref[2], true[2], tc[2], fm[2])]
    if out.cs is not None:
        sums.append(('dx_colsum', out.cs, init[2], ref[0], true[0], tc[0].sum(0), fm[0]))
    for name, got, i0, terms, terms_true, s_torch, t_formula in sums:
        want, scale = i0.double() + terms.sum(0), i0.double().abs() + terms.abs().sum(0)
        want_t, scale_t = i0.double() + terms_true.sum(0), i0.double().abs() + terms_true.abs().sum(0)
        within(f'{label} {name}', vec_err(got, want, scale), vec_err(i0 + s_torch, want_t, scale_t), vec_err(seq_sum(t_formula, i0), want, scale))
    if out.dx16 is not None:
        assert torch.equal(out.dx16, out.dx.to(BF16))
    if int_dy:
        assert torch.equal(out.db.cpu(), init[1] + dy.sum(0)), label


def ln_bwd_both_ways(lib, entry, label, c, k, off=None, isolated=True):
    """One shape through `entry` twice: 'chain' (statistics from the forward kernel, an integer dy, so db is exact) and 'isolated'
    (float64 statistics rounded to fp32, a normal dy).  k picks the options: bit 0 dx_accumulate, bit 1 dx_bf16, bit 2 dx_colsum."""
    M, D = c.M, c.D
    init = ln_bwd_init(D, 5 * M + D)
    fwd = ln_fwd_gpu(lib, c)
    for mode in ('chain', 'isolated') if isolated else ('chain',):
        accum, want16, want_cs = k & 1, ((k >> 1) & 1) | int(bool(off) and 'dx16' in off), (k >> 2) & 1
        dy = int_grad((M, D), 3 * M + D) if mode == 'chain' else real_grad((M, D), 3 * M + D)
        base = (real_grad((M, D), M + D) * ln_dx_scale(c, dy)[:, None]).float()
        stats = None if mode == 'chain' else (c.ref[1].float(), c.ref[2].float())
        mean, rstd = (fwd.mean, fwd.rstd) if stats is None else stats
        out = ln_bwd_gpu(lib, entry, c, dy, mean, rstd, base, accum, want16, want_cs, init, off)
        check_ln_bwd(f'{label} {mode} opts={k & 7}', c, dy, out, base, accum, init, stats, int_dy=(mode == 'chain'))
        k += 3
    return k


LN_BWD_PATHS = [('rows_vec', d, (1, 9, 33)) for d in (256, 512, 768)] + [('rows', d, (1, 7, 8, 9, 33)) for d in (1, 2, 63, 64, 65, 100, 700, 767)] \
    + [('generic', d, (7,)) for d in (769, 1000, 1024)]


@gpu
@pytest.mark.parametrize('fam', LN_FAMILIES)
@pytest.mark.parametrize('path,D,Ms', LN_BWD_PATHS)
def test_layernorm_bwd(lib, path, D, Ms, fam):
    """With one row a column's d(gamma) is the single product dy xhat: nothing averages over the error of the saved mean, so the
    'chain' cases at M = 1 are the test of the forward kernel's mean (from an fp32 sum they were 3.1 - 3.7 x e32, LABNOTES.md)."""
    k = D + 3 * LN_FAMILIES.index(fam)
    for M in Ms:
        k = ln_bwd_both_ways(lib, 'bwd', f'layernorm_bwd {path} {fam} M={M} D={D}', ln_case(fam, M, D), k) + 1


@gpu
@pytest.mark.parametrize('fam', LN_FAMILIES)
@pytest.mark.parametrize('path,D', [('rows_vec', 256), ('rows_vec', 512), ('rows_vec', 768), ('generic', 769), ('generic', 1000), ('generic', 1024)])
def test_layernorm_bwd_grid_stride(lib, path, D, fam):
    """M = 1027: 129 row groups on 128 workgroups (rows_vec), 1027 rows on 1024 waves (generic) — the loops take a second turn."""
    ln_bwd_both_ways(lib, 'bwd', f'layernorm_bwd {path}-stride {fam} M=1027 D={D}', ln_case(fam, 1027, D), D // 256 + LN_FAMILIES.index(fam))


@gpu
@pytest.mark.parametrize('fam', ['plain', 'offset', 'outlier'])
@pytest.mark.parametrize('which', ['dy', 'x', 'dx', 'dx16'])
@pytest.mark.parametrize('D', [768, 256])
def test_layernorm_bwd_unaligned_operands_take_the_rows_kernel(lib, D, which, fam):
    for M in (9, 33):
        k = 2 | (LN_FAMILIES.index(fam) + M + (D >> 8))           # dx_bf16 always asked for
        ln_bwd_both_ways(lib, 'bwd', f'layernorm_bwd rows-unaligned-{which} {fam} M={M} D={D}', ln_case(fam, M, D), k, off={which: 1})


@gpu
@pytest.mark.parametrize('k', range(8))
@pytest.mark.parametrize('entry,D', [('bwd', 768), ('bwd', 100), ('bwd', 1000), ('part', 256)])
def test_layernorm_bwd_every_option_on_every_kernel(lib, entry, D, k):
    """dx_accumulate x dx_bf16 x dx_colsum, all eight, on rows_vec, rows, the generic kernel and the partial-record form."""
    c = ln_case('scales', 9, D)
    init = ln_bwd_init(D, 77)
    fwd = ln_fwd_gpu(lib, c)
    dy = real_grad((9, D), 78)
    base = (real_grad((9, D), 79) * ln_dx_scale(c, dy)[:, None]).float()
    out = ln_bwd_gpu(lib, entry, c, dy, fwd.mean, fwd.rstd, base, k & 1, (k >> 1) & 1, (k >> 2) & 1, init)
    check_ln_bwd(f'layernorm_bwd{"_part" if entry == "part" else ""} options scales M=9 D={D} opts={k}', c, dy, out, base, k & 1, init)
    assert (out.dx16 is not None) == bool(k & 2) and (out.cs is not None) == bool(k & 4)


PART_SHAPES = [(D, M) for D in (256, 1024) for M in (1, 9, 2047, 2049, 4097, 6145)]


@gpu
@pytest.mark.parametrize('D,M', PART_SHAPES)
def test_layernorm_bwd_part(lib, D, M):
    """1, 2, 3 and 4 row groups per workgroup of the record form (families take turns over the shapes; all of them at M = 1, 9);
    the records fully written, nothing behind G 3 D floats; the reduce adds into non-zero targets; twice is bitwise the same."""
    i = PART_SHAPES.index((D, M))
    fams = LN_FAMILIES if M <= 9 else [LN_FAMILIES[(i * 5 + 1) % 6]]
    for fam in fams:
        c = ln_case(fam, M, D)
        ln_bwd_both_ways(lib, 'part', f'layernorm_bwd_part {fam} M={M} D={D}', c, i + LN_FAMILIES.index(fam), isolated=(M <= 2049))
    fwd = ln_fwd_gpu(lib, c)
    dy, init = real_grad((M, D), 9), ln_bwd_init(D, 10)
    base = real_grad((M, D), 11)
    a, b = (ln_bwd_gpu(lib, 'part', c, dy, fwd.mean, fwd.rstd, base, 1, 1, 1, init) for _ in range(2))
    for name in ('dx', 'dx16', 'dw', 'db', 'cs', 'part'):
        assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name


# ---- vitae_ln_grad_reduce on synthetic records
RED_D, RED_G = [4, 100, 256, 1024], [1, 15, 16, 17, 113, 128, 129, 200, 256, 300]


def _reduce_case(lib, Ds, Gs, integer, null_entries=(), null_array=False, seed=0):
    n = len(Ds)
    recs = [int_grad((G, 3 * D), seed + 31 * i, lim=4) if integer else real_grad((G, 3 * D), seed + 31 * i) for i, (D, G) in enumerate(zip(Ds, Gs))]
    mk = (lambda D, s: int_grad((D,), s, lim=5)) if integer else (lambda D, s: real_grad((D,), s))
    inits = [[mk(D, seed + 1000 + 3 * i + j) for j in range(3)] for i, D in enumerate(Ds)]
    parts = [Buf(r.shape, r) for r in recs]
    tg = [[Buf((D,), inits[i][j]) for j in range(3)] for i, D in enumerate(Ds)]
    css = None if null_array else [None if i in null_entries else tg[i][2] for i in range(n)]
    reduce_gpu(lib, parts, [t[0] for t in tg], [t[1] for t in tg], css, Gs, Ds)
    assert all_intact(*parts, *[b for t in tg for b in t])
    return recs, inits, tg, css


def _check_reduce_exact(recs, inits, tg, css, Ds):
    for i, D in enumerate(Ds):
        s = recs[i].sum(0)
        assert torch.equal(s.double(), recs[i].double().sum(0))                     # the host sum itself is exact
        for j in range(3):
            live = j < 2 or (css is not None and css[i] is not None)
            want = inits[i][j] + s[j * D:(j + 1) * D] if live else inits[i][j]
            assert torch.equal(tg[i][j].t.cpu(), want), (i, j, D)


@gpu
@pytest.mark.parametrize('D', RED_D)
def test_ln_grad_reduce_every_record_count(lib, D):
    """n = 1: tail loop only (G <= 112), both loops (113, 129, 200, 300), unrolled loop with no tail for some lanes (128, 256)."""
    for G in RED_G:
        recs, inits, tg, css = _reduce_case(lib, [D], [G], True, seed=G + D)
        _check_reduce_exact(recs, inits, tg, css, [D])


@gpu
@pytest.mark.parametrize('null_array', [False, True])
@pytest.mark.parametrize('n', [3, 49, 97])
def test_ln_grad_reduce_many_instances_mixed_widths(lib, n, null_array):
    """Mixed D in one call (the launch is as wide as the widest), 49 and 97 instances = 2 and 3 launches of <= 48, every third
    instance without a column-sum target, or no column-sum array at all."""
    Ds = [RED_D[(i + n) % 4] for i in range(n)]
    Gs = [RED_G[(3 * i + n) % 10] for i in range(n)]
    recs, inits, tg, css = _reduce_case(lib, Ds, Gs, True, null_entries=set(range(1, n, 3)), null_array=null_array, seed=n)
    _check_reduce_exact(recs, inits, tg, css, Ds)


@gpu
def test_ln_grad_reduce_real_records(lib):
    Ds, Gs = [100, 1024, 4, 256], [300, 113, 200, 129]
    outs = []
    for rep in range(2):
        recs, inits, tg, css = _reduce_case(lib, Ds, Gs, False, null_entries={2}, seed=5)
        outs.append([b.t.clone() for t in tg for b in t])
    for a, b in zip(*outs):
        assert torch.equal(_bits(a), _bits(b))                                       # fixed order: bitwise reproducible
    for i, D in enumerate(Ds):
        r = recs[i]
        for j, name in enumerate(('dw', 'db', 'dx_colsum')):
            i0, t = inits[i][j], r[:, j * D:(j + 1) * D]
            if j == 2 and i == 2:
                assert torch.equal(tg[i][j].t.cpu(), i0)
                continue
            want, scale = i0.double() + t.double().sum(0), i0.double().abs() + t.double().abs().sum(0)
            within(f'ln_grad_reduce real G={Gs[i]} D={D} {name}', vec_err(tg[i][j].t, want, scale), vec_err(i0 + t.sum(0), want, scale),
                   vec_err(seq_sum(t, i0), want, scale))


# ---- vitae_colsum_accum
@gpu
@pytest.mark.parametrize('integer', [True, False])
@pytest.mark.parametrize('N', [1, 255, 256, 257])
def test_colsum_accum(lib, N, integer):
    """ld = N + 3 > N with 1e6 in the padding columns, a non-zero target: exact under an integer dy, within the bound otherwise."""
    for M in (1, 31, 32, 33, 65):
        ld = N + 3
        dy = int_grad((M, N), M + N) if integer else real_grad((M, N), M + N)
        padded = torch.full((M, ld), 1e6)
        padded[:, :N] = dy
        i0 = int_grad((N,), M, lim=5) if integer else real_grad((N,), M)
        dyd, out = Buf((M, ld), padded), Buf((N,), i0)
        lib.vitae_colsum_accum(dyd.ptr, ld, out.ptr, M, N, st())
        assert all_intact(out)
        if integer:
            assert torch.equal(out.t.cpu(), i0 + dy.sum(0)), (M, N)
        else:
            want, scale = i0.double() + dy.double().sum(0), i0.double().abs() + dy.double().abs().sum(0)
            within(f'colsum_accum real M={M} N={N}', vec_err(out.t, want, scale), vec_err(i0 + dy.sum(0), want, scale),
                   vec_err(seq_sum(dy, i0), want, scale))


# ---- BatchNorm1d + ReLU
def bn_case(fam, R, D, bias=None):
    key = ('bn', fam, R, D, bias)
    if key in _CACHE:
        return _CACHE[key]
    seed = 2000 + 5 * R + D
    x, (w, b), eps = bn_family(fam, R, D, seed), bn_params(fam, D, seed + 1, bias), f32(EPS_BN)
    g = torch.Generator().manual_seed(seed + 2)
    c = NS(fam=fam, R=R, D=D, x=x, w=w, b=b, ref=bn_fwd_ref(x, w, b, eps, F64), f32=bn_fwd_ref(x, w, b, eps, F32),
           std64=x.double().std(0, unbiased=False), rm0=torch.randn(D, generator=g), rv0=torch.rand(D, generator=g) + 0.5)
    _CACHE[key] = c
    return c


def bn_ws(lib, R, D):
    n = int(lib.vitae_bn1d_split_ws_floats(R, D))
    assert n == bn_split_plan(R, D)[0] * 3 * D          # the forward's records: mean as two floats, M2
    return Buf((n,), inner=float('nan'))


def bn_fwd_gpu(lib, form, c, rm0, rv0, nbt0, mom, want16=True, track=True):
    """form 'one' | 'split'.  track False: running_mean is NULL (running_var and the counter are still passed and must not move)."""
    R, D = c.R, c.D
    xd, wd, bd = Buf((R, D), c.x), Buf((D,), c.w), Buf((D,), c.b)
    y, y16 = Buf((R, D)), (Buf((R, D), dtype=BF16) if want16 else None)
    sm, sr, rm, rv = Buf((D,)), Buf((D,)), Buf((D,), rm0), Buf((D,), rv0)
    nbt = Buf((1,), torch.tensor([nbt0]), dtype=torch.int64)
    args = (xd.ptr, wd.ptr, bd.ptr, y.ptr, ptr(y16), sm.ptr, sr.ptr, rm.ptr if track else None, rv.ptr, nbt.ptr, R, D, EPS_BN, mom)
    ws = None
    if form == 'split':
        ws = bn_ws(lib, R, D)
        lib.vitae_bn1d_relu_fwd_split(*args, ws.ptr, st())
    else:
        lib.vitae_bn1d_relu_fwd(*args, st())
    assert all_intact(y, y16, sm, sr, rm, rv, nbt, ws)
    assert ws is None or not bool(torch.isnan(ws.t).any())
    return NS(y=y.t, y16=None if y16 is None else y16.t, sm=sm.t, sr=sr.t, rm=rm.t, rv=rv.t, nbt=int(nbt.t[0]))


def check_bn_fwd(label, c, out, rm0, rv0, mom, track=True):
    eps = f32(EPS_BN)
    y64, m64, r64, u64 = c.ref
    yf, mf, rf, uf = c.f32
    yt, mt, rt, rmt, rvt = torch_bn_fwd(c.x, c.w, c.b, eps, rm0, rv0, mom)
    assert bool(torch.isfinite(out.y).all())
    within(f'{label} y', col_err(out.y, y64), col_err(yt, y64), col_err(yf, y64))
    sc = m64.abs() + c.std64
    within(f'{label} save_mean', vec_err(out.sm, m64, sc), vec_err(mt, m64, sc), vec_err(mf, m64, sc))
    within(f'{label} save_rstd', vec_err(out.sr, r64), vec_err(rt, r64), vec_err(rf, r64))
    if out.y16 is not None:
        assert torch.equal(out.y16, out.y.to(BF16))
    if track:
        for name, got, r0, s64, s32, tch in (('running_mean', out.rm, rm0, m64, mf, rmt), ('running_var', out.rv, rv0, u64, uf, rvt)):
            want, scale = running_ref(r0, s64, f32(mom), F64)
            within(f'{label} {name}', vec_err(got, want, scale), vec_err(tch, want, scale), vec_err(running_ref(r0, s32, f32(mom), F32)[0], want, scale))
    else:
        assert torch.equal(out.rm.cpu(), rm0) and torch.equal(out.rv.cpu(), rv0)
    if c.fam == 'const':
        assert float(out.sm[0]) == 3.0 and float(out.sm[1]) == -2.0
        assert bool((out.y[:, 0] == 0).all()) and bool((out.y[:, 1] == 0.75).all())


def bn_bwd_gpu(lib, form, c, dy, y_given, sm, sr, init, want16):
    R, D = c.R, c.D
    dyd, xd, yd, wd = Buf((R, D), dy), Buf((R, D), c.x), Buf((R, D), y_given), Buf((D,), c.w)
    smd, srd = Buf((D,), sm), Buf((D,), sr)
    dx, dx16 = Buf((R, D)), (Buf((R, D), dtype=BF16) if want16 else None)
    dw, db = Buf((D,), init[0]), Buf((D,), init[1])
    args = (dyd.ptr, xd.ptr, yd.ptr, wd.ptr, smd.ptr, srd.ptr, dx.ptr, ptr(dx16), dw.ptr, db.ptr, R, D)
    ws = None
    if form == 'split':
        ws = bn_ws(lib, R, D)
        lib.vitae_bn1d_relu_bwd_split(*args, ws.ptr, st())
    else:
        lib.vitae_bn1d_relu_bwd(*args, st())
    assert all_intact(dx, dx16, dw, db, ws)
    if ws is not None:                                            # the backward's records are two floats a column of the three
        used = ws.n // 3 * 2
        assert not bool(torch.isnan(ws.t[:used]).any()) and bool(torch.isnan(ws.t[used:]).all())
    return NS(dx=dx.t, dx16=None if dx16 is None else dx16.t, dw=dw.t, db=db.t)


def check_bn_bwd(label, c, dy, y_given, out, init, stats=None):
    """y_given: the CPU copy of the y the kernel got (its mask).  stats None: the kernel got the forward kernel's save_mean /
    save_rstd and the reference uses the float64 statistics of x; else the fp32 pair both were given."""
    eps = f32(EPS_BN)
    _, m64, r64, _ = c.ref
    true = bn_bwd_ref(dy, c.x, y_given, c.w, m64, r64, F64)
    ref = true if stats is None else bn_bwd_ref(dy, c.x, y_given, c.w, stats[0], stats[1], F64)
    m32, r32 = (c.f32[1], c.f32[2]) if stats is None else stats
    fm = bn_bwd_ref(dy, c.x, y_given, c.w, m32, r32, F32)
    g = dy * (y_given > 0)
    tc = torch_bn_bwd(g, c.x, c.w, eps)
    sc = c.w.double().abs() * r64 * g.double().abs().amax(0)
    assert bool(torch.isfinite(out.dx).all())
    within(f'{label} dx', col_err(out.dx, ref[0], sc), col_err(tc[0], true[0], sc), col_err(fm[0], ref[0], sc))
    for name, got, i0, k in (('dw', out.dw, init[0], 1), ('db', out.db, init[1], 2)):
        want, scale = i0.double() + ref[k].sum(0), i0.double().abs() + ref[k].abs().sum(0)
        want_t, scale_t = i0.double() + true[k].sum(0), i0.double().abs() + true[k].abs().sum(0)
        within(f'{label} {name}', vec_err(got, want, scale), vec_err(i0 + tc[k], want_t, scale_t), vec_err(seq_sum(fm[k], i0), want, scale))
    if out.dx16 is not None:
        assert torch.equal(out.dx16, out.dx.to(BF16))
    if c.fam == 'const':                                         # column 0: y == 0 everywhere, nothing flows
        assert bool((out.dx[:, 0] == 0).all()) and float(out.dw[0]) == float(init[0][0]) and float(out.db[0]) == float(init[1][0])


def bn_both_passes(lib, form, label, c, k):
    """Forward twice (momentum 0.1 then 0.3, from random running statistics; the second call starts from what the first left), then
    the backward 'chain' and 'isolated'.  Bit 0 of k: the bf16 copies."""
    R, D = c.R, c.D
    want16 = bool(k & 1)
    one = bn_fwd_gpu(lib, form, c, c.rm0, c.rv0, 0, 0.1, want16)
    check_bn_fwd(f'{label} call 1', c, one, c.rm0, c.rv0, 0.1)
    rm1, rv1 = one.rm.cpu().clone(), one.rv.cpu().clone()
    two = bn_fwd_gpu(lib, form, c, rm1, rv1, one.nbt, 0.3, want16)
    check_bn_fwd(f'{label} call 2', c, two, rm1, rv1, 0.3)
    assert (one.nbt, two.nbt) == (1, 2) and torch.equal(_bits(one.y), _bits(two.y))
    init = ln_bwd_init(D, R + D)[:2]
    for mode in ('chain', 'isolated'):
        dy = real_grad((R, D), 7 * R + D + len(mode))
        if mode == 'chain':
            y_given, sm, sr, stats = one.y, one.sm, one.sr, None
        else:
            stats = (c.ref[1].float(), c.ref[2].float())
            y_given, sm, sr = c.ref[0].float(), stats[0], stats[1]
        out = bn_bwd_gpu(lib, form, c, dy, y_given, sm, sr, init, want16 ^ (mode == 'isolated'))
        check_bn_bwd(f'{label} {mode}', c, dy, y_given.cpu(), out, init, stats)
    return one


@gpu
@pytest.mark.parametrize('fam', BN_FAMILIES)
@pytest.mark.parametrize('D', [4, 60, 64, 68, 100])
def test_bn1d_relu_one_workgroup_per_strip(lib, D, fam):
    """R = 65, D = 100 has a column whose outputs nearly cancel (w = 0.047, b = -0.075): its y shows an error of M2 four-fold
    (LABNOTES.md)."""
    for i, R in enumerate((2, 15, 16, 17, 63, 64, 65, 130)):
        bn_both_passes(lib, 'one', f'bn1d_relu {fam} R={R} D={D}', bn_case(fam, R, D), i + D // 4)


BN_SPLIT_SHAPES = [(2, 4), (100, 64), (97, 64), (1000, 4), (12289, 4)]


@gpu
@pytest.mark.parametrize('fam', BN_FAMILIES)
@pytest.mark.parametrize('R,D', BN_SPLIT_SHAPES)
def test_bn1d_relu_split(lib, R, D, fam):
    """One split; four even ones; an uneven last one; a last split shorter than the 16 row groups; RS < rs.  The workspace is
    written in full and not past vitae_bn1d_split_ws_floats; twice is bitwise the same."""
    c = bn_case(fam, R, D)
    a = bn_both_passes(lib, 'split', f'bn1d_relu_split {fam} R={R} D={D}', c, BN_FAMILIES.index(fam))
    b = bn_fwd_gpu(lib, 'split', c, c.rm0, c.rv0, 0, 0.1, a.y16 is not None)
    for name in ('y', 'sm', 'sr', 'rm', 'rv'):
        assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name
    dy, init = real_grad((R, D), 3), ln_bwd_init(D, 4)[:2]
    o1, o2 = (bn_bwd_gpu(lib, 'split', c, dy, a.y, a.sm, a.sr, init, True) for _ in range(2))
    for name in ('dx', 'dx16', 'dw', 'db'):
        assert torch.equal(_bits(getattr(o1, name)), _bits(getattr(o2, name))), name


@gpu
@pytest.mark.parametrize('form', ['one', 'split'])
def test_bn1d_relu_without_running_statistics(lib, form):
    """running_mean == NULL: y and the saved statistics as ever; running_var and num_batches_tracked are passed and do not move."""
    for R, D in ((17, 60), (100, 64)):
        c = bn_case('plain', R, D)
        out = bn_fwd_gpu(lib, form, c, c.rm0, c.rv0, 5, 0.1, True, track=False)
        check_bn_fwd(f'bn1d_relu{"_split" if form == "split" else ""} untracked plain R={R} D={D}', c, out, c.rm0, c.rv0, 0.1, track=False)
        assert out.nbt == 5


@gpu
@pytest.mark.parametrize('form', ['one', 'split'])
def test_bn1d_relu_bwd_db_is_exact_where_every_unit_is_on(lib, form):
    """bias 100: y > 0 everywhere, so db += sum of an integer dy exactly — every row, every split, once."""
    shapes = BN_SPLIT_SHAPES if form == 'split' else [(R, D) for D in (4, 60, 64, 68, 100) for R in (2, 15, 16, 17, 63, 64, 65, 130)]
    for R, D in shapes:
        c = bn_case('plain', R, D, bias=100.0)
        fwd = bn_fwd_gpu(lib, form, c, c.rm0, c.rv0, 0, 0.1, False)
        assert bool((fwd.y > 0).all())
        dy, init = int_grad((R, D), R + D, lim=4), ln_bwd_init(D, R)[:2]
        out = bn_bwd_gpu(lib, form, c, dy, fwd.y, fwd.sm, fwd.sr, init, False)
        assert torch.equal(out.db.cpu(), init[1] + dy.sum(0)), (R, D)
        check_bn_bwd(f'bn1d_relu{"_split" if form == "split" else ""} all-on plain R={R} D={D}', c, dy, fwd.y.cpu(), out, init)


@gpu
@pytest.mark.parametrize('fam', ['plain', 'tiny', 'scales'])
@pytest.mark.parametrize('D', [7, 64, 768])
def test_bn1d_relu_eval(lib, D, fam):
    """Eval mode from running statistics; 'tiny' gives column 0 a running variance of 1e-6 against eps = 1e-5."""
    for R in (1, 37):
        c = bn_case(fam if fam != 'tiny' else 'plain', R, D)
        rm, rv = c.rm0.clone(), c.rv0.clone()
        x = c.x.clone()
        if fam == 'tiny':
            rv[0] = 1e-6
            x[:, 0] = rm[0] + 1e-3 * real_grad((R,), 5)
        eps = f32(EPS_BN)
        y = Buf((R, D))
        bufs = [Buf(t.shape, t) for t in (x, c.w, c.b, rm, rv)]
        lib.vitae_bn1d_relu_eval(*[t.ptr for t in bufs], y.ptr, R, D, EPS_BN, st())
        assert all_intact(y)
        y64 = bn_eval_ref(x, c.w, c.b, rm, rv, eps, F64)
        within(f'bn1d_relu_eval {fam} R={R} D={D} y', col_err(y.t, y64), col_err(F.relu(F.batch_norm(x, rm, rv, c.w, c.b, False, 0.1, eps)), y64),
               col_err(bn_eval_ref(x, c.w, c.b, rm, rv, eps, F32), y64))


# ---- refusals: VitaeError, and not one byte written
def _refused(VitaeError, fn, args, outs):
    with pytest.raises(VitaeError):
        fn(*args)
    torch.cuda.synchronize()
    for o in outs:
        assert o.untouched()


@gpu
def test_layernorm_refusals(lib, VitaeError):
    def bufs(M, D):
        z = torch.zeros(M, D)
        return NS(x=Buf((M, D), z), w=Buf((D,), z[0]), b=Buf((D,), z[0]), y=Buf((M, D), keep=True), y16=Buf((M, D), dtype=BF16, keep=True),
                  mean=Buf((M,), keep=True), rstd=Buf((M,), keep=True), dy=Buf((M, D), z), dx=Buf((M, D), keep=True),
                  dw=Buf((D,), keep=True), db=Buf((D,), keep=True), dx16=Buf((M, D), dtype=BF16, keep=True), cs=Buf((D,), keep=True))

    def fwd_args(q, M, D, drop=()):
        a = dict(x=q.x.ptr, w=q.w.ptr, b=q.b.ptr, y=q.y.ptr, y16=q.y16.ptr, mean=q.mean.ptr, rstd=q.rstd.ptr)
        a.update({k: None for k in drop})
        return tuple(a.values()) + (M, D, EPS_LN, st())

    def bwd_args(q, M, D, drop=()):
        a = dict(dy=q.dy.ptr, x=q.x.ptr, w=q.w.ptr, mean=q.mean.ptr, rstd=q.rstd.ptr, dx=q.dx.ptr, dw=q.dw.ptr, db=q.db.ptr, dx16=q.dx16.ptr, cs=q.cs.ptr)
        a.update({k: None for k in drop})
        return tuple(a.values()) + (M, D, 0, st())

    q = bufs(3, 1025)
    outs = [q.y, q.y16, q.mean, q.rstd, q.dx, q.dw, q.db, q.dx16, q.cs]
    _refused(VitaeError, lib.vitae_layernorm_fwd, fwd_args(q, 3, 1025), outs)
    _refused(VitaeError, lib.vitae_layernorm_bwd, bwd_args(q, 3, 1025), outs)
    q = bufs(3, 64)
    outs = [q.y, q.y16, q.mean, q.rstd, q.dx, q.dw, q.db, q.dx16, q.cs]
    _refused(VitaeError, lib.vitae_layernorm_fwd, fwd_args(q, 0, 64), outs)
    _refused(VitaeError, lib.vitae_layernorm_bwd, bwd_args(q, 0, 64), outs)
    for drop in (('x',), ('w',), ('b',), ('mean',), ('rstd',), ('y', 'y16')):
        _refused(VitaeError, lib.vitae_layernorm_fwd, fwd_args(q, 3, 64, drop), outs)
    for drop in ('dy', 'x', 'w', 'mean', 'rstd', 'dx', 'dw', 'db'):
        _refused(VitaeError, lib.vitae_layernorm_bwd, bwd_args(q, 3, 64, (drop,)), outs)


@gpu
def test_layernorm_bwd_part_refusals(lib, VitaeError):
    """D outside {256, 512, 768, 1024}; any operand 4 bytes off (dx_bf16: 2 bytes)."""
    M = 9
    for D, which in ((100, None), (256, 'dy'), (256, 'x'), (256, 'w'), (256, 'dx'), (256, 'part'), (256, 'dx16')):
        z = torch.zeros(M, D)
        o = lambda name: 1 if which == name else 0
        dy, x, w = Buf((M, D), z, off=o('dy')), Buf((M, D), z, off=o('x')), Buf((D,), z[0], off=o('w'))
        mean, rstd = Buf((M,), z[:, 0]), Buf((M,), z[:, 0] + 1)
        dx, part = Buf((M, D), off=o('dx'), keep=True), Buf((2, 3 * D), off=o('part'), keep=True)
        dx16 = Buf((M, D), dtype=BF16, off=o('dx16'), keep=True)
        _refused(VitaeError, lib.vitae_layernorm_bwd_part, (dy.ptr, x.ptr, w.ptr, mean.ptr, rstd.ptr, dx.ptr, part.ptr, dx16.ptr, M, D, 0, st()),
                 [dx, part, dx16])


@gpu
@pytest.mark.parametrize('form', ['one', 'split'])
def test_bn1d_relu_refusals(lib, VitaeError, form):
    """D % 4 != 0; an operand 4 bytes off (the split forms' workspace included)."""
    R = 17
    cases = [(6, None), (8, 'x'), (8, 'y'), (8, 'dy'), (8, 'dx'), (8, 'sm')] + ([(8, 'ws')] if form == 'split' else [])
    for D, which in cases:
        z = torch.zeros(R, D)
        o = lambda name: 1 if which == name else 0
        x, w, b, dy = Buf((R, D), z, off=o('x')), Buf((D,), z[0] + 1), Buf((D,), z[0]), Buf((R, D), z, off=o('dy'))
        y, y16, dx, dx16 = Buf((R, D), off=o('y'), keep=True), Buf((R, D), dtype=BF16, keep=True), Buf((R, D), off=o('dx'), keep=True), Buf((R, D), dtype=BF16, keep=True)
        sm, sr, rm, rv = Buf((D,), off=o('sm'), keep=True), Buf((D,), keep=True), Buf((D,), keep=True), Buf((D,), keep=True)
        nbt, dw, db = Buf((1,), dtype=torch.int64, keep=True), Buf((D,), keep=True), Buf((D,), keep=True)
        ws = Buf((max(int(lib.vitae_bn1d_split_ws_floats(R, D)), 4),), off=o('ws'), keep=True)
        outs = [y, y16, dx, dx16, sm, sr, rm, rv, nbt, dw, db, ws]
        tail = (ws.ptr, st()) if form == 'split' else (st(),)
        if which in (None, 'x', 'y', 'sm', 'ws'):
            fn = lib.vitae_bn1d_relu_fwd_split if form == 'split' else lib.vitae_bn1d_relu_fwd
            _refused(VitaeError, fn, (x.ptr, w.ptr, b.ptr, y.ptr, y16.ptr, sm.ptr, sr.ptr, rm.ptr, rv.ptr, nbt.ptr, R, D, EPS_BN, 0.1) + tail, outs)
        if which in (None, 'x', 'y', 'dy', 'dx', 'sm', 'ws'):
            fn = lib.vitae_bn1d_relu_bwd_split if form == 'split' else lib.vitae_bn1d_relu_bwd
            _refused(VitaeError, fn, (dy.ptr, x.ptr, y.ptr, w.ptr, sm.ptr, sr.ptr, dx.ptr, dx16.ptr, dw.ptr, db.ptr, R, D) + tail, outs)


@gpu
def test_ln_grad_reduce_refusals(lib, VitaeError):
    """n = 0, a record count of 0, D % 4 != 0, and any part / dw / db / dx_colsum pointer off 16 bytes — in the first launch's
    instances or in a later one's (49 instances, the 49th bad): the call is judged before anything is launched."""
    def case(n, bad, what):
        Ds, Gs = [8] * n, [3] * n
        if what == 'D':
            Ds[bad] = 6
        if what == 'G':
            Gs[bad] = 0
        o = lambda i, name: 1 if (i == bad and what == name) else 0
        parts = [Buf((3, 3 * 8), torch.ones(3, 24), off=o(i, 'part')) for i in range(n)]
        tg = [[Buf((8,), off=o(i, name), keep=True) for name in ('dw', 'db', 'cs')] for i in range(n)]
        return parts, tg, Ds, Gs

    for n, bad in ((1, 0), (3, 1), (49, 48)):
        for what in ('D', 'G', 'part', 'dw', 'db', 'cs'):
            parts, tg, Ds, Gs = case(n, bad, what)
            with pytest.raises(VitaeError):
                reduce_gpu(lib, parts, [t[0] for t in tg], [t[1] for t in tg], [t[2] for t in tg], Gs, Ds)
            torch.cuda.synchronize()
            assert all(b.untouched() for t in tg for b in t), (n, bad, what)
    parts, tg, Ds, Gs = case(1, 0, None)
    a = np.zeros(1, dtype=np.uint64)
    with pytest.raises(VitaeError):
        lib.vitae_ln_grad_reduce(0, a.ctypes.data, a.ctypes.data, a.ctypes.data, a.ctypes.data, a.ctypes.data, a.ctypes.data, st())
    reduce_gpu(lib, parts, [t[0] for t in tg], [t[1] for t in tg], [t[2] for t in tg], Gs, Ds)      # and the good call goes through
    torch.cuda.synchronize()
    assert all(bool((b.t == SENT + 3).all()) and b.intact() for t in tg for b in t)
