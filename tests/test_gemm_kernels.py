"""The dense contractions of csrc/gemm.hip, gemm_bf16.hip, gemm_glds.hip and gemm_bt.hip: bit for bit on integer operands, and per
element against float64 — with NaN around every operand and sentinels around every output.

One harness (``gemm_call``; ``pair_bf16_call`` / ``pair_glds_call`` / ``group_call`` for the paired and grouped launchers): operands
live inside larger allocations whose surroundings are NaN (one guard row before and after, the gap columns when ld > width, 64
elements behind); every output (C, C16, aux, dx, dx16, dw, dw16, column and row sums) lives in a buffer of the sentinel SENT = 7.25
(exact in bf16) with one guard row before and after, the gap columns and >= 64 elements behind, starts as NaN inside (or as the
accumulated old content) and must leave every sentinel unchanged.  Split-K workspaces have exactly the library's own ``*_ws_floats``
floats, tickets zero and the rest NaN, then 64 sentinels: afterwards tickets zero, sentinels untouched.  A refused call (a
VITAE_ERR_* return) must leave every output sentinel-clean.  NaN in the gaps of A, B, residual and aux is part of the test: a
kernel that reads past a row's width, or past K in a zero-filled k-tail, and lets it reach a valid output shows NaN.

Family 1 — exact operands, ``torch.equal`` against the float64 result cast to fp32, no tolerance.  A and B are integers in
[-4, 4]; bias, residual and the old C integers in [-8, 8]: every product and partial sum is an integer below K 16 + 24 < 2^24
(asserted), so the result is the same bits in any summation order, on any tile, at any split and any precision.  Two-term operands
(VITAE_PREC_BF16X3, vitae_gemm_wsx3, vitae_gemm_glds_w2, vitae_cast_bf16_hilo): one operand is hi + lo, hi a nonzero integer of
+-[1, 4], lo an integer of [-3, 3] times 2^-11 (bf16(hi + lo) == hi and bf16(hi + lo - hi) == lo; 3 x 2^-10 would NOT do:
1 - 3 x 2^-10 rounds to 1 - 2^-8), the other an integer in [-2, 2], K <= 512: the fp32 product is the float64 one, the bf16-only
product is not, and a kernel that drops the lo plane, adds it twice or drops hi.lo against lo.hi gives a wrong exact value.
GELU epilogues: one operand is scaled by a power of two so that the pre-activations sit on a grid of 1/8 or finer with a deviation
of about 3; the saved pre-activation is bitwise the exact value (its bf16 with VITAE_EPI_AUX_BF16), ReLU and the ReLU mask are
bitwise, and GELU / GELU' / DGELU are compared per element with the float64 erf formulas on the exact fp32 pre-activation:
|y - y64| / |v|, v the factor the GELU term multiplies (the pre-activation; acc for DGELU), bound max(FACTOR e32, FLOOR) with e32 the
same metric of torch's fp32 F.gelu / its autograd on the CPU.

Family 2 — rounding quality per element against float64.  Reference: the float64 product of the operand values the header gives the
path — PREC_F32: the fp32 operands; one-term bf16 paths: the RNE-rounded operands; split paths: the three terms hi.hi + hi.lo + lo.hi
of hi = bf16(x), lo = bf16(x - hi); vitae_gemm_glds_w2: x16 (W_hi + W_lo)^T; the LDS-DMA family: the bf16 inputs as given.  The
terms are laid side by side along k (``path_operands``), so every path is one product over n = K, 2 K or 3 K addends.
Metric: e = |c - c64| / (sum over the addends |a||b| + |bias| + |residual| + |old C|), the worst element.  Bound:
e <= max(FACTOR e32, FLOOR); e32 is the same metric on the same operand values of the plain fp32 statement, the larger of torch's
fp32 matmul on the CPU and the k-ordered running sum acc += a_k b_k in fp32.  FACTOR = 3 and FLOOR = 4 x 2^-24 as in
tests/test_norm_kernels.py.  Split paths also against the TRUE fp32-operand product: e <= 2^-16 + FACTOR e32 — hi + lo carries an
operand to 2^-18 of itself (bf16 keeps 8 bits, twice: |x - hi - lo| <= 2^-9 2^-9 |x|), so the two kept cross terms and hi.hi miss
at most 2 x 2^-18 |a||b|, and the dropped lo.lo term is at most 2^-9 2^-9 = 2^-18 |a||b|: together under 2^-16 sum |a||b|.
A path that is bitwise right in family 1 but exceeds FACTOR e32 on `plain` would be held to the a-priori any-order bound
(n + 2) 2^-23 instead (LABNOTES.md says which, if any).
Input families (``family``; properties CPU-tested): plain N(0, 1) — scales: row scales of A and column scales of B log-uniform over
1e-3 .. 1e3 — cancel: a constant-sign A against rows of B that sum to nearly zero, |c| << sum |a||b| — small-epilogue: bias,
residual and old C at 1e-3 of the product's scale; there the numerator is the difference to the call without them minus the
addends, the denominator |bias| + |residual| + |old| alone, so a missing or misplaced addend is of order one.

Which shape reaches which kernel (restated from the launchers; the environment knobs are not touched):
  vitae_gemm prec 0 / 1, vitae_linear_*   gemm_kernel, 64 x 64 tile, BK = 32, operand extents % 4; split s gives
                        kps = ceil32(ceil(K / s)) and ceil(K / kps) launches in z + splitk_reduce_kernel (GELU: never split).
                        (M, N, K) around (60|64|68, 63|64|65, 4|28|32|36|68|100|132): K = 68 at s = 2 is 64 + 4, K = 100 at
                        s = 3 becomes 64 + 36, K = 132 at s = 3 is 64 + 64 + 4; K = 1028 has partial sums of several hundred (a bf16
                        round trip of one is then a wrong integer: everything up to 256 is exact in bf16).
  prec 2 / vitae_gemm_bf16x3   gemm_bf16_kernel<64, 64, 128, X3> (64 x 128 needs >= 512 tiles): kps = ceil128(..): K = 132, s = 2: 128 + 4.
  vitae_gemm_bf16       pick_cfg: 64 x 64 x 256 below 512 64 x 128 tiles, 64 x 128 x 128 from there (2052 x 1992: 33 x 16 = 528);
                        bf16 B needs its contiguous extent % 8; K = 260 at s = 2 is 256 + 4.
  vitae_linear_bwd_pair_bf16   N % 8, K % 8; each half by pick_cfg: gemm_bf16_pair_kernel<256, 64, 64, 256, 64, 64, 256> at the small
                        sizes; 2052 x 1992 (528 tiles of 64 x 128) makes a half wide: (2052, 8, 1992) the input gradient,
                        (8, 2056, 1992) the weight gradient, (2052, 2056, 1992) both (``pair_cfgs`` restates the rule).
  vitae_gemm_wsx3       gemm_wsx3_kernel, 64 x 64, 64-deep k-tiles with a zero-filled tail (K = 4, 60, 64, 68, 132), in-launch
                        split-K kps = ceil64(ceil(K / s)); M, N >= 8, N % 4 and 16-byte aligned C / aux / residual / bias.
  vitae_gemm_glds       vec_epilogue_ok fails for N % 4, ld % 4 or a C that is not 16-byte aligned -> the 64-row family with the
                        scalar epilogue; bt tile mode -2 -> the 64-row family: forward form with <= 512 workgroups
                        gemm_glds_pipe_kernel, other forms the 64 x 64 kernel, ceil(M / 64) ceil(N / 128) >= 400 the 64 x 128
                        kernel (1280 x 2560).  A forced tile t (vitae_gemm_glds_set_bt_tile; 0: 256 x 256, 3 / 4: 128 x 128, 5:
                        64 x 64, 6: 128 x 256 weight-gradient form only) serves the call iff vitae_gemm_glds_bt_choice == t AND the
                        split passed equals vitae_gemm_glds_pick_split_k_form (both asserted); the grid is rounded up to a
                        multiple of 8 workgroups, so 1, 7 and 9 tiles leave 7, 1 and 7 workgroups without one.  The planner's
                        split under a forced tile is found by scanning K (``k_for_split``): 2 and 3 on tiles 3 - 6.
  vitae_gemm_glds_w2    w2_plan: tile 5 / none -> the two-plane 64 x 64 workgroup (ws64_w2_launch), a forced big tile -> that tile
                        over 2 K with the activations wrapping.
  vitae_linear_bwd_pair_glds   mode -1, both halves without a big tile -> one gemm_ws64_pair_kernel launch; mode -2 ->
                        gemm_glds_pair_kernel; forced 3 / 4 / 0 -> two launches through the planner; dw == NULL -> the input
                        gradient alone.
  vitae_wgrad_group_bt  kinds by forced tile (-1 planner, 3 ping-pong, 4 / 6 wave-specialised); Mpad >= 256; the split is shrunk
                        to what the workspace holds.
Every GPU case of family 2 prints ``RATIO`` lines (run with -s); LABNOTES.md keeps the table."""
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_norm_kernels import FACTOR, FLOOR
from vit_ae_plus_plus_amd._abi import CONSTS

GUARD, SENT, NAN = 64, 7.25, float('nan')           # SENT is exact in bf16
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
FORMS = {'fwd': (1, 1), 'dgrad': (1, 0), 'wgrad': (0, 0), 'tn': (0, 1)}      # (a_kcontig, b_kcontig)
FAMILIES = ['plain', 'scales', 'cancel', 'small-epilogue']
E32_SANE = 2e-6            # the fp32 chain at K <= 1920 addends: ~1e-7 of sum |a||b| (kernel guide), sqrt(n) 2^-24 at most a few 1e-7
gpu = pytest.mark.gpu


# =========================================================================== inputs
def ints(shape, lim, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


def hilo_operand(shape, seed):
    """-> x = hi + lo, hi, lo: hi a nonzero integer of +-[1, 4], lo an integer of [-3, 3] times 2^-11"""
    g = torch.Generator().manual_seed(seed)
    hi = torch.randint(1, 5, shape, generator=g).float() * (1 - 2 * torch.randint(0, 2, shape, generator=g)).float()
    lo = torch.randint(-3, 4, shape, generator=g).float() * 2.0 ** -11
    return hi + lo, hi, lo


def gelu_scale(K, lim=4):
    """the power of two that brings an integer product over K addends to a deviation of about 3"""
    sd = (lim * (lim + 1) / 3.0) * math.sqrt(K)          # E x^2 = lim (lim + 1) / 3 for a uniform integer of [-lim, lim]
    return 2.0 ** -max(0, round(math.log2(sd / 3.0)))


def family(fam, M, N, K, seed):
    """-> a [M, K], b [N, K], bias [N] | None, res [M, N] | None, old [M, N] | None (fp32)"""
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    bias = res = old = None
    if fam == 'scales':
        a = a * (10.0 ** (torch.rand(M, generator=g) * 6 - 3))[:, None]
        b = b * (10.0 ** (torch.rand(N, generator=g) * 6 - 3))[:, None]
    elif fam == 'cancel':
        a = 1.0 + 0.01 * a
        b = b - b.mean(1, keepdim=True)
    elif fam == 'small-epilogue':
        b = b * K ** -0.5
        bias, res, old = (1e-3 * torch.randn(*s, generator=g) for s in ((N,), (M, N), (M, N)))
    elif fam != 'plain':
        raise ValueError(fam)
    return a.float().contiguous(), b.float().contiguous(), bias, res, old


def rne(x):
    return x.to(BF16).float()


def path_operands(path, a, b):
    """The operand values the header gives a path, its terms side by side along k: -> A' [M, n], B' [N, n] (float64)."""
    if path == 'f32':
        A, B = [a], [b]
    elif path == 'bf16':
        A, B = [rne(a)], [rne(b)]
    elif path == 'x3':
        ah, bh = rne(a), rne(b)
        al, bl = rne(a - ah), rne(b - bh)
        A, B = [ah, ah, al], [bh, bl, bh]
    elif path == 'w2':                                   # a is bf16 already
        bh = rne(b)
        A, B = [a, a], [bh, rne(b - bh)]
    else:
        raise ValueError(path)
    return torch.cat(A, 1).double(), torch.cat(B, 1).double()


# =========================================================================== references and metrics
def epilogue_ref(acc, bias=None, res=None, old=None):
    c = acc.clone()
    if bias is not None:
        c = c + bias.to(c.dtype)
    if res is not None:
        c = c + res.to(c.dtype)
    if old is not None:
        c = c + old.to(c.dtype)
    return c


def gemm_ref(A, B, bias=None, res=None, old=None):
    """float64: -> c64, the sum of the absolute addends"""
    A, B = A.double(), B.double()
    z = lambda t: None if t is None else t.double().abs()
    return epilogue_ref(A @ B.t(), bias, res, old), epilogue_ref(A.abs() @ B.abs().t(), z(bias), z(res), z(old))


def running_sum32(A, B):
    """acc += a_k b_k in fp32, k after k (a loop on purpose: the order is the statement)"""
    A, B = A.float(), B.float()
    acc = torch.zeros(A.shape[0], B.shape[0])
    for k in range(A.shape[1]):
        acc = acc + A[:, k:k + 1] * B[:, k][None, :]
    return acc


def plain32(A, B, bias=None, res=None, old=None):
    """the plain fp32 statement, twice: torch's matmul and the running sum, each with the epilogue in the kernels' order"""
    return [epilogue_ref(p, bias, res, old) for p in (A.float() @ B.float().t(), running_sum32(A, B))]


def _ratio(num, den):
    """num / den with 0 / 0 = 0 and x / 0 = inf; NaN counts as inf"""
    inf, zero = torch.full_like(num, float('inf')), torch.zeros_like(num)
    r = torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num == 0, zero, inf))
    return torch.where(torch.isnan(r), inf, r)


def elem_err(c, c64, den):
    return float(_ratio((c.double() - c64).abs(), den).max())


def gelu64(v):
    v = v.double()
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def dgelu64(v):
    v = v.double()
    return 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0))) + v * torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)


def torch_dgelu32(v):
    x = v.float().clone().requires_grad_(True)
    F.gelu(x).sum().backward()
    return x.grad


def within(label, e, *e32s, extra=0.0):
    e32 = max(e32s)
    r = e / e32 if e32 > 0 else (0.0 if e == 0 else float('inf'))
    print(f'RATIO {label}: e={e:.3e} e32={e32:.3e} ratio={r:.2f}')
    assert e <= max(FACTOR * e32, FLOOR) + extra, (label, e, e32)
    return r


def gelu_checks(label, pre, y=None, dsaved=None, dgelu=None, acc=None):
    """pre: the exact fp32 pre-activation (CPU).  y = GELU(pre), dsaved = GELU'(pre), dgelu = acc GELU'(pre): each |got - f64| / |v|."""
    pre = pre.float()
    if y is not None:
        within(label + ' gelu', elem_err(y, gelu64(pre), pre.double().abs()), elem_err(F.gelu(pre), gelu64(pre), pre.double().abs()))
    if dsaved is not None:
        within(label + ' gelu-deriv', elem_err(dsaved, dgelu64(pre), pre.double().abs()),
               elem_err(torch_dgelu32(pre), dgelu64(pre), pre.double().abs()))
    if dgelu is not None:
        acc = acc.float()
        x = pre.clone().requires_grad_(True)
        F.gelu(x).backward(acc)
        within(label + ' dgelu', elem_err(dgelu, acc.double() * dgelu64(pre), acc.double().abs()),
               elem_err(x.grad, acc.double() * dgelu64(pre), acc.double().abs()))


# =========================================================================== CPU tests of the constructions above
def test_integer_operands_are_exact_in_any_order_and_precision():
    K = 4096
    assert K * 16 + 24 < 2 ** 24
    a, b = ints((33, K), 4, 1), ints((29, K), 4, 2)
    want = (a.double() @ b.double().t())
    assert float(want.abs().max()) + 24 < 2 ** 24
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(3))
    assert torch.equal(a @ b.t(), want.float()) and torch.equal(a[:, perm] @ b[:, perm].t(), want.float())
    assert torch.equal(rne(a) @ rne(b).t(), want.float()) and torch.equal(running_sum32(a, b), want.float())
    assert torch.equal(torch.tensor(SENT).to(BF16).float(), torch.tensor(SENT))


def test_two_term_operands_split_exactly():
    K = 512
    x, hi, lo = hilo_operand((40, K), 4)
    y = ints((24, K), 2, 5)
    assert float(hi.abs().min()) >= 1 and torch.equal(rne(x), hi) and torch.equal(rne(x - rne(x)), lo)
    want = x.double() @ y.double().t()
    assert torch.equal(x @ y.t(), want.float()) and torch.equal(y @ x.t(), want.t().float())
    assert torch.equal(running_sum32(x, y), want.float())
    assert not torch.equal(rne(x) @ y.t(), want.float())                       # the bf16-only product loses the lo plane
    A, B = path_operands('x3', x, y)                                            # hi.hi + hi.lo + lo.hi is everything: y has no lo
    assert torch.equal((A @ B.t()).float(), want.float())
    A, B = path_operands('w2', y, x)
    assert torch.equal((A @ B.t()).float(), want.t().float())
    bad = torch.tensor(1.0 - 3 * 2.0 ** -10)                                    # why lo stops at 3 x 2^-11
    assert float(rne(bad)) == 1.0 - 2.0 ** -8


def test_references_against_torch_float64():
    a, b, bias, res, old = family('small-epilogue', 37, 29, 132, 6)
    c64, den = gemm_ref(a, b, bias, res, old)
    want = F.linear(a.double(), b.double(), bias.double()) + res.double() + old.double()
    assert float((c64 - want).abs().max()) < 1e-12 and bool((den >= c64.abs() - 1e-12).all())
    assert float((running_sum32(a, b).double() - a.double() @ b.double().t()).abs().max()) < 1e-4
    v = torch.linspace(-6, 6, 97, dtype=F64)
    x = v.clone().requires_grad_(True)
    F.gelu(x).sum().backward()
    assert float((gelu64(v) - F.gelu(v)).abs().max()) < 1e-14 and float((dgelu64(v) - x.grad).abs().max()) < 1e-14
    A, B = path_operands('x3', a, b)
    assert A.shape[1] == 3 * 132
    true = a.double() @ b.double().t()
    assert elem_err((A @ B.t()), true, a.double().abs() @ b.double().abs().t()) < 2.0 ** -16     # the split paths' extra bound


@pytest.mark.parametrize('fam', FAMILIES)
def test_input_families_have_their_properties(fam):
    M, N, K = 68, 65, 640
    a, b, bias, res, old = family(fam, M, N, K, 7)
    c64, den = gemm_ref(a, b)
    if fam == 'scales':
        ra, rb = a.abs().amax(1), b.abs().amax(1)
        assert float(ra.max() / ra.min()) > 1e4 and float(rb.max() / rb.min()) > 1e4
    if fam == 'cancel':
        assert bool((a > 0).all()) and float((c64.abs() / den).max()) < 0.02
    if fam == 'small-epilogue':
        scale = float(c64.std())
        assert 0.5 < scale < 2 and all(3e-4 < float(t.std()) < 3e-3 for t in (bias, res, old))
    else:
        assert bias is None and res is None and old is None
    for path in ('f32', 'bf16', 'x3'):                           # e32 is what the kernel guide says of the fp32 chain
        A, B = path_operands(path, a, b)
        c64p, denp = gemm_ref(A, B)
        e32 = max(elem_err(p, c64p, denp) for p in plain32(A, B))
        assert 0 < e32 < E32_SANE, (fam, path, e32)


def test_gelu_scale_and_e32_of_gelu():
    for K in (64, 128, 192):
        s = gelu_scale(K)
        pre = (ints((64, K), 4, 8) @ ints((64, K), 4, 9).t()) * s
        assert math.log2(s) == round(math.log2(s)) and s <= 1 / 8 and 1.5 < float(pre.std()) < 6
        assert float((pre.abs() <= 6).float().mean()) > 0.6
        e32 = elem_err(F.gelu(pre), gelu64(pre), pre.double().abs())
        assert e32 < 3e-7, e32


def test_new_metric_sees_what_the_old_one_missed():
    """The defects of the issue's blind spots, applied on the CPU to an honest fp32 result of bf16 operands (the LDS-DMA family's
    contract): under max|got - want| / max|want| each passes the old tolerance of 2e-3; under the new metric each is more than 100
    times max(FACTOR e32, FLOOR)."""
    M, N, K = 128, 768, 768
    g = torch.Generator().manual_seed(10)
    a, b = rne(torch.randn(M, K, generator=g)), rne(torch.randn(N, K, generator=g) * K ** -0.5)
    bias, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    c64, den = gemm_ref(a, b, bias, res)
    e32 = max(elem_err(p, c64, den) for p in plain32(a, b, bias, res))
    bound = max(FACTOR * e32, FLOOR)
    prod = a @ b.t()
    parts = [a[:, :K // 2] @ b[:, :K // 2].t(), a[:, K // 2:] @ b[:, K // 2:].t()]
    defects = {
        'product through bf16': rne(prod) + bias + res,
        'residual read as bf16': prod + bias + rne(res),
        'one split-K partial in bf16': rne(parts[0]) + parts[1] + bias + res,
        'bias rounded to bf16': prod + rne(bias) + res,
    }
    for name, got in defects.items():
        e = elem_err(got, c64, den)
        old_metric = float((got.double() - c64).abs().max() / c64.abs().max())
        assert old_metric < 2e-3 and e > 100 * bound, (name, e, bound, old_metric)
    # a missing bias of the last column at scale 1e-3: 4.6e-5 of the old metric; the small-epilogue metric, |difference to the
    # call without the addends - addends| / |addends|, against its own e32 (the fp32 statement with and without the bias)
    small = 1e-3 * torch.sign(bias) * (0.5 + bias.abs())      # (no bias near zero: a denominator of 1e-7 would measure the product's rounding)
    with_, without = prod + small, prod.clone()
    with_[:, -1] = prod[:, -1]
    den_s = small.double().abs().expand(M, N)
    metric = lambda w: float(_ratio(((w.double() - without.double()) - small.double()).abs(), den_s).max())
    e32s = metric(prod + small)
    assert float((with_.double() - (prod + small).double()).abs().max() / c64.abs().max()) < 2e-3
    assert metric(with_) == 1.0 and 1.0 > 100 * max(FACTOR * e32s, FLOOR), e32s
    # the zeroed smallest-scale row under log-uniform scales
    a2, b2, _, _, _ = family('scales', 130, 72, 768, 11)
    c64s, dens = gemm_ref(a2, b2)
    bound_s = max(FACTOR * max(elem_err(p, c64s, dens) for p in plain32(a2, b2)), FLOOR)
    got = a2 @ b2.t()
    got[int(a2.abs().amax(1).argmin())] = 0
    assert float((got.double() - c64s).abs().max() / c64s.abs().max()) < 1e-5 and elem_err(got, c64s, dens) > 100 * bound_s


# =========================================================================== the GPU harness
@pytest.fixture(scope='module')
def lib():
    from vit_ae_plus_plus_amd._abi import lib as L
    L.load()
    return L


@pytest.fixture(scope='module')
def C():
    return CONSTS


@pytest.fixture
def bt_mode(lib):
    yield lib.vitae_gemm_glds_set_bt_tile
    lib.vitae_gemm_glds_set_bt_tile(-1)


def st():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """A rows x width matrix (a vector: rows = 1) inside `off` + (rows + 2) x ld + GUARD elements of `fill` (NaN around inputs,
    SENT around outputs): one guard row before and after, the gap columns of every row, GUARD elements behind.  `data` (CPU) or
    `init` fills the rectangle.  The rectangle starts on a 16-byte boundary whatever ld is, plus `off` elements: a bad ld or a
    bad pointer is then the ONLY thing wrong with a call."""

    def __init__(self, rows, width, ld=None, dtype=F32, fill=SENT, data=None, init=NAN, off=0):
        self.ld = ld = width if ld is None else ld
        assert ld >= width
        per16 = 16 // torch.empty((), dtype=dtype).element_size()
        off += -ld % per16                                 # torch's allocations are 512-byte aligned; one guard row is ld elements
        n = off + (rows + 2) * ld + GUARD
        self.fill = fill
        self.full = torch.full((n,), fill, dtype=dtype, device='cuda')
        self.mask = torch.zeros(n, dtype=torch.bool, device='cuda')
        self.mask[off:off + (rows + 2) * ld].view(rows + 2, ld)[1:rows + 1, :width] = True
        self.view = self.full[off:off + (rows + 2) * ld].view(rows + 2, ld)[1:rows + 1, :width]
        if data is not None:
            self.view.copy_(data.reshape(rows, width).to(dtype))
        else:
            self.view.fill_(init)
        self.ptr = self.view.data_ptr()

    def clean(self):
        o = self.full[~self.mask]
        return bool(o.isnan().all()) if self.fill != self.fill else bool((o == self.fill).all())

    def untouched(self):
        return bool((self.full == self.fill).all())

    def cpu(self):
        return self.view.detach().cpu().clone()


class Workspace:
    """exactly n floats (the first `tickets` zero, the rest NaN) and GUARD sentinels behind"""

    def __init__(self, n, tickets=0):
        self.n, self.tickets = n, min(tickets, n)
        self.full = torch.full((n + GUARD,), NAN, device='cuda')
        self.full[:self.tickets] = 0
        self.full[n:] = SENT
        self.ptr = self.full.data_ptr() if n > 0 else None

    def clean(self):
        return bool((self.full[self.n:] == SENT).all()) and bool((self.full[:self.tickets].view(torch.int32) == 0).all())


def _p(b):
    return None if b is None else b.ptr


def _ld(b):
    return 0 if b is None else b.ld


def gemm_call(lib, entry, a, b, form='fwd', *, prec=0, b16=0, ld=None, bias=None, res=None, old=None, epi=0, aux=None, split=1,
              c32=True, c16=False, colsum=None, rowsum=None, acolsum=None, c_off=0, a_off=0, no_ws=False, expect=0):
    """One call of a GEMM entry point ('gemm', 'x3', 'bf16', 'wsx3', 'glds', 'w2') on the logical operands a [M, K], b [N, K]
    (CPU fp32) in the storage of `form`, with leading dimensions ld = {a, b, c, r, aux, c16}, the epilogue options, the split and
    (through the bt_mode fixture, by the caller) a forced tile.  -> every output on the CPU; guards are asserted here."""
    dll = lib.load()
    CO = CONSTS
    akc, bkc = FORMS[form]
    (M, K), N = a.shape, b.shape[0]
    ld = dict(ld or {})
    op16 = entry in ('glds', 'w2')
    refused = expect != 0
    init = SENT if refused else NAN
    As = a if akc else a.t()
    A = Buf(As.shape[0], As.shape[1], ld.get('a'), BF16 if op16 else F32, NAN, As, off=a_off)
    if entry == 'w2':
        hi = b.to(BF16)
        Bs = torch.cat([hi.float(), (b - hi.float()).to(BF16).float()], 1)
    else:
        Bs = b if bkc else b.t()
    B = Buf(Bs.shape[0], Bs.shape[1], ld.get('b'), BF16 if (op16 or b16) else F32, NAN, Bs)
    kind = epi & 15
    aux16 = bool(epi & CO['VITAE_EPI_AUX_BF16'])
    outs = {}
    Cb = C16 = AUX = None
    if c32:
        Cb = outs['C'] = Buf(M, N, ld.get('c'), F32, SENT, None if refused else old, init, off=c_off)
    if c16:
        C16 = outs['C16'] = Buf(M, N, ld.get('c16'), BF16, SENT, None, init)
    if kind == CO['VITAE_EPI_GELU']:
        AUX = outs['aux'] = Buf(M, N, ld.get('aux'), BF16 if aux16 else F32, SENT, None, init)
    elif aux is not None:
        AUX = Buf(M, N, ld.get('aux'), BF16 if aux16 else F32, NAN, aux)
    BIAS = None if bias is None else Buf(1, N, None, F32, NAN, bias)
    RES = None if res is None else Buf(M, N, ld.get('r'), F32, NAN, res)
    vec = lambda name, t, n: None if t is None else outs.setdefault(name, Buf(1, n, None, F32, SENT, None if refused else t, init))
    CS, RS, ACS = vec('colsum', colsum, N), vec('rowsum', rowsum, M), vec('acolsum', acolsum, K)
    if entry in ('gemm', 'x3', 'bf16'):
        ws = Workspace(dll.vitae_gemm_workspace_floats(M, N, K, split))
    else:
        ws = Workspace(dll.vitae_gemm_glds_ws_floats(M, N, split), CO['VITAE_GLDS_TICKETS'])
    wsp = None if no_ws else ws.ptr
    tail = (_p(BIAS), _p(RES), _ld(RES), epi, _p(AUX), _ld(AUX), int(old is not None), split, wsp)
    if entry == 'gemm':
        rc = dll.vitae_gemm(prec, akc, bkc, A.ptr, A.ld, B.ptr, B.ld, _p(Cb), _ld(Cb), M, N, K, *tail, st())
    elif entry == 'x3':
        rc = dll.vitae_gemm_bf16x3(akc, bkc, A.ptr, A.ld, B.ptr, B.ld, _p(Cb), _ld(Cb), M, N, K, *tail, st())
    elif entry == 'bf16':
        rc = dll.vitae_gemm_bf16(akc, bkc, A.ptr, A.ld, B.ptr, B.ld, b16, _p(Cb), _ld(Cb), M, N, K, *tail, _p(ACS), st())
    elif entry == 'wsx3':
        rc = dll.vitae_gemm_wsx3(akc, bkc, A.ptr, A.ld, B.ptr, B.ld, _p(Cb), _ld(Cb), M, N, K, *tail, _p(CS), _p(RS), st())
    elif entry == 'glds':
        rc = dll.vitae_gemm_glds(akc, bkc, A.ptr, A.ld, B.ptr, B.ld, _p(Cb), _ld(Cb), _p(C16), _ld(C16), M, N, K, *tail, _p(CS), st())
    elif entry == 'w2':
        assert form == 'fwd' and B.ld == 2 * K
        rc = dll.vitae_gemm_glds_w2(A.ptr, A.ld, B.ptr, _p(Cb), _ld(Cb), _p(C16), _ld(C16), M, N, K, *tail, _p(CS), st())
    else:
        raise ValueError(entry)
    torch.cuda.synchronize()
    assert rc == expect, (entry, form, rc, expect)
    for name, o in outs.items():
        assert o.untouched() if refused else o.clean(), f'{entry} {form}: the guards of {name} were written'
    assert ws.clean(), f'{entry} {form}: split-K workspace tickets / guards'
    return types.SimpleNamespace(rc=rc, **{k: v.cpu() for k, v in outs.items()})


def strides(form, M, N, K, v):
    """leading dimensions that all differ from the widths and from one another, multiples of the vector width v"""
    akc, bkc = FORMS[form]
    return dict(a=(K if akc else M) + v, b=(K if bkc else N) + 2 * v, c=N + 3 * v, r=N + 4 * v, aux=N + 5 * v, c16=N + 6 * v)


def exact_problem(M, N, K, seed, lim=4):
    a, b = ints((M, K), lim, seed), ints((N, K), lim, seed + 1)
    bias, res, old = ints((N,), 8, seed + 2), ints((M, N), 8, seed + 3), ints((M, N), 8, seed + 4)
    assert K * lim * lim + 24 < 2 ** 24
    prod = a.double() @ b.double().t()
    assert float(prod.abs().max()) + 24 < 2 ** 24
    return a, b, bias, res, old, prod


def exact_suite(lib, entry, form, M, N, K, splits, seed=0, vecw=4, ldc_scalar=False, **kw):
    """plain at every split, bias + residual, accumulate, all three, then all three on strided operands: the integer answer, bitwise"""
    a, b, bias, res, old, prod = exact_problem(M, N, K, seed)
    full = epilogue_ref(prod, bias, res, old).float()
    for s in splits:
        assert torch.equal(gemm_call(lib, entry, a, b, form, split=s, **kw).C, prod.float()), (entry, form, 'split', s)
    assert torch.equal(gemm_call(lib, entry, a, b, form, bias=bias, res=res, **kw).C, epilogue_ref(prod, bias, res).float())
    assert torch.equal(gemm_call(lib, entry, a, b, form, old=old, split=splits[-1], **kw).C, (prod + old.double()).float())
    assert torch.equal(gemm_call(lib, entry, a, b, form, bias=bias, res=res, old=old, **kw).C, full)
    ld = strides(form, M, N, K, vecw)
    if ldc_scalar:
        ld['c'] += 1                                        # the 64-tile fp32 family stores element by element: any ldc
    assert torch.equal(gemm_call(lib, entry, a, b, form, bias=bias, res=res, old=old, ld=ld, split=splits[-1], **kw).C, full)
    return a, b, bias, res, old, prod


def _mn(form, M, N, v=4):
    """row-contiguous operands move in groups of v rows: round that extent to v"""
    akc, bkc = FORMS[form]
    return (M if akc else (M + v - 1) // v * v), (N if bkc else (N + v - 1) // v * v)


# =========================================================================== vitae_gemm (prec 0, 1, 2) and vitae_linear_*
GEMM_SHAPES = [(60, 63, 4), (64, 64, 28), (68, 65, 32), (60, 64, 36), (64, 63, 68), (68, 65, 100), (64, 64, 132), (68, 64, 1028)]


@gpu
@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('M,N,K', GEMM_SHAPES)
def test_gemm_exact(lib, form, M, N, K):
    """vitae_gemm at every precision, layout and split: the same bits, the integer answer"""
    M, N = _mn(form, M, N)
    for prec in (0, 1, 2):
        exact_suite(lib, 'gemm', form, M, N, K, (1, 2, 3), seed=K, ldc_scalar=True, prec=prec)
    exact_suite(lib, 'x3', form, M, N, K, (1, 2), seed=K, ldc_scalar=True)


@gpu
@pytest.mark.parametrize('form', ['fwd', 'wgrad'])
def test_gemm_x3_wide_tile_exact(lib, form):
    """33 x 16 = 528 tiles of 64 x 128: gemm_bf16_kernel<64, 128, 64, X3>, through vitae_gemm at VITAE_PREC_BF16X3"""
    M, N, K = 2052, 1992, 68
    assert (M + 63) // 64 * ((N + 127) // 128) >= 512
    a, b, bias, res, old, prod = exact_problem(M, N, K, 17)
    o = gemm_call(lib, 'gemm', a, b, form, prec=2, bias=bias, res=res, old=old, split=2, ld=strides(form, M, N, K, 4))
    assert torch.equal(o.C, epilogue_ref(prod, bias, res, old).float())
    x, _, _ = hilo_operand((M, K), 18)
    y = ints((N, K), 2, 19)
    assert torch.equal(gemm_call(lib, 'gemm', x, y, form, prec=2).C, (x.double() @ y.double().t()).float())


@gpu
@pytest.mark.parametrize('M,N,K', [(60, 64, 36), (68, 60, 100)])
def test_linear_entry_points_exact(lib, M, N, K):
    dll = lib.load()
    a, w, bias, res, old, prod = exact_problem(M, N, K, 3)
    dy = ints((M, N), 4, 9)
    wsf = dll.vitae_gemm_workspace_floats
    for prec in (0, 1, 2):
        x, W, r_, DY = (Buf(t.shape[0], t.shape[1], None, F32, NAN, t) for t in (a, w, res, dy))
        b_ = Buf(1, N, None, F32, NAN, bias)
        for split in (1, 2):
            w1, w2, w3 = Workspace(wsf(M, N, K, split)), Workspace(wsf(M, K, N, split)), Workspace(wsf(N, K, M, split))
            y, dx, dw = Buf(M, N), Buf(M, K, data=ints((M, K), 8, 5)), Buf(N, K, data=ints((N, K), 8, 6))
            dx0, dw0 = dx.cpu(), dw.cpu()
            assert dll.vitae_linear_fwd(prec, x.ptr, W.ptr, b_.ptr, y.ptr, M, N, K, 0, None, r_.ptr, split, w1.ptr, st()) == 0
            assert dll.vitae_linear_bwd_input(prec, DY.ptr, W.ptr, dx.ptr, M, N, K, 0, None, 1, split, w2.ptr, st()) == 0
            assert dll.vitae_linear_bwd_weight(prec, DY.ptr, x.ptr, dw.ptr, M, N, K, 1, split, w3.ptr, st()) == 0
            torch.cuda.synchronize()
            assert y.clean() and dx.clean() and dw.clean() and w1.clean() and w2.clean() and w3.clean()
            assert torch.equal(y.cpu(), epilogue_ref(prod, bias, res).float())
            assert torch.equal(dx.cpu(), (dx0.double() + dy.double() @ w.double()).float())
            assert torch.equal(dw.cpu(), (dw0.double() + dy.double().t() @ a.double()).float())


@gpu
@pytest.mark.parametrize('entry,kw', [('gemm', dict(prec=2)), ('x3', {}), ('wsx3', {})])
@pytest.mark.parametrize('form', ['fwd', 'dgrad', 'wgrad'])
def test_two_term_operands_exact(lib, entry, kw, form):
    """hi + lo on A, then on B: hi.hi + hi.lo + lo.hi is the whole product, so the result is the exact one — a lost, doubled or
    swapped lo plane is a wrong exact value"""
    M, N, K = 68, 64, 132
    x, _, _ = hilo_operand((M, K), 12)
    y = ints((N, K), 2, 13)
    want = (x.double() @ y.double().t())
    assert float(want.abs().max()) * 2 ** 11 < 2 ** 24
    for split in (1, 2):
        assert torch.equal(gemm_call(lib, entry, x, y, form, split=split, **kw).C, want.float()), 'split on A'
    x2, _, _ = hilo_operand((N, K), 14)
    y2 = ints((M, K), 2, 15)
    assert torch.equal(gemm_call(lib, entry, y2, x2, form, **kw).C, (y2.double() @ x2.double().t()).float()), 'split on B'


@gpu
@pytest.mark.parametrize('entry,kw,path', [('gemm', dict(prec=0), 'f32'), ('gemm', dict(prec=1), 'bf16'), ('gemm', dict(prec=2), 'x3')])
@pytest.mark.parametrize('fam', FAMILIES)
@pytest.mark.parametrize('form,M,N,K', [('fwd', 68, 65, 132), ('dgrad', 60, 64, 640), ('wgrad', 64, 68, 260), ('tn', 68, 63, 100)])
def test_gemm_rounding(lib, entry, kw, path, fam, form, M, N, K):
    rounding_case(lib, entry, kw, path, fam, form, M, N, K, split=2 if K > 128 else 1)


def rounding_case(lib, entry, kw, path, fam, form, M, N, K, split=1, pre16=False, label=None, **ckw):
    """family 2 for one path: the kernel against the float64 product of the path's operand values, per element"""
    a, b, bias, res, old = family(fam, M, N, K, seed=K + M)
    if pre16:
        a = rne(a)
        if path == 'bf16':
            b = rne(b)
    label = label or f'{entry}{kw.get("prec", "")}/{form}/{fam}/{M}x{N}x{K}/s{split}'
    A, B = path_operands(path, a, b)
    got = gemm_call(lib, entry, a, b, form, bias=bias, res=res, old=old, split=split, **kw, **ckw).C
    if fam == 'small-epilogue':
        plain = gemm_call(lib, entry, a, b, form, split=split, **kw, **ckw).C
        add = epilogue_ref(torch.zeros(M, N, dtype=F64), bias, res, old)
        den = epilogue_ref(torch.zeros(M, N, dtype=F64), bias.abs(), res.abs(), old.abs())
        e = float(_ratio(((got.double() - plain.double()) - add).abs(), den).max())
        e32 = max(float(_ratio(((w.double() - wo.double()) - add).abs(), den).max())
                  for w, wo in zip(plain32(A, B, bias, res, old), plain32(A, B)))
        within(label + ' addends', e, e32)
    c64, den = gemm_ref(A, B, bias, res, old)
    e32 = max(elem_err(p, c64, den) for p in plain32(A, B, bias, res, old))
    assert e32 < E32_SANE
    within(label, elem_err(got, c64, den), e32)
    if path in ('x3', 'w2'):
        t64, tden = gemm_ref(a, b, bias, res, old)
        within(label + ' vs-true', elem_err(got, t64, tden), e32, extra=2.0 ** -16)


# =========================================================================== vitae_gemm_bf16, vitae_linear_bwd_pair_bf16
@gpu
@pytest.mark.parametrize('b16', [0, 1])
@pytest.mark.parametrize('form,M,N,K', [('fwd', 60, 63, 36), ('fwd', 68, 65, 260), ('dgrad', 64, 64, 68), ('dgrad', 68, 72, 260),
                                        ('wgrad', 60, 64, 100), ('wgrad', 68, 136, 260), ('tn', 64, 65, 64), ('fwd', 64, 72, 1028), ('fwd', 2052, 1992, 132), ('dgrad', 2052, 1992, 36)])
def test_gemm_bf16_exact(lib, b16, form, M, N, K):
    akc, bkc = FORMS[form]
    v = 8 if b16 else 4
    M, N = _mn(form, M, N, v)
    if b16 and bkc:
        K = (K + 7) // 8 * 8
    splits = (1,) if K < 128 and M > 1000 else (1, 2)          # (the wide tile's k-phase is 128: K = 132 / 136 at split 2 is 128 + 4 / 8)
    a, b, bias, res, old, prod = exact_suite(lib, 'bf16', form, M, N, K, splits, seed=K + b16, vecw=8, ldc_scalar=True, b16=b16)
    if akc and (M < 1000 or K > 128):                     # the bias gradient riding on the A tiles: exact integer column sums, added
        cs0 = ints((K,), 8, 21)
        want = cs0.double() + a.double().sum(0)
        assert float(want.abs().max()) < 2 ** 24
        for s in splits:
            o = gemm_call(lib, 'bf16', a, b, form, b16=b16, split=s, acolsum=cs0)
            assert torch.equal(o.C, prod.float()) and torch.equal(o.acolsum.view(-1), want.float()), s


@gpu
@pytest.mark.parametrize('b16', [0, 1])
@pytest.mark.parametrize('fam', FAMILIES)
@pytest.mark.parametrize('form,M,N,K', [('fwd', 68, 65, 264), ('dgrad', 60, 64, 640), ('wgrad', 64, 72, 260)])
def test_gemm_bf16_rounding(lib, b16, fam, form, M, N, K):
    M, N = _mn(form, M, N, 8)
    rounding_case(lib, 'bf16', dict(b16=b16), 'bf16', fam, form, M, N, K, split=2)


def pair_bf16_call(lib, dy, w, x, *, epi=0, aux=None, old_dx=None, old_dw=None, db0=None, expect=0):
    dll = lib.load()
    (M, N), K = dy.shape, w.shape[1]
    refused = expect != 0
    init = SENT if refused else NAN
    DY, W, X = Buf(M, N, None, F32, NAN, dy), Buf(N, K, None, BF16, NAN, w), Buf(M, K, None, F32, NAN, x)
    AUX = None if aux is None else Buf(M, K, None, F32, NAN, aux)
    dx, dw = Buf(M, K, data=None if refused else old_dx, init=init), Buf(N, K, data=None if refused else old_dw, init=init)
    db = None if db0 is None else Buf(1, N, data=None if refused else db0, init=init)
    rc = dll.vitae_linear_bwd_pair_bf16(DY.ptr, W.ptr, X.ptr, dx.ptr, dw.ptr, _p(db), M, N, K, epi, _p(AUX), int(old_dx is not None),
                                        int(old_dw is not None), st())
    torch.cuda.synchronize()
    assert rc == expect
    for o in (dx, dw, db):
        assert o is None or (o.untouched() if refused else o.clean())
    return types.SimpleNamespace(dx=dx.cpu(), dw=dw.cpu(), db=None if db is None else db.cpu().view(-1))


def pair_family(fam, M, N, K, seed):
    """dy [M, N], w [N, K] (bf16 values), x [M, K] of a Linear's backward in the families above"""
    g = torch.Generator().manual_seed(seed)
    dy, w, x = torch.randn(M, N, generator=g), torch.randn(N, K, generator=g), torch.randn(M, K, generator=g)
    if fam == 'scales':
        dy = dy * (10.0 ** (torch.rand(M, generator=g) * 6 - 3))[:, None]
        x = x * (10.0 ** (torch.rand(K, generator=g) * 6 - 3))[None, :]
        w = w * (10.0 ** (torch.rand(K, generator=g) * 6 - 3))[None, :]
    if fam == 'cancel':
        dy = 1.0 + 0.01 * dy
        w = w - w.mean(0, keepdim=True)
        x = x - x.mean(0, keepdim=True)
    return dy, rne(w), x


def pair_cfgs(M, N, K):
    """pick_cfg of gemm_bf16.hip for the two halves: 2 (64 x 128 x 128) from 512 tiles of 64 x 128, else 1 (64 x 64 x 256)"""
    cfg = lambda m, n: 2 if n >= 128 and ((m + 63) // 64) * ((n + 127) // 128) >= 512 else 1
    return cfg(M, K), cfg(N, K)


# (M, N, K) -> the instantiation of gemm_bf16_pair_kernel: <64x64x256, 64x64x256> at the small shapes; 2052 x 1992 is 33 x 16 = 528
# tiles of 64 x 128, so (2052, 8, 1992) is <64x128x128, 64x64x256>, (8, 2056, 1992) <64x64x256, 64x128x128>, (2052, 2056, 1992) both wide
PAIR_BF16_SHAPES = [((60, 64, 72), (1, 1)), ((68, 72, 64), (1, 1)), ((100, 136, 56), (1, 1)), ((260, 8, 264), (1, 1)),
                    ((2052, 8, 1992), (2, 1)), ((8, 2056, 1992), (1, 2)), ((2052, 2056, 1992), (2, 2))]


@gpu
@pytest.mark.parametrize('shape,cfgs', PAIR_BF16_SHAPES)
def test_linear_bwd_pair_bf16_exact(lib, C, shape, cfgs):
    M, N, K = shape
    assert pair_cfgs(M, N, K) == cfgs
    dy, w, x = ints((M, N), 4, 31), ints((N, K), 4, 32), ints((M, K), 4, 33)
    odx, odw, db0 = ints((M, K), 8, 34), ints((N, K), 8, 35), ints((N,), 8, 36)
    dxw, dww = dy.double() @ w.double(), dy.double().t() @ x.double()
    assert max(M, N) * 16 + 24 < 2 ** 24 and float(dy.double().sum(0).abs().max()) + 8 < 2 ** 24
    o = pair_bf16_call(lib, dy, w, x, db0=db0)
    assert torch.equal(o.dx, dxw.float()) and torch.equal(o.dw, dww.float())
    assert torch.equal(o.db, (db0.double() + dy.double().sum(0)).float())
    o = pair_bf16_call(lib, dy, w, x, old_dx=odx, old_dw=odw)
    assert torch.equal(o.dx, (dxw + odx).float()) and torch.equal(o.dw, (dww + odw).float())
    mask = ints((M, K), 2, 37)
    o = pair_bf16_call(lib, dy, w, x, epi=C['VITAE_EPI_RELU_MASK'], aux=mask, db0=db0)
    assert torch.equal(o.dx, torch.where(mask > 0, dxw.float(), torch.zeros(()))) and torch.equal(o.dw, dww.float())
    assert torch.equal(o.db, (db0.double() + dy.double().sum(0)).float())
    s = gelu_scale(N)
    h = ints((M, K), 24, 38) / 8
    o = pair_bf16_call(lib, dy, w * s, x, epi=C['VITAE_EPI_DGELU'], aux=h)
    gelu_checks(f'pair_bf16 {M}x{N}x{K}', h, dgelu=o.dx, acc=(dxw * s).float())
    assert torch.equal(o.dw, dww.float())


@gpu
@pytest.mark.parametrize('fam', ['plain', 'scales', 'cancel'])
@pytest.mark.parametrize('shape,cfgs', [((132, 136, 72), (1, 1)), ((2052, 8, 1992), (2, 1)), ((8, 2056, 1992), (1, 2))])
def test_linear_bwd_pair_bf16_rounding(lib, fam, shape, cfgs):
    """the mixed instantiations carry the wide half at a reduction of 8 (dx of the first, dw of the second) and the 64 x 64 half at
    2052 / 2056: both halves of both are measured"""
    M, N, K = shape
    assert pair_cfgs(M, N, K) == cfgs
    dy, w, x = pair_family(fam, M, N, K, 41)
    o = pair_bf16_call(lib, dy, w, x)
    for name, got, (A, B) in (('dx', o.dx, path_operands('bf16', dy, w.t().contiguous())),
                              ('dw', o.dw, path_operands('bf16', dy.t().contiguous(), x.t().contiguous()))):
        c64, den = gemm_ref(A, B)
        within(f'pair_bf16/{cfgs[0]}{cfgs[1]}/{name}/{fam}', elem_err(got, c64, den), *(elem_err(p, c64, den) for p in plain32(A, B)))


# =========================================================================== vitae_gemm_wsx3
@gpu
@pytest.mark.parametrize('form', ['fwd', 'dgrad', 'wgrad'])
@pytest.mark.parametrize('M,N,K', [(8, 8, 4), (60, 64, 60), (64, 68, 64), (68, 60, 68), (132, 72, 132), (68, 64, 1028)])
def test_gemm_wsx3_exact(lib, form, M, N, K):
    a, b, bias, res, old, prod = exact_suite(lib, 'wsx3', form, M, N, K, (1, 2, 4), seed=K)
    cs0, rs0 = ints((N,), 8, 51), ints((M,), 8, 52)
    for split in (1, 2):
        o = gemm_call(lib, 'wsx3', a, b, form, bias=bias, res=res, split=split, colsum=cs0, rowsum=rs0 if form == 'wgrad' else None)
        want = epilogue_ref(prod, bias, res)
        assert torch.equal(o.C, want.float()) and torch.equal(o.colsum.view(-1), (cs0.double() + want.sum(0)).float())
        if form == 'wgrad':
            assert torch.equal(o.rowsum.view(-1), (rs0.double() + a.double().sum(1)).float())


@gpu
@pytest.mark.parametrize('fam', FAMILIES)
@pytest.mark.parametrize('form,M,N,K,split', [('fwd', 68, 72, 132, 1), ('dgrad', 60, 64, 640, 4), ('wgrad', 64, 68, 260, 2)])
def test_gemm_wsx3_rounding(lib, fam, form, M, N, K, split):
    rounding_case(lib, 'wsx3', {}, 'x3', fam, form, M, N, K, split=split)


# =========================================================================== vitae_gemm_glds: the 64-row family
def glds_exact(lib, form, M, N, K, splits, seed=0, ld=None, c_off=0, check16=True):
    """the LDS-DMA entry point on integer operands: plain at every split, the bf16 copy (alone and beside C), bias + residual +
    accumulate + column sums — all the integer answer"""
    a, b, bias, res, old, prod = exact_problem(M, N, K, seed)
    kw = dict(ld=ld, c_off=c_off)
    for s in splits:
        assert torch.equal(gemm_call(lib, 'glds', a, b, form, split=s, **kw).C, prod.float()), (form, 'split', s)
    cs0 = ints((N,), 8, seed + 7)
    full = epilogue_ref(prod, bias, res, old)
    assert float(full.sum(0).abs().max()) + 8 < 2 ** 24
    o = gemm_call(lib, 'glds', a, b, form, bias=bias, res=res, old=old, colsum=cs0, c16=check16, split=splits[-1], **kw)
    assert torch.equal(o.C, full.float()) and torch.equal(o.colsum.view(-1), (cs0.double() + full.sum(0)).float())
    if check16:
        assert torch.equal(o.C16, o.C.to(BF16))
        o2 = gemm_call(lib, 'glds', a, b, form, bias=bias, res=res, c32=False, c16=True, **kw)
        assert torch.equal(o2.C16, epilogue_ref(prod, bias, res).float().to(BF16))
    return a, b, bias, res, old, prod


@gpu
@pytest.mark.parametrize('how,form', [('N%4', 'fwd'), ('ldc%4', 'fwd'), ('ldc%4', 'dgrad'), ('ldc%4', 'wgrad'), ('C+4B', 'fwd'), ('C+4B', 'dgrad'),
                                      ('C+4B', 'wgrad')])
def test_gemm_glds_scalar_epilogue_exact(lib, bt_mode, how, form):
    """vec_epilogue_ok fails -> the 64-row family's element-by-element epilogue, even under a forced big tile.  One trigger at a
    time (Buf keeps every rectangle on a 16-byte boundary): N = 70 with every ld a multiple of 8 (N % 4 != 0 needs a k-contiguous B:
    a row-contiguous one moves 8 columns at a time); ldc = N + 26 with N % 4 == 0, every other ld a multiple of 8 and an aligned C;
    a C four bytes past the boundary with ld == width."""
    M, N, K = 72, (70 if how == 'N%4' else 72), 192
    ld = strides(form, M, N, K, 8)
    if how == 'N%4':
        ld.update(c=96, r=104, aux=112, c16=120)
    if how == 'ldc%4':
        ld['c'] += 2
    assert all(v % 8 == 0 for k, v in ld.items() if not (how == 'ldc%4' and k == 'c'))
    bt_mode(5)
    glds_exact(lib, form, M, N, K, (1, 3), seed=61, ld=ld if how != 'C+4B' else None, c_off=1 if how == 'C+4B' else 0)


@gpu
@pytest.mark.parametrize('form', ['fwd', 'dgrad', 'wgrad'])
@pytest.mark.parametrize('M,N,K', [(56, 64, 64), (64, 72, 128), (72, 56, 192), (136, 136, 320)])
def test_gemm_glds_64_row_family_exact(lib, bt_mode, form, M, N, K):
    """mode -2: forward form on gemm_glds_pipe_kernel (<= 512 workgroups), the others on the 64 x 64 kernel; K = 64, 128, 192;
    split 3 of K = 192 is three parts of one k-tile, split 2 of K = 320 is 192 + 128: a last part of exactly two k-tiles"""
    bt_mode(-2)
    akc, bkc = FORMS[form]
    assert lib.load().vitae_gemm_glds_bt_choice(akc, bkc, M, N, K) == -1
    glds_exact(lib, form, M, N, K, (1, 2, 3), seed=K + M)
    glds_exact(lib, form, M, N, K, (2,), seed=K + M + 1, ld=strides(form, M, N, K, 8))


@gpu
@pytest.mark.parametrize('form', ['fwd', 'dgrad', 'wgrad'])
@pytest.mark.parametrize('K,split', [(64, 1), (128, 2), (192, 2), (192, 3)])
def test_gemm_glds_64x128_kernel_exact(lib, bt_mode, form, K, split):
    """20 x 20 = 400 tiles of 64 x 128; one k-tile, two parts of one, 128 + 64 and three parts of one"""
    M, N = 1280, 2560
    bt_mode(-2)
    akc, bkc = FORMS[form]
    assert (M + 63) // 64 * ((N + 127) // 128) >= 400 and lib.load().vitae_gemm_glds_bt_choice(akc, bkc, M, N, K) == -1
    a, b, bias, res, old, prod = exact_problem(M, N, K, 71 + K)
    o = gemm_call(lib, 'glds', a, b, form, bias=bias, res=res, old=old, c16=True, split=split)
    assert torch.equal(o.C, epilogue_ref(prod, bias, res, old).float()) and torch.equal(o.C16, o.C.to(BF16))


# =========================================================================== vitae_gemm_glds: forced big tiles
TILE_DIMS = {0: (256, 256), 3: (128, 128), 4: (128, 128), 5: (64, 64), 6: (128, 256)}


def k_for_split(dll, akc, bkc, M, N, tile, want):
    """the shortest reduction at which the planner cuts (M, N) `want` ways on the forced tile"""
    for K in range(128, 4097, 64):
        if dll.vitae_gemm_glds_bt_choice(akc, bkc, M, N, K) == tile and dll.vitae_gemm_glds_pick_split_k_form(akc, bkc, M, N, K) == want:
            return K
    return None


TILE_FORMS = [(t, f) for t in (0, 3, 4, 5) for f in ('fwd', 'dgrad', 'wgrad')] + [(6, 'wgrad')]      # tile 6: the weight-gradient form only


@gpu
def test_tile_6_serves_the_weight_gradient_form_only(lib, bt_mode):
    bt_mode(6)
    dll = lib.load()
    assert dll.vitae_gemm_glds_bt_choice(1, 1, 264, 520, 192) == -1 and dll.vitae_gemm_glds_bt_choice(1, 0, 264, 520, 192) == -1
    assert dll.vitae_gemm_glds_bt_choice(0, 0, 264, 520, 192) == 6
    glds_exact(lib, 'fwd', 264, 520, 192, (1,), seed=6)            # served all the same: by the 64-row family


@gpu
@pytest.mark.parametrize('tile,form', TILE_FORMS)
@pytest.mark.parametrize('tiles', [1, 7, 9])
def test_gemm_glds_forced_tile_exact(lib, bt_mode, tile, form, tiles):
    dll = lib.load()
    akc, bkc = FORMS[form]
    bm, bn = TILE_DIMS[tile]
    M, N = {1: (bm - 8, bn), 7: (bm, 7 * bn - 8), 9: (2 * bm + 8, 2 * bn + 8)}[tiles]
    bt_mode(tile)
    assert ((M + bm - 1) // bm) * ((N + bn - 1) // bn) == tiles
    for K in (128, 192):
        assert dll.vitae_gemm_glds_bt_choice(akc, bkc, M, N, K) == tile and dll.vitae_gemm_glds_pick_split_k_form(akc, bkc, M, N, K) == 1
        glds_exact(lib, form, M, N, K, (1,), seed=tile + K, ld=strides(form, M, N, K, 8) if K == 192 else None)


@gpu
@pytest.mark.parametrize('tile,form', [tf for tf in TILE_FORMS if tf[0] != 0])      # (tile 0 has no split-K)
@pytest.mark.parametrize('split', [2, 3])
def test_gemm_glds_forced_tile_split_exact(lib, bt_mode, tile, form, split):
    """in-launch split-K of the big tiles, at the reduction length where the planner itself wants that split (any other split
    would be served by the 64-row family); the same bits as the unsplit 64-row launch"""
    dll = lib.load()
    akc, bkc = FORMS[form]
    bm, bn = TILE_DIMS[tile]
    bt_mode(tile)
    # one tile: the cost model goes from 1 straight to 3; it stops at 2 where a third part would need a second round of workgroups
    # (10 x 10 tiles on the 256 slots of tiles 4 - 6, 13 x 14 on the 512 of tile 3 and on tile 5's two per CU)
    for M, N in ((bm + 8, bn - 8), (10 * bm - 8, 10 * bn), (13 * bm - 8, 14 * bn)):
        K = k_for_split(dll, akc, bkc, M, N, tile, split)
        if K is not None:
            break
    assert K is not None, 'the planner never asks for this split under the forced tile'
    a, b, bias, res, old, prod = glds_exact(lib, form, M, N, K, (split,), seed=tile + split)
    bt_mode(-2)
    assert torch.equal(gemm_call(lib, 'glds', a, b, form).C, prod.float())


GLDS_ROUNDING_SHAPES = {'fwd': (136, 120, 192), 'dgrad': (120, 136, 640), 'wgrad': (136, 136, 256)}


@gpu
@pytest.mark.parametrize('tile,form', [(-2, f) for f in GLDS_ROUNDING_SHAPES] + TILE_FORMS)
@pytest.mark.parametrize('fam', FAMILIES)
def test_gemm_glds_rounding(lib, bt_mode, tile, fam, form):
    dll = lib.load()
    M, N, K = GLDS_ROUNDING_SHAPES[form]
    akc, bkc = FORMS[form]
    bt_mode(tile)
    assert dll.vitae_gemm_glds_bt_choice(akc, bkc, M, N, K) == (tile if tile >= 0 else -1)
    split = dll.vitae_gemm_glds_pick_split_k_form(akc, bkc, M, N, K)
    rounding_case(lib, 'glds', {}, 'bf16', fam, form, M, N, K, split=split, pre16=True, label=f'glds/t{tile}/{form}/{fam}/s{split}')


# =========================================================================== epilogues of every entry point
EPI_ENTRIES = [('gemm', dict(prec=0), False), ('gemm', dict(prec=1), False), ('gemm', dict(prec=2), False), ('bf16', dict(b16=1), False),
               ('wsx3', {}, False), ('glds', {}, True), ('w2', {}, True)]


@gpu
@pytest.mark.parametrize('entry,kw,has16', EPI_ENTRIES)
@pytest.mark.parametrize('M,N,K', [(68, 72, 128), (60, 136, 192)])
def test_epilogues_on_exact_preactivations(lib, C, bt_mode, entry, kw, has16, M, N, K):
    GELU, DGELU, MASK, RELU = C['VITAE_EPI_GELU'], C['VITAE_EPI_DGELU'], C['VITAE_EPI_RELU_MASK'], C['VITAE_EPI_RELU']
    A16, DV = C['VITAE_EPI_AUX_BF16'], C['VITAE_EPI_AUX_DERIV']
    a, b, bias, res, old, prod = exact_problem(M, N, K, 81)
    s = gelu_scale(K)
    bs, biass = b * s, bias / 8
    pre = (prod * s + biass.double()).float()
    acc = (prod * s).float()
    lab = f'{entry}{kw.get("prec", "")} {M}x{N}x{K}'
    ld = strides('fwd', M, N, K, 8)
    if entry == 'w2':
        ld.pop('b')
    o = gemm_call(lib, entry, a, bs, bias=biass, epi=GELU, ld=ld, **kw)
    assert torch.equal(o.aux, pre), 'the saved pre-activation is the exact value'
    gelu_checks(lab, pre, y=o.C)
    od = gemm_call(lib, entry, a, bs, bias=biass, epi=GELU | DV, **kw)
    assert torch.equal(od.C, o.C), 'AUX_DERIV leaves the forward output alone'
    gelu_checks(lab + ' saved', pre, dsaved=od.aux)
    h = ints((M, N), 24, 82) / 8
    gelu_checks(lab, h, dgelu=gemm_call(lib, entry, a, bs, epi=DGELU, aux=h, ld=ld, **kw).C, acc=acc)
    assert torch.equal(gemm_call(lib, entry, a, bs, epi=DGELU | DV, aux=h, **kw).C, (acc.double() * h.double()).float())
    assert torch.equal(gemm_call(lib, entry, a, bs, epi=MASK, aux=h, res=res, **kw).C,
                       (torch.where(h > 0, acc, torch.zeros(())).double() + res).float())
    if has16:
        assert torch.equal(gemm_call(lib, entry, a, bs, bias=biass, epi=RELU, **kw).C, pre.clamp_min(0))
        both = gemm_call(lib, entry, a, bs, bias=biass, epi=GELU | A16, c16=True, ld=ld, **kw)
        assert torch.equal(both.aux, pre.to(BF16)) and torch.equal(both.C16, both.C.to(BF16))
        gelu_checks(lab + ' with-c16', pre, y=both.C)
        o16 = gemm_call(lib, entry, a, bs, bias=biass, epi=GELU | A16, c32=False, c16=True, ld=ld, **kw)
        assert torch.equal(o16.aux, pre.to(BF16)) and torch.equal(o16.C16, both.C16), 'the bf16 output alone: the bits of the call that asks for both'
        od16 = gemm_call(lib, entry, a, bs, bias=biass, epi=GELU | A16 | DV, c16=True, **kw)
        assert torch.equal(od16.C, both.C) and torch.equal(od16.C16, both.C16)
        h16 = rne(h)
        gelu_checks(lab + ' aux16', h16, dgelu=gemm_call(lib, entry, a, bs, epi=DGELU | A16, aux=h16, **kw).C, acc=acc)
        if entry == 'glds':
            for tile in (3, 4, 5, 0):
                bt_mode(tile)
                assert lib.load().vitae_gemm_glds_bt_choice(1, 1, M, N, K) == tile
                t = gemm_call(lib, entry, a, bs, bias=biass, epi=GELU, c16=True, ld=ld)
                assert torch.equal(t.aux, pre) and torch.equal(t.C16, t.C.to(BF16))
                gelu_checks(f'{lab} tile {tile}', pre, y=t.C)
                gelu_checks(f'{lab} tile {tile}', h, dgelu=gemm_call(lib, entry, a, bs, epi=DGELU, aux=h).C, acc=acc)
                assert torch.equal(gemm_call(lib, entry, a, bs, bias=biass, epi=RELU, res=res).C, (pre.clamp_min(0).double() + res).float())


# =========================================================================== vitae_gemm_glds_w2, vitae_cast_bf16(_hilo)
@gpu
@pytest.mark.parametrize('tile', [-1, 3, 4, 0])
@pytest.mark.parametrize('M,N,K', [(72, 136, 128), (136, 120, 192), (264, 264, 512)])
def test_gemm_glds_w2_exact_and_rounding(lib, bt_mode, tile, M, N, K):
    """few rows: the two-plane 64 x 64 workgroup (the planner's tile 5 / none); a forced big tile: the reduction over 2 K"""
    dll = lib.load()
    bt_mode(tile)
    route = dll.vitae_gemm_glds_bt_choice(1, 1, M, N, 2 * K)
    assert route == tile if tile >= 0 else route in (5, -1)
    split = dll.vitae_gemm_glds_w2_pick_split_k(M, N, K)
    x = ints((M, K), 2, 91)
    w, hi, lo = hilo_operand((N, K), 92)
    bias, res, old, cs0 = ints((N,), 8, 93), ints((M, N), 8, 94), ints((M, N), 8, 95), ints((N,), 8, 96)
    want = x.double() @ w.double().t()
    assert float(want.abs().max()) * 2 ** 11 < 2 ** 24 and K <= 512
    ld = dict(a=K + 8, c=N + 4, r=N + 8, c16=N + 16)
    for sp in {1, split} | ({2} if K >= 256 else set()):
        assert torch.equal(gemm_call(lib, 'w2', x, w, split=sp).C, want.float()), ('two-plane product', sp)
    o = gemm_call(lib, 'w2', x, w, bias=bias, res=res, old=old, c16=True, split=split, ld=ld)
    assert torch.equal(o.C, epilogue_ref(want, bias, res, old).float()) and torch.equal(o.C16, o.C.to(BF16))
    full = epilogue_ref(x.double() @ hi.double().t(), bias, res, old)          # integer weights: the column sums are exact in any order
    o = gemm_call(lib, 'w2', x, hi, bias=bias, res=res, old=old, colsum=cs0, split=split)
    assert torch.equal(o.C, full.float()) and torch.equal(o.colsum.view(-1), (cs0.double() + full.sum(0)).float())
    for fam in FAMILIES:
        rounding_case(lib, 'w2', {}, 'w2', fam, 'fwd', M, N, K, split=split, pre16=True, label=f'w2/t{tile}/{fam}/{M}x{N}x{K}/s{split}')


@gpu
@pytest.mark.parametrize('n', [1, 3, 4, 1021, 4100])
def test_cast_bf16_bitwise(lib, n):
    dll = lib.load()
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * 10.0 ** (torch.rand(n, generator=g) * 8 - 4)
    ties = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -1 - 2.0 ** -8, 2.0 ** -130, 0.0, -0.0, 3.3895314e38, 1 + 2.0 ** -8 + 2.0 ** -20])
    x[:min(n, len(ties))] = ties[:n]
    ld = (n + 7) // 8 * 8                                  # the guard row in front keeps the arrays 16-byte aligned
    src, dst = Buf(1, n, ld, F32, NAN, x), Buf(1, n, ld, BF16)
    assert dll.vitae_cast_bf16(src.ptr, dst.ptr, n, st()) == 0
    torch.cuda.synchronize()
    assert dst.clean() and torch.equal(dst.cpu().view(-1).view(torch.int16), x.to(BF16).view(torch.int16))


@gpu
@pytest.mark.parametrize('rows,K,count,gap', [(5, 4, 1, 0), (33, 68, 3, 8), (64, 128, 2, 1024)])
def test_cast_bf16_hilo_bitwise(lib, rows, K, count, gap):
    dll = lib.load()
    stride = rows * K + gap
    g = torch.Generator().manual_seed(rows)
    x = torch.full((count * stride,), NAN)
    hi_want, lo_want = [], []
    for t in range(count):
        w = torch.randn(rows, K, generator=g)
        if t == 0:
            w, _, _ = hilo_operand((rows, K), 97)
            w[0, 0] = 1 + 2.0 ** -8
        x[t * stride:t * stride + rows * K] = w.reshape(-1)
        hi_want.append(w.to(BF16))
        lo_want.append((w - w.to(BF16).float()).to(BF16))
    src, dst = Buf(1, count * stride, None, F32, NAN, x), Buf(count * rows, 2 * K, None, BF16)
    assert dll.vitae_cast_bf16_hilo(src.ptr, dst.ptr, rows, K, stride, count, st()) == 0
    torch.cuda.synchronize()
    out = dst.cpu().view(count, rows, 2 * K)
    assert dst.clean()
    assert torch.equal(out[:, :, :K].view(torch.int16), torch.stack(hi_want).view(torch.int16))
    assert torch.equal(out[:, :, K:].view(torch.int16), torch.stack(lo_want).view(torch.int16))
    hx, hh, hl = hilo_operand((rows, K), 97)
    assert torch.equal(out[0, 1:, :K].float(), hh[1:]) and torch.equal(out[0, 1:, K:].float(), hl[1:])


# =========================================================================== vitae_linear_bwd_pair_glds, vitae_wgrad_group_bt
def pad_rows(t, rows):
    return torch.cat([t, torch.zeros(max(rows - t.shape[0], 0), t.shape[1])], 0)


def pair_glds_call(lib, dy, w, x, Mpad, *, epi=0, aux=None, dx32=True, dx16=False, dw=True, dw16=False, old_dx=None, old_dw=None,
                   dxcs0=None, dycs0=None, split=1, ws_for=None, expect=0):
    """dy [M, N], w [N, K], x [M, K] (bf16-exact CPU values); rows M .. Mpad - 1 of the operands are zero, what follows is NaN"""
    dll = lib.load()
    CO = CONSTS
    (M, N), K = dy.shape, w.shape[1]
    refused = expect != 0
    init = SENT if refused else NAN
    pad = lambda t: torch.cat([t, torch.zeros(max(Mpad - M, 0), t.shape[1])], 0)
    DY, W, X = Buf(max(Mpad, M), N, None, BF16, NAN, pad(dy)), Buf(N, K, None, BF16, NAN, w), Buf(max(Mpad, M), K, None, BF16, NAN, pad(x))
    aux16 = bool(epi & CO['VITAE_EPI_AUX_BF16'])
    AUX = None if aux is None else Buf(M, K, None, BF16 if aux16 else F32, NAN, aux)
    outs = {}
    mk = lambda name, on, r, c, dt, data: outs.setdefault(name, Buf(r, c, None, dt, SENT, None if refused else data, init)) if on else None
    DX, DX16 = mk('dx', dx32, M, K, F32, old_dx), mk('dx16', dx16, M, K, BF16, None)
    DW, DW16 = mk('dw', dw, N, K, F32, old_dw), mk('dw16', dw16, N, K, BF16, None)
    DXCS, DYCS = mk('dxcs', dxcs0 is not None, 1, K, F32, dxcs0), mk('dycs', dycs0 is not None, 1, N, F32, dycs0)
    wm, wn, wsp = ws_for or (M, K, split)
    ws = Workspace(dll.vitae_gemm_glds_ws_floats(wm, wn, wsp), CO['VITAE_GLDS_TICKETS'])
    rc = dll.vitae_linear_bwd_pair_glds(DY.ptr, W.ptr, X.ptr, _p(DX), _p(DX16), _p(DW), _p(DW16), M, Mpad, N, K, epi, _p(AUX), _p(DXCS), _p(DYCS),
                                        int(old_dx is not None), int(old_dw is not None), split, ws.ptr, ws.n, st())
    torch.cuda.synchronize()
    assert rc == expect, (rc, expect)
    for name, o in outs.items():
        assert o.untouched() if refused else o.clean(), f'pair_glds: the guards of {name} were written'
    assert ws.clean()
    return types.SimpleNamespace(**{k: v.cpu() for k, v in outs.items()})


def pair_exact(lib, C, M, Mpad, N, K, seed=0):
    """every output of the paired backward on integer operands; -> the plain call's outputs (for cross-route bit equality)"""
    dll = lib.load()
    dy, w, x = ints((M, N), 4, seed + 1), ints((N, K), 4, seed + 2), ints((M, K), 4, seed + 3)
    odx, odw, cs0, ycs0 = ints((M, K), 8, seed + 4), ints((N, K), 8, seed + 5), ints((K,), 8, seed + 6), ints((N,), 8, seed + 7)
    dxw, dww = dy.double() @ w.double(), dy.double().t() @ x.double()
    assert max(M, N) * 16 + 24 < 2 ** 24
    split = dll.vitae_linear_bwd_pair_pick_split_k(M, Mpad, N, K)
    o = pair_glds_call(lib, dy, w, x, Mpad, dx16=True, dw16=True, dxcs0=cs0, dycs0=ycs0, split=split)
    assert torch.equal(o.dx, dxw.float()) and torch.equal(o.dw, dww.float())
    assert torch.equal(o.dx16, o.dx.to(BF16)) and torch.equal(o.dw16, o.dw.to(BF16))
    assert torch.equal(o.dxcs.view(-1), (cs0.double() + dxw.sum(0)).float()) and torch.equal(o.dycs.view(-1), (ycs0.double() + dy.double().sum(0)).float())
    a = pair_glds_call(lib, dy, w, x, Mpad, old_dx=odx, old_dw=odw, dw16=True, split=split)
    assert torch.equal(a.dx, (dxw + odx).float()) and torch.equal(a.dw, (dww + odw).float()) and torch.equal(a.dw16, a.dw.to(BF16))
    only16 = pair_glds_call(lib, dy, w, x, Mpad, dx32=False, dx16=True, split=split)
    assert torch.equal(only16.dx16, o.dx16) and torch.equal(only16.dw, o.dw)
    nodw = pair_glds_call(lib, dy, w, x, Mpad, dw=False, dx16=True, dxcs0=cs0, split=split)
    assert torch.equal(nodw.dx, o.dx) and torch.equal(nodw.dx16, o.dx16) and torch.equal(nodw.dxcs, o.dxcs)
    if N >= 256:                                          # a forced split of the input gradient's reduction
        f = pair_glds_call(lib, dy, w, x, Mpad, split=2, dxcs0=cs0)
        assert torch.equal(f.dx, o.dx) and torch.equal(f.dw, o.dw) and torch.equal(f.dxcs, o.dxcs)
    mask = ints((M, K), 2, seed + 8)
    m = pair_glds_call(lib, dy, w, x, Mpad, epi=C['VITAE_EPI_RELU_MASK'], aux=mask, split=split)
    assert torch.equal(m.dx, torch.where(mask > 0, dxw.float(), torch.zeros(()))) and torch.equal(m.dw, o.dw)
    s = gelu_scale(N)
    h = ints((M, K), 24, seed + 9) / 8
    d = pair_glds_call(lib, dy, w * s, x, Mpad, epi=C['VITAE_EPI_DGELU'], aux=h, dx16=True, split=split)
    gelu_checks(f'pair_glds {M}/{Mpad}x{N}x{K}', h, dgelu=d.dx, acc=(dxw * s).float())
    assert torch.equal(d.dx16, d.dx.to(BF16)) and torch.equal(d.dw, dww.float())
    return o


@gpu
@pytest.mark.parametrize('M,Mpad,N,K', [(8, 64, 128, 72), (100, 128, 128, 136), (128, 128, 256, 64), (136, 192, 320, 72), (100, 256, 128, 72)])
def test_linear_bwd_pair_glds_exact(lib, C, bt_mode, M, Mpad, N, K):
    """the single-launch routes: mode -1 and mode -2 (the 64-row pair kernel) give the same bits, the integer answer; Mpad =
    ceil64(M) and one Mpad = M + 156 (zero rows, then NaN).  Asserted of mode -1: neither half is planned on a big tile (so the
    two-launch route is out).  ASSUMED, the library has no query for it: that the launch is then gemm_ws64_pair_kernel."""
    dll = lib.load()
    assert dll.vitae_gemm_glds_bt_choice(1, 0, M, K, N) in (5, -1) and dll.vitae_gemm_glds_bt_choice(0, 0, N, K, Mpad) in (5, -1)
    o1 = pair_exact(lib, C, M, Mpad, N, K, seed=M)
    bt_mode(-2)
    o2 = pair_exact(lib, C, M, Mpad, N, K, seed=M)
    assert all(torch.equal(getattr(o1, k), getattr(o2, k)) for k in ('dx', 'dw', 'dx16', 'dw16', 'dxcs', 'dycs'))


@gpu
@pytest.mark.parametrize('tile', [0, 3, 4, 5])
@pytest.mark.parametrize('M,Mpad,N,K', [(100, 128, 128, 136), (136, 192, 256, 264)])
def test_linear_bwd_pair_glds_forced_tiles_exact(lib, C, bt_mode, tile, M, Mpad, N, K):
    """a forced tile sends the halves out as two launches through the planner of vitae_gemm_glds (tile 5: one launch)"""
    dll = lib.load()
    bt_mode(tile)
    assert dll.vitae_gemm_glds_bt_choice(1, 0, M, K, N) == tile and dll.vitae_gemm_glds_bt_choice(0, 0, N, K, Mpad) == tile
    pair_exact(lib, C, M, Mpad, N, K, seed=tile + M)


@gpu
@pytest.mark.parametrize('tile', [3, 4, 5])
def test_linear_bwd_pair_glds_planned_dgrad_split(lib, bt_mode, tile):
    """with a workspace that has room, the pair's planner cuts the input gradient's long reduction itself (3 ways at N = 1536 on
    these tiles: asserted through the same planner), whatever split the caller passes; the same bits as without a workspace"""
    dll = lib.load()
    M, Mpad, N, K = 100, 128, 1536, 136
    bt_mode(tile)
    assert dll.vitae_gemm_glds_bt_choice(1, 0, M, K, N) == tile and dll.vitae_gemm_glds_pick_split_k_form(1, 0, M, K, N) == 3
    dy, w, x = ints((M, N), 4, 171), ints((N, K), 4, 172), ints((M, K), 4, 173)
    cs0 = ints((K,), 8, 174)
    dxw, dww = dy.double() @ w.double(), dy.double().t() @ x.double()
    split = dll.vitae_linear_bwd_pair_pick_split_k(M, Mpad, N, K)
    for ws_for in ((M, K, 8), (M, K, 1)):
        o = pair_glds_call(lib, dy, w, x, Mpad, dx16=True, dxcs0=cs0, split=split if ws_for[2] > 1 else 1, ws_for=ws_for)
        assert torch.equal(o.dx, dxw.float()) and torch.equal(o.dw, dww.float()) and torch.equal(o.dx16, o.dx.to(BF16))
        assert torch.equal(o.dxcs.view(-1), (cs0.double() + dxw.sum(0)).float())


@gpu
@pytest.mark.parametrize('mode', [-1, -2, 3])
@pytest.mark.parametrize('fam', ['plain', 'scales', 'cancel'])
def test_linear_bwd_pair_glds_rounding(lib, bt_mode, mode, fam):
    M, Mpad, N, K = 132, 192, 320, 136
    bt_mode(mode)
    dy, w, x = (rne(t) for t in pair_family(fam, M, N, K, 43))
    split = lib.load().vitae_linear_bwd_pair_pick_split_k(M, Mpad, N, K)
    o = pair_glds_call(lib, dy, w, x, Mpad, split=split)
    for name, got, (A, B) in (('dx', o.dx, (dy.double(), w.t().double())), ('dw', o.dw, (dy.t().double(), x.t().double()))):
        c64, den = gemm_ref(A, B)
        within(f'pair_glds/m{mode}/{name}/{fam}', elem_err(got, c64, den), *(elem_err(p, c64, den) for p in plain32(A, B)))


def group_call(lib, dys, xs, M, Mpad, *, olds=None, want16=True, colsums=None, ws_floats=0, expect=0):
    dll = lib.load()
    CO = CONSTS
    n = len(dys)
    refused = expect != 0
    init = SENT if refused else NAN
    rows = max(M, Mpad)
    DY = [Buf(rows, t.shape[1], None, BF16, NAN, pad_rows(t, rows)) for t in dys]
    X = [Buf(rows, t.shape[1], None, BF16, NAN, pad_rows(t, rows)) for t in xs]
    DW = [Buf(dys[i].shape[1], xs[i].shape[1], data=None if olds is None or refused else olds[i], init=init) for i in range(n)]
    D16 = [Buf(dys[i].shape[1], xs[i].shape[1], None, BF16, init=init) for i in range(n)] if want16 else None
    CS = None if colsums is None else [Buf(1, dys[i].shape[1], data=None if refused else colsums[i], init=init) for i in range(n)]
    ws = Workspace(ws_floats, CO['VITAE_GLDS_TICKETS'])
    arr = lambda bs: None if bs is None else np.array([b.ptr for b in bs], dtype=np.uint64)
    ptrs = [arr(DY), arr(X), arr(DW), arr(D16), arr(CS)]
    Ns, Ks = np.array([t.shape[1] for t in dys], dtype=np.int32), np.array([t.shape[1] for t in xs], dtype=np.int32)
    cp = lambda a: None if a is None else a.ctypes.data
    rc = dll.vitae_wgrad_group_bt(n, *(cp(a) for a in ptrs), cp(Ns), cp(Ks), M, Mpad, int(olds is not None), ws.ptr, ws.n, st())
    torch.cuda.synchronize()
    assert rc == expect, (rc, expect)
    for b in DW + (D16 or []) + (CS or []):
        assert b.untouched() if refused else b.clean()
    assert ws.clean()
    return [b.cpu() for b in DW], None if D16 is None else [b.cpu() for b in D16], None if CS is None else [b.cpu().view(-1) for b in CS]


@gpu
@pytest.mark.parametrize('kind', [-1, 3, 4, 6])
@pytest.mark.parametrize('dims', [[(136, 264)], [(120, 128), (264, 72)], [(64, 136), (136, 64), (128, 256), (8, 8)]])
@pytest.mark.parametrize('M,Mpad', [(250, 256), (1500, 1536)])
def test_wgrad_group_bt_exact(lib, bt_mode, kind, dims, M, Mpad):
    """n = 1, 2, 4 unequal problems, every kind; at Mpad = 1536 (24 k-tiles: splits of 1 - 3 are legal, and the ping-pong kind's
    clocks 12000 + 2650 nk / s + 9000 + 4000 s are lowest at 3) with room for any split, with room for a 2-way split of the 128 x 128
    tiles only (the split is shrunk to fit) and with no workspace: the integer answer every time.  Which kind and split the
    launcher took is ASSUMED from its cost model (it has no query); what is asserted is that no workspace size changes a bit and
    that nothing outside the given floats is touched."""
    dll = lib.load()
    bt_mode(kind)
    dys = [ints((M, N), 4, 100 + i) for i, (N, K) in enumerate(dims)]
    xs = [ints((M, K), 4, 110 + i) for i, (N, K) in enumerate(dims)]
    olds = [ints((N, K), 8, 120 + i) for i, (N, K) in enumerate(dims)]
    cs0 = [ints((N,), 8, 130 + i) for i, (N, K) in enumerate(dims)]
    want = [dys[i].double().t() @ xs[i].double() for i in range(len(dims))]
    area = sum(((N + 127) // 128) * ((K + 127) // 128) * 128 * 128 for N, K in dims)
    area2 = sum(((N + 127) // 128) * ((K + 255) // 256) * 128 * 256 for N, K in dims)
    tk = CONSTS['VITAE_GLDS_TICKETS']
    for wsf in ((0,) if Mpad < 1024 else (tk + 8 * max(area, area2), tk + 2 * area, 0)):
        dw, d16, cs = group_call(lib, dys, xs, M, Mpad, colsums=cs0, ws_floats=wsf)
        for i in range(len(dims)):
            assert torch.equal(dw[i], want[i].float()) and torch.equal(d16[i], dw[i].to(BF16)), (i, wsf)
            assert torch.equal(cs[i], (cs0[i].double() + dys[i].double().sum(0)).float())
    dw, d16, _ = group_call(lib, dys, xs, M, Mpad, olds=olds, ws_floats=0)
    for i in range(len(dims)):
        assert torch.equal(dw[i], (want[i] + olds[i]).float()) and torch.equal(d16[i], dw[i].to(BF16))


# =========================================================================== the weight-gradient sum-of-squares hooks
@gpu
@pytest.mark.parametrize('tile', [-2, 3, 4, 5, 6])
def test_wgrad_sqnorm_hooks_exact(lib, C, bt_mode, tile):
    """sum(dw_stored^2), exactly (operands in {-1, 0, 1}: integers whose squares total less than 2^24), without and with accumulate, through the
    single slot and through the spread slots (totalled as the header says: the slots `stride` doubles apart)"""
    dll = lib.load()
    M, N, K = 136, 264, 192
    bt_mode(tile)
    assert dll.vitae_gemm_glds_bt_choice(0, 0, M, N, K) == (tile if tile >= 0 else -1)
    a, b, old = ints((M, K), 1, 140), ints((N, K), 1, 141), ints((M, N), 8, 142)
    prod = a.double() @ b.double().t()
    # the slot is a double, but a workgroup may total its tile in fp32 first: with the whole sum below 2^24 every partial sum, in
    # any grouping and either format, is an exact integer
    assert float(prod.pow(2).sum()) < 2 ** 24 and float((prod + old).pow(2).sum()) < 2 ** 24
    n_slots, stride = 8, 4
    for spread in (False, True):
        sq = torch.zeros(n_slots * stride + GUARD, dtype=F64, device='cuda')
        sq[n_slots * stride:] = SENT
        try:
            if spread:
                assert dll.vitae_gemm_glds_set_wgrad_sqnorm_spread(sq.data_ptr(), n_slots, stride) == 0
            else:
                assert dll.vitae_gemm_glds_set_wgrad_sqnorm(sq.data_ptr()) == 0
            o1 = gemm_call(lib, 'glds', a, b, 'wgrad')
            o2 = gemm_call(lib, 'glds', a, b, 'wgrad', old=old)
        finally:
            assert dll.vitae_gemm_glds_set_wgrad_sqnorm(None) == 0
        torch.cuda.synchronize()
        assert torch.equal(o1.C, prod.float()) and torch.equal(o2.C, (prod + old.double()).float())
        want = float(o1.C.double().pow(2).sum() + o2.C.double().pow(2).sum())
        slots = sq[:n_slots * stride].view(n_slots, stride).cpu()
        assert float(slots[:, 0].sum()) == want if spread else float(slots[0, 0]) == want, (spread, float(slots.sum()), want)
        assert float(slots.sum()) == want and bool((sq[n_slots * stride:] == SENT).all())
    gemm_call(lib, 'glds', a, b, 'wgrad')                    # the hook is off again: nothing to write to
    # the weight-gradient half of the paired backward under the same mode
    dy, w, x = ints((100, 128), 1, 143), ints((128, 136), 1, 144), ints((100, 136), 1, 145)
    dww = dy.double().t() @ x.double()
    assert float(dww.pow(2).sum()) < 2 ** 24
    sq = torch.zeros(1 + GUARD, dtype=F64, device='cuda')
    sq[1:] = SENT
    try:
        assert dll.vitae_gemm_glds_set_wgrad_sqnorm(sq.data_ptr()) == 0
        o = pair_glds_call(lib, dy, w, x, 128)
    finally:
        assert dll.vitae_gemm_glds_set_wgrad_sqnorm(None) == 0
    torch.cuda.synchronize()
    assert torch.equal(o.dw, dww.float()) and float(sq[0]) == float(dww.pow(2).sum()) and bool((sq[1:] == SENT).all())


# =========================================================================== refusals leave everything alone
@gpu
def test_refused_calls_write_nothing(lib, C, bt_mode):
    INV, UNS = -1, -2                                       # VITAE_ERR_INVALID_ARG, VITAE_ERR_UNSUPPORTED_SHAPE (include/vitae_hip.h)
    a, b, bias, res, old, _ = exact_problem(64, 72, 128, 150)
    every = dict(bias=bias, res=res)
    # misaligned operand pointers (4 / 2 bytes past a 16-byte boundary)
    for entry, kw in (('gemm', dict(prec=0)), ('gemm', dict(prec=1)), ('gemm', dict(prec=2)), ('x3', {}), ('bf16', {}), ('wsx3', {}), ('glds', dict(c16=True)), ('w2', dict(c16=True))):
        gemm_call(lib, entry, a, b, a_off=1, expect=UNS, **every, **kw)
    # ld not a multiple of the vector width (4 floats; 8 bf16)
    for entry, kw, bad_a, bad_b in (('gemm', dict(prec=0), 2, 2), ('gemm', dict(prec=1), 2, 2), ('gemm', dict(prec=2), 2, 2), ('bf16', dict(b16=1), 2, 4),
                                    ('wsx3', {}, 2, 2), ('glds', dict(c16=True), 4, 4), ('w2', dict(c16=True), 4, None)):
        gemm_call(lib, entry, a, b, ld=dict(a=128 + bad_a), expect=UNS, **every, **kw)
        if bad_b:
            gemm_call(lib, entry, a, b, ld=dict(b=128 + bad_b), expect=UNS, **every, **kw)
    gemm_call(lib, 'wsx3', a, b, ld=dict(c=72 + 2), expect=UNS, **every)           # no scalar epilogue on this kernel
    gemm_call(lib, 'w2', a, b, ld=dict(c=72 + 2), expect=UNS, **every)
    # K % 64 on the LDS-DMA family, K % 4 on the others
    a2, b2 = ints((64, 136), 4, 151), ints((72, 136), 4, 152)
    gemm_call(lib, 'glds', a2, b2, expect=UNS, c16=True, **every)
    gemm_call(lib, 'w2', a2, b2, expect=UNS, **every)
    gemm_call(lib, 'w2', a[:, :64], b[:, :64], expect=UNS, **every)                 # two k-tiles at least
    a3, b3 = ints((64, 30), 4, 153), ints((72, 30), 4, 154)
    for entry, kw in (('gemm', dict(prec=0)), ('gemm', dict(prec=2)), ('bf16', {})):
        gemm_call(lib, entry, a3, b3, expect=UNS, **every, **kw)
    # split_k > 1 without a workspace (K = 512: two parts on every family's k-tile)
    a4, b4 = ints((64, 512), 4, 155), ints((72, 512), 4, 156)
    for entry, kw in (('gemm', dict(prec=0)), ('gemm', dict(prec=1)), ('gemm', dict(prec=2)), ('x3', {}), ('bf16', {}), ('wsx3', {}), ('glds', {}), ('w2', {})):
        gemm_call(lib, entry, a4, b4, split=2, no_ws=True, expect=INV, **every, **kw)
    # an epilogue that needs aux without one; bf16 aux on the fp32 families
    gemm_call(lib, 'gemm', a, b, epi=C['VITAE_EPI_DGELU'], expect=INV)
    gemm_call(lib, 'gemm', a, b, epi=C['VITAE_EPI_DGELU'] | C['VITAE_EPI_AUX_BF16'], aux=old, expect=UNS)
    # the paired backward: Mpad < M, Mpad % 64, N % 64, K % 8, a split the workspace cannot hold
    dy, w, x = ints((100, 128), 4, 157), ints((128, 72), 4, 158), ints((100, 72), 4, 159)
    full = dict(dx16=True, dw16=True, dxcs0=ints((72,), 8, 160), dycs0=ints((128,), 8, 161))
    pair_glds_call(lib, dy, w, x, 64, expect=UNS, **full)
    pair_glds_call(lib, dy, w, x, 120, expect=UNS, **full)
    pair_glds_call(lib, dy[:, :120], w[:120], x, 128, expect=UNS, **full)
    pair_glds_call(lib, dy, w[:, :68], x[:, :68], 128, expect=UNS, dx16=True, dw16=True)
    pair_glds_call(lib, dy, w, x, 128, split=2, ws_for=(100, 72, 1), expect=INV, **full)
    pair_bf16_call(lib, dy[:, :124], w[:124], x, db0=ints((124,), 8, 162), expect=UNS)
    # the grouped weight gradient: Mpad < 256, Mpad < M
    group_call(lib, [dy], [x], 100, 128, expect=UNS)
    group_call(lib, [pad_rows(dy, 300)], [pad_rows(x, 300)], 300, 256, expect=INV)

