"""The kernels of the 3-D ResNet baseline (csrc/conv3d.hip and the BasicBlock tail of csrc/norm.hip) where they can go wrong.

Reference: torch's own ``F.conv3d``, ``torch.nn.grad.conv3d_input`` / ``conv3d_weight``, ``F.max_pool3d(return_indices=True)`` and
a hand-written two-pass BatchNorm in float64 on the CPU, on permuted copies of the channels-last operands.

Convolution (forward, input gradient, weight gradient share ``CASES``)
  bit for bit   operands are integers in [-3, 3], so every partial sum is exact in fp32 (9 K < 2^24, 9 M < 2^24): the result must
                EQUAL float64's.  The weight gradient has one more case whose M spans three chunks of VITAE_CONV3D_WGRAD_CHUNK rows
                with a partial last one.
  per element   operands N(3, 1) rounded to bf16; e = |y - y64| / sum |x| |w| per output element, worst element;
                bound max(FACTOR e32, FLOOR), e32 the same metric of torch's fp32 CPU convolution on the same operands
                (FACTOR = 3, FLOOR = 4 x 2^-24: the rule of tests/test_gemm_kernels.py).  ``RATIO`` lines are printed (run with -s).
  predicates    one NaN element in the gathered operand poisons exactly the outputs whose window covers it; every other output
                equals the clean run bit for bit.  For the weight gradient a NaN in dy16[m, co] poisons dW[co] as a whole: row m is
                an addend of every tap of that output channel — with a zero x where the tap falls into the padding, and NaN x 0 is
                NaN on the MFMA as it is in torch's own float64 conv3d_weight; a NaN in x16 poisons exactly the taps that read it.
  guards        every operand sits between two NaN-filled regions, every output and workspace has sentinels behind it.
  repeats are bit-equal; every refusal leaves the outputs untouched.

BatchNorm tail y = [relu](bn(x) [+ res]): the rule of tests/test_norm_kernels.py — per column, the error in units of what is
subtracted, bound max(3 e32, 4 x 2^-24), e32 the larger of torch's fp32 op and the formula evaluated in fp32."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
GUARD, SENT = 64, 7.25
FACTOR, FLOOR = 3.0, 4.0 * 2.0 ** -24
EPS_BN, MOM = 1e-5, 0.1


def conv_case(N, vol, cin, cout, k, s, p):
    return dict(N=N, vol=vol, Cin=cin, Cout=cout, k=(k,) * 3 if isinstance(k, int) else k, s=s, p=(p,) * 3 if isinstance(p, int) else p)


CASES = {
    'stem_1_4': conv_case(2, (5, 9, 10), 1, 4, 7, (1, 2, 2), 3),            # K = 343
    'stem_1_64': conv_case(2, (5, 9, 10), 1, 64, 7, (1, 2, 2), 3),
    'stem_4_4': conv_case(2, (5, 9, 10), 4, 4, 7, (1, 2, 2), 3),            # K = 1372
    'stem_4_64': conv_case(2, (5, 9, 10), 4, 64, 7, (1, 2, 2), 3),
    'stem_1_64_t2': conv_case(2, (5, 9, 10), 1, 64, 7, (2, 2, 2), 3),       # conv1_t_stride = 2
    'stem_4_4_t2': conv_case(2, (5, 9, 10), 4, 4, 7, (2, 2, 2), 3),
    'k3_8_8': conv_case(1, (3, 4, 5), 8, 8, 3, (1, 1, 1), 1),
    'k3_4_8': conv_case(1, (3, 4, 5), 4, 8, 3, (1, 1, 1), 1),               # K = 108: not a multiple of the k step
    'k3_12_12': conv_case(1, (3, 4, 5), 12, 12, 3, (1, 1, 1), 1),           # Cin not a power of two
    'k3_64_64': conv_case(3, (4, 4, 4), 64, 64, 3, (1, 1, 1), 1),           # 192 rows: they cross a 128-row tile edge
    'k3s2_64_128': conv_case(1, (5, 6, 7), 64, 128, 3, (2, 2, 2), 1),       # -> (3, 3, 4)
    'k1s2_16_32': conv_case(1, (5, 6, 7), 16, 32, 1, (2, 2, 2), 0),
    'k3_unit': conv_case(1, (1, 1, 1), 8, 8, 3, (1, 1, 1), 1),              # all taps but one are padding
}
CASE_IDS = list(CASES)


def out_vol(c):
    return tuple((c['vol'][i] + 2 * c['p'][i] - c['k'][i]) // c['s'][i] + 1 for i in range(3))


def geo_args(c):
    return (c['N'], *c['vol'], c['Cin'], c['Cout'], *c['k'], *c['s'], *c['p'])


def int_operands(c, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (c['N'], c['Cin'], *c['vol']), generator=g).to(F32)
    w = torch.randint(-3, 4, (c['Cout'], c['Cin'], *c['k']), generator=g).to(F32)
    dy = torch.randint(-3, 4, (c['N'], c['Cout'], *out_vol(c)), generator=g).to(F32)
    return x, w, dy


def gauss_operands(c, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: (torch.randn(*s, generator=g) + 3.0).to(BF16).to(F32)
    return r(c['N'], c['Cin'], *c['vol']), r(c['Cout'], c['Cin'], *c['k']), r(c['N'], c['Cout'], *out_vol(c))


def _native(fn):
    """torch's own CPU convolution with oneDNN off: its fp32 weight gradient for the stem at temporal stride 2 corrupts the heap in
    this torch build (glibc aborts with 'double free or corruption'); the float64 calls never take that path."""
    def wrapped(*a, **k):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            with torch.backends.mkldnn.flags(enabled=False):
                return fn(*a, **k)
    return wrapped


@_native
def ref_fwd(x, w, c, dt=F64):
    return F.conv3d(x.to(dt), w.to(dt), None, c['s'], c['p'])


@_native
def ref_dx(dy, w, c, dt=F64):
    return torch.nn.grad.conv3d_input((c['N'], c['Cin'], *c['vol']), w.to(dt), dy.to(dt), c['s'], c['p'])


@_native
def ref_dw(x, dy, c, dt=F64):
    return torch.nn.grad.conv3d_weight(x.to(dt), (c['Cout'], c['Cin'], *c['k']), dy.to(dt), c['s'], c['p'])


def cl(t):
    """[N, C, D, H, W] -> channels-last rows [N D H W, C]"""
    return t.permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1]).contiguous()


def uncl(rows, N, vol):
    return rows.reshape(N, *vol, rows.shape[-1]).permute(0, 4, 1, 2, 3).contiguous()


# ---------------------------------------------------------------------------- CPU: the references and the cases themselves
def test_cases_cover_the_paths():
    ks = {c['Cin'] * int(np.prod(c['k'])) for c in CASES.values()}
    assert 108 in ks and 343 in ks and any(k % 16 for k in ks)
    assert any(c['Cout'] < 32 for c in CASES.values())
    assert any(c['N'] * int(np.prod(out_vol(c))) > 128 for c in CASES.values())
    assert out_vol(CASES['k3s2_64_128']) == (3, 3, 4)
    for c in CASES.values():                                         # integers stay exact in fp32
        K = c['Cin'] * int(np.prod(c['k']))
        assert 9 * K < 2 ** 24 and 9 * c['N'] * int(np.prod(out_vol(c))) < 2 ** 24


def test_float64_references_agree_with_autograd():
    c = CASES['k3s2_64_128']
    x, w, dy = gauss_operands(c, 0)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    F.conv3d(xr, wr, None, c['s'], c['p']).backward(dy.double())
    assert torch.allclose(ref_dx(dy, w, c), xr.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(ref_dw(x, dy, c), wr.grad, rtol=1e-12, atol=1e-12)


def test_abi_declares_the_resnet_entry_points():
    from vit_ae_plus_plus_amd import _abi
    assert _abi.CONSTS['VITAE_ABI_VERSION'] >= 56
    assert _abi.CONSTS['VITAE_CONV3D_WGRAD_CHUNK'] > 0 and _abi.CONSTS['VITAE_CONV3D_K_STEP'] == 16
    for name in ('vitae_conv3d_fwd', 'vitae_conv3d_bwd_input', 'vitae_conv3d_bwd_weight', 'vitae_conv3d_wgrad_ws_floats',
                 'vitae_conv3d_pack_weight', 'vitae_to_channels_last_bf16', 'vitae_maxpool3d_fwd', 'vitae_maxpool3d_bwd',
                 'vitae_rows_mean_fwd', 'vitae_rows_mean_bwd', 'vitae_bn_tail_fwd_split', 'vitae_bn_tail_eval', 'vitae_bn_tail_bwd_split'):
        assert name in _abi.PROTOS, name


def test_host_size_queries():
    from vit_ae_plus_plus_amd import _abi
    lib, chunk = _abi.lib, _abi.CONSTS['VITAE_CONV3D_WGRAD_CHUNK']
    assert lib.vitae_conv3d_packed_elems(64, 1, 7, 7, 7, 0) == 64 * 352            # 343 -> 352
    assert lib.vitae_conv3d_packed_elems(8, 4, 3, 3, 3, 0) == 8 * 112              # 108 -> 112
    assert lib.vitae_conv3d_packed_elems(8, 4, 3, 3, 3, 1) == 4 * 224              # 27 * 8 = 216 -> 224
    c = CASES['k3_64_64']
    assert lib.vitae_conv3d_wgrad_ws_floats(*geo_args(c)) == 1 * 64 * 27 * 64
    big = conv_case(1, (2 * chunk + 7, 1, 1), 4, 4, 1, (1, 1, 1), 0)
    assert lib.vitae_conv3d_wgrad_ws_floats(*geo_args(big)) == 3 * 4 * 4
    bad = dict(c, Cout=6)
    assert lib.vitae_conv3d_wgrad_ws_floats(*geo_args(bad)) == 0


# ---------------------------------------------------------------------------- GPU plumbing
def _lib():
    from vit_ae_plus_plus_amd import _abi
    return _abi.lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def operand(t, dtype):
    """A device copy of t between two NaN-filled guard regions (a read outside the operand poisons the result)."""
    n = t.numel()
    buf = torch.full((n + 2 * GUARD,), float('nan'), dtype=dtype, device='cuda')
    view = buf[GUARD:GUARD + n].view(t.shape)
    view.copy_(t.to(dtype))
    view._guard = buf
    return view


class Out:
    """An output (or workspace) with sentinels behind it; `fill` is what an element nobody wrote shows."""

    def __init__(self, shape, dtype=F32, fill=SENT):
        n = int(np.prod(shape))
        self.n, self.fill, self.sent = n, fill, SENT if dtype.is_floating_point else 7
        self.buf = torch.full((n + GUARD,), fill, dtype=dtype, device='cuda')
        self.buf[n:] = self.sent
        self.t = self.buf[:n].view(shape)

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        assert bool((self.buf[self.n:] == self.sent).all()), 'sentinels behind an output were overwritten'
        return self.t

    def untouched(self):
        self.intact()
        assert bool((self.buf[:self.n] == self.fill).all()), 'a refused call wrote to its output'


def dev_pack(w, transposed):
    lib = _lib()
    co, ci, kd, kh, kw = w.shape
    n = lib.vitae_conv3d_packed_elems(co, ci, kd, kh, kw, transposed)
    wd = operand(w, F32)
    out = Out((n,), BF16)
    lib.vitae_conv3d_pack_weight(wd.data_ptr(), out.ptr(), co, ci, kd, kh, kw, transposed, _stream())
    packed = out.intact()
    keep = operand(packed.float().cpu(), BF16)                       # between NaN guards, as every operand
    return keep


def host_pack(w, transposed):
    co, ci = w.shape[:2]
    taps = int(np.prod(w.shape[2:]))
    w3 = w.reshape(co, ci, taps)
    m = w3.permute(1, 2, 0).reshape(ci, taps * co) if transposed else w3.permute(0, 2, 1).reshape(co, taps * ci)
    kp = (m.shape[1] + 15) // 16 * 16
    return F.pad(m, (0, kp - m.shape[1])).to(BF16)


def run_fwd(c, x, w16, want=('f32', 'bf16')):
    lib, M = _lib(), c['N'] * int(np.prod(out_vol(c)))
    x16 = x if x.dtype == BF16 and x.is_cuda else operand(cl(x), BF16)
    y = Out((M, c['Cout'])) if 'f32' in want else None
    y16 = Out((M, c['Cout']), BF16) if 'bf16' in want else None
    lib.vitae_conv3d_fwd(x16.data_ptr(), w16.data_ptr(), y.ptr() if y else None, y16.ptr() if y16 else None, *geo_args(c), _stream())
    torch.cuda.synchronize()
    return (y.intact() if y else None), (y16.intact() if y16 else None)


def run_dx(c, dy, w16t, want=('f32', 'bf16'), base=None):
    lib, V = _lib(), c['N'] * int(np.prod(c['vol']))
    dy16 = dy if dy.dtype == BF16 and dy.is_cuda else operand(cl(dy), BF16)
    dx = Out((V, c['Cin'])) if 'f32' in want else None
    dx16 = Out((V, c['Cin']), BF16) if 'bf16' in want else None
    if base is not None:
        dx.t.copy_(base)
    lib.vitae_conv3d_bwd_input(dy16.data_ptr(), w16t.data_ptr(), dx.ptr() if dx else None, dx16.ptr() if dx16 else None, 0 if base is None else 1,
                               *geo_args(c), _stream())
    torch.cuda.synchronize()
    return (dx.intact() if dx else None), (dx16.intact() if dx16 else None)


def run_dw(c, x, dy, accumulate=None):
    lib = _lib()
    x16 = x if x.dtype == BF16 and x.is_cuda else operand(cl(x), BF16)
    dy16 = dy if dy.dtype == BF16 and dy.is_cuda else operand(cl(dy), BF16)
    n = lib.vitae_conv3d_wgrad_ws_floats(*geo_args(c))
    ws = Out((n,), fill=float('nan'))
    dw = Out((c['Cout'], c['Cin'], *c['k']))
    if accumulate is not None:
        dw.t.copy_(accumulate)
    lib.vitae_conv3d_bwd_weight(dy16.data_ptr(), x16.data_ptr(), dw.ptr(), ws.ptr(), n, 0 if accumulate is None else 1, *geo_args(c), _stream())
    torch.cuda.synchronize()
    ws.intact()
    assert not bool(torch.isnan(ws.t).any()) or bool(torch.isnan(dw.t).any()), 'a workspace element was never written'
    return dw.intact()


def rows_to(t, c, which):
    """kernel rows -> torch layout, float64 on the CPU"""
    vol = out_vol(c) if which == 'y' else c['vol']
    return uncl(t.double().cpu(), c['N'], vol)


# ---------------------------------------------------------------------------- packing
@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(4, 1, 7, 7, 7), (8, 4, 3, 3, 3), (32, 16, 1, 1, 1), (12, 12, 3, 3, 3)])
def test_pack_weight(shape):
    g = torch.Generator().manual_seed(1)
    w = torch.randn(shape, generator=g)
    for tr in (0, 1):
        got = dev_pack(w, tr).cpu()
        assert torch.equal(got.view(torch.int16), host_pack(w, tr).reshape(-1).view(torch.int16)), (shape, tr)


@pytest.mark.gpu
def test_channels_last_bf16():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 3, 4, 5, 6, generator=g)
    xd = operand(x, F32)
    out = Out((2 * 4 * 5 * 6, 3), BF16)
    _lib().vitae_to_channels_last_bf16(xd.data_ptr(), out.ptr(), 2, 3, 4, 5, 6, _stream())
    torch.cuda.synchronize()
    assert torch.equal(out.intact().cpu().view(torch.int16), cl(x).to(BF16).view(torch.int16))


# ---------------------------------------------------------------------------- bit for bit on integers
@pytest.mark.gpu
@pytest.mark.parametrize('name', CASE_IDS)
def test_conv_exact_on_integers(name):
    c = CASES[name]
    x, w, dy = int_operands(c, 11)
    y, y16 = run_fwd(c, x, dev_pack(w, 0))
    y64 = ref_fwd(x, w, c)
    assert torch.equal(rows_to(y, c, 'y'), y64), name
    assert torch.equal(y16.view(torch.int16), y.to(BF16).view(torch.int16))
    dx, dx16 = run_dx(c, dy, dev_pack(w, 1))
    assert torch.equal(rows_to(dx, c, 'x'), ref_dx(dy, w, c)), name
    assert torch.equal(dx16.view(torch.int16), dx.to(BF16).view(torch.int16))
    # accumulate: added to what dx held (the residual branch's gradient); the bf16 copy is that of the total
    held = torch.randint(-5, 6, dx.shape).to(F32)
    dx2, dx216 = run_dx(c, dy, dev_pack(w, 1), base=held.cuda())
    assert torch.equal(dx2.double().cpu(), dx.double().cpu() + held.double()), name
    assert torch.equal(dx216.view(torch.int16), dx2.to(BF16).view(torch.int16))
    dw = run_dw(c, x, dy)
    assert torch.equal(dw.double().cpu(), ref_dw(x, dy, c)), name
    # accumulation (accum_iter > 1): added to what dW held
    base = torch.randint(-5, 6, dw.shape).to(F32)
    dw2 = run_dw(c, x, dy, accumulate=base.cuda())
    assert torch.equal(dw2.double().cpu(), ref_dw(x, dy, c) + base.double()), name


@pytest.mark.gpu
def test_only_one_output_requested_gives_the_same_bits():
    c = CASES['k3_4_8']
    x, w, dy = gauss_operands(c, 3)
    w16, w16t = dev_pack(w, 0), dev_pack(w, 1)
    y, y16 = run_fwd(c, x, w16)
    assert torch.equal(run_fwd(c, x, w16, want=('f32',))[0], y) and torch.equal(run_fwd(c, x, w16, want=('bf16',))[1], y16)
    dx, dx16 = run_dx(c, dy, w16t)
    assert torch.equal(run_dx(c, dy, w16t, want=('f32',))[0], dx) and torch.equal(run_dx(c, dy, w16t, want=('bf16',))[1], dx16)


@pytest.mark.gpu
def test_wgrad_three_chunks_with_a_partial_last():
    from vit_ae_plus_plus_amd import _abi
    chunk = _abi.CONSTS['VITAE_CONV3D_WGRAD_CHUNK']
    # 3 x 3 x 3 over (D, 8, 8): M = 64 D rows; D chosen so that M = 2 chunks + 192 rows
    assert chunk % 64 == 0
    D = 2 * chunk // 64 + 3
    c = conv_case(1, (D, 8, 8), 4, 8, 3, (1, 1, 1), 1)
    M = int(np.prod(out_vol(c)))
    assert 2 * chunk < M < 3 * chunk and 9 * M < 2 ** 24
    assert _lib().vitae_conv3d_wgrad_ws_floats(*geo_args(c)) == 3 * 8 * 108
    x, w, dy = int_operands(c, 12)
    dw = run_dw(c, x, dy)
    assert torch.equal(dw.double().cpu(), ref_dw(x, dy, c))
    assert torch.equal(run_dw(c, x, dy), dw)


# ---------------------------------------------------------------------------- per element
def elem_err(got, ref64, den):
    """worst element of |got - ref64| / den; where den == 0 (no addend at all) the result must be an exact zero"""
    num = (got.double() - ref64).abs()
    live = den > 0
    assert bool((num[~live] == 0).all())
    return float((num[live] / den[live]).max())


def within(label, e, e32):
    r = e / e32 if e32 > 0 else (0.0 if e == 0 else float('inf'))
    print(f'RATIO {label}: e={e:.3e} e32={e32:.3e} ratio={r:.2f}')
    assert e <= max(FACTOR * e32, FLOOR), (label, e, e32)


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASE_IDS)
def test_conv_per_element(name):
    c = CASES[name]
    x, w, dy = gauss_operands(c, 21)
    y, _ = run_fwd(c, x, dev_pack(w, 0))
    y64, den = ref_fwd(x, w, c), ref_fwd(x.abs(), w.abs(), c)
    within(f'conv_fwd {name}', elem_err(rows_to(y, c, 'y'), y64, den), elem_err(ref_fwd(x, w, c, F32), y64, den))
    dx, _ = run_dx(c, dy, dev_pack(w, 1))
    dx64, den = ref_dx(dy, w, c), ref_dx(dy.abs(), w.abs(), c)
    within(f'conv_bwd_input {name}', elem_err(rows_to(dx, c, 'x'), dx64, den), elem_err(ref_dx(dy, w, c, F32), dx64, den))
    dw = run_dw(c, x, dy)
    dw64, den = ref_dw(x, dy, c), ref_dw(x.abs(), dy.abs(), c)
    within(f'conv_bwd_weight {name}', elem_err(dw.cpu(), dw64, den), elem_err(ref_dw(x, dy, c, F32), dw64, den))


# ---------------------------------------------------------------------------- gather predicates
def assert_poisoned_exactly(got, clean, expect_nan, label):
    got, clean = got.cpu(), clean.cpu()
    nan = torch.isnan(got)
    assert torch.equal(nan, expect_nan), (label, int(nan.sum()), int(expect_nan.sum()))
    assert torch.equal(got[~nan].view(torch.int32), clean[~nan].view(torch.int32)), label


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['stem_4_4', 'stem_1_64_t2', 'k3_4_8', 'k3_64_64', 'k3s2_64_128', 'k1s2_16_32', 'k3_unit'])
def test_one_nan_poisons_exactly_its_windows(name):
    c = CASES[name]
    x, w, dy = gauss_operands(c, 31)
    w16, w16t = dev_pack(w, 0), dev_pack(w, 1)
    ones_w = torch.ones_like(w).double()
    g = torch.Generator().manual_seed(32)
    # forward: a NaN in x
    pos = tuple(int(torch.randint(0, s, (1,), generator=g)) for s in x.shape)
    ind = torch.zeros_like(x).double(); ind[pos] = 1
    xn = x.clone(); xn[pos] = float('nan')
    cover = F.conv3d(ind, ones_w, None, c['s'], c['p']) > 0           # [N, Cout, Do, Ho, Wo]: every channel of a covered row
    assert_poisoned_exactly(run_fwd(c, xn, w16)[0], run_fwd(c, x, w16)[0], cl(cover), f'fwd {name}')
    # weight gradient: the same NaN in x poisons the taps that read it, in every output channel
    cover_w = ref_dw(ind, torch.ones_like(dy), c) > 0
    assert_poisoned_exactly(run_dw(c, xn, dy), run_dw(c, x, dy), cover_w, f'wgrad x {name}')
    # input gradient: a NaN in dy
    pos = tuple(int(torch.randint(0, s, (1,), generator=g)) for s in dy.shape)
    ind = torch.zeros_like(dy).double(); ind[pos] = 1
    dyn = dy.clone(); dyn[pos] = float('nan')
    cover = ref_dx(ind, ones_w, c) > 0
    assert_poisoned_exactly(run_dx(c, dyn, w16t)[0], run_dx(c, dy, w16t)[0], cl(cover), f'dx {name}')
    # weight gradient: a NaN in dy[m, co] poisons dW[co] (see the module docstring), no other output channel
    cover_w = torch.zeros(c['Cout'], c['Cin'], *c['k'], dtype=torch.bool); cover_w[pos[1]] = True
    assert_poisoned_exactly(run_dw(c, x, dyn), run_dw(c, x, dy), cover_w, f'wgrad dy {name}')


# ---------------------------------------------------------------------------- refusals
def bad_geometries():
    c = CASES['k3_8_8']
    yield 'Cout % 4', dict(c, Cout=6)
    yield 'kernel 8', dict(c, k=(8, 3, 3), p=(1, 1, 1))
    yield 'kernel 0', dict(c, k=(3, 0, 3))
    yield 'stride 3', dict(c, s=(1, 3, 1))
    yield 'stride 0', dict(c, s=(0, 1, 1))
    yield 'pad == kernel', dict(c, p=(3, 1, 1))
    yield 'pad < 0', dict(c, p=(1, -1, 1))
    yield 'extent 0', dict(c, vol=(3, 0, 5))
    yield 'N 0', dict(c, N=0)
    yield 'Cin 0', dict(c, Cin=0)
    yield 'output extent 0', dict(c, vol=(1, 4, 5), k=(5, 3, 3), p=(1, 1, 1))


@pytest.mark.gpu
def test_refusals_write_nothing():
    from vit_ae_plus_plus_amd import _abi
    dll = _abi.lib.load()                                            # raw return codes
    st = _stream()
    src = operand(torch.zeros(4096), BF16)
    wsrc = operand(torch.zeros(4096), F32)
    out, out16, ws = Out((4096,)), Out((4096,), BF16), Out((65536,))
    for label, c in bad_geometries():
        ga = geo_args(c)
        assert dll.vitae_conv3d_fwd(src.data_ptr(), src.data_ptr(), out.ptr(), out16.ptr(), *ga, st) in (-1, -2), label
        assert dll.vitae_conv3d_bwd_input(src.data_ptr(), src.data_ptr(), out.ptr(), out16.ptr(), 0, *ga, st) in (-1, -2), label
        assert dll.vitae_conv3d_bwd_weight(src.data_ptr(), src.data_ptr(), out.ptr(), ws.ptr(), 65536, 0, *ga, st) in (-1, -2), label
        assert dll.vitae_conv3d_wgrad_ws_floats(*ga) == 0, label
    c = CASES['k3_8_8']
    ga = geo_args(c)
    need = dll.vitae_conv3d_wgrad_ws_floats(*ga)
    assert need == 8 * 27 * 8
    assert dll.vitae_conv3d_bwd_weight(src.data_ptr(), src.data_ptr(), out.ptr(), ws.ptr(), need - 1, 0, *ga, st) == -1      # workspace too small
    for args in ((None, src.data_ptr(), out.ptr(), out16.ptr()), (src.data_ptr(), None, out.ptr(), out16.ptr()), (src.data_ptr(), src.data_ptr(), None, None)):
        assert dll.vitae_conv3d_fwd(*args, *ga, st) == -1
        assert dll.vitae_conv3d_bwd_input(*args, 0, *ga, st) == -1
    assert dll.vitae_conv3d_bwd_input(src.data_ptr(), src.data_ptr(), None, out16.ptr(), 1, *ga, st) == -1            # accumulate needs dx
    for args in ((None, src.data_ptr(), out.ptr(), ws.ptr()), (src.data_ptr(), None, out.ptr(), ws.ptr()), (src.data_ptr(), src.data_ptr(), None, ws.ptr()),
                 (src.data_ptr(), src.data_ptr(), out.ptr(), None)):
        assert dll.vitae_conv3d_bwd_weight(*args, need, 0, *ga, st) == -1
    assert dll.vitae_conv3d_pack_weight(None, out16.ptr(), 8, 8, 3, 3, 3, 0, st) == -1
    assert dll.vitae_conv3d_pack_weight(wsrc.data_ptr(), None, 8, 8, 3, 3, 3, 0, st) == -1
    assert dll.vitae_conv3d_pack_weight(wsrc.data_ptr(), out16.ptr(), 6, 8, 3, 3, 3, 0, st) == -2
    assert dll.vitae_conv3d_pack_weight(wsrc.data_ptr(), out16.ptr(), 8, 8, 3, 9, 3, 0, st) == -2
    assert dll.vitae_to_channels_last_bf16(None, out16.ptr(), 1, 1, 2, 2, 2, st) == -1
    assert dll.vitae_to_channels_last_bf16(wsrc.data_ptr(), out16.ptr(), 1, 0, 2, 2, 2, st) == -1
    idx = Out((4096,), torch.uint8, fill=3)
    assert dll.vitae_maxpool3d_fwd(None, out.ptr(), out16.ptr(), idx.ptr(), 1, 2, 2, 2, 4, st) == -1
    assert dll.vitae_maxpool3d_fwd(wsrc.data_ptr(), None, None, idx.ptr(), 1, 2, 2, 2, 4, st) == -1
    assert dll.vitae_maxpool3d_fwd(wsrc.data_ptr(), out.ptr(), out16.ptr(), None, 1, 2, 2, 2, 4, st) == -1
    assert dll.vitae_maxpool3d_fwd(wsrc.data_ptr(), out.ptr(), out16.ptr(), idx.ptr(), 1, 0, 2, 2, 4, st) == -1
    assert dll.vitae_maxpool3d_bwd(wsrc.data_ptr(), idx.ptr(), None, None, 1, 2, 2, 2, 4, st) == -1
    assert dll.vitae_maxpool3d_bwd(wsrc.data_ptr(), None, out.ptr(), out16.ptr(), 1, 2, 2, 2, 4, st) == -1
    assert dll.vitae_rows_mean_fwd(wsrc.data_ptr(), None, None, 2, 3, 4, st) == -1
    assert dll.vitae_rows_mean_fwd(wsrc.data_ptr(), out.ptr(), None, 2, 0, 4, st) == -1
    assert dll.vitae_rows_mean_bwd(None, out.ptr(), None, 2, 3, 4, st) == -1
    assert dll.vitae_rows_mean_bwd(wsrc.data_ptr(), None, None, 2, 3, 4, st) == -1
    # the BatchNorm tail: C % 4, NULL pointers, no rows
    x = wsrc.data_ptr()
    assert dll.vitae_bn_tail_fwd_split(x, None, x, x, out.ptr(), out16.ptr(), out.ptr(), out.ptr(), None, None, None, 8, 6, EPS_BN, MOM, 1, ws.ptr(), st) == -2
    assert dll.vitae_bn_tail_fwd_split(x, None, x, x, out.ptr(), out16.ptr(), out.ptr(), out.ptr(), None, None, None, 0, 8, EPS_BN, MOM, 1, ws.ptr(), st) == -1
    assert dll.vitae_bn_tail_fwd_split(x, None, x, x, out.ptr(), out16.ptr(), out.ptr(), out.ptr(), None, None, None, 8, 8, EPS_BN, MOM, 1, None, st) == -1
    assert dll.vitae_bn_tail_fwd_split(None, None, x, x, out.ptr(), out16.ptr(), out.ptr(), out.ptr(), None, None, None, 8, 8, EPS_BN, MOM, 1, ws.ptr(), st) == -1
    assert dll.vitae_bn_tail_eval(x, None, x, x, x, x, out.ptr(), out16.ptr(), 8, 6, EPS_BN, 1, st) == -2
    assert dll.vitae_bn_tail_eval(x, None, x, x, None, x, out.ptr(), out16.ptr(), 8, 8, EPS_BN, 1, st) == -1
    assert dll.vitae_bn_tail_bwd_split(x, x, x, x, x, x, out.ptr(), out16.ptr(), None, out.ptr(), out.ptr(), 8, 6, 1, ws.ptr(), st) == -2
    assert dll.vitae_bn_tail_bwd_split(x, x, None, x, x, x, out.ptr(), out16.ptr(), None, out.ptr(), out.ptr(), 8, 8, 1, ws.ptr(), st) == -1   # relu needs y
    assert dll.vitae_bn_tail_bwd_split(x, x, x, x, x, x, out.ptr(), out16.ptr(), None, out.ptr(), out.ptr(), 8, 8, 1, None, st) == -1
    torch.cuda.synchronize()
    for o in (out, out16, ws, idx):
        o.untouched()


# ---------------------------------------------------------------------------- repeats
@pytest.mark.gpu
@pytest.mark.parametrize('name', ['stem_4_64', 'k3_64_64', 'k3s2_64_128'])
def test_repeats_are_bit_equal(name):
    c = CASES[name]
    x, w, dy = gauss_operands(c, 41)
    w16, w16t = dev_pack(w, 0), dev_pack(w, 1)
    a, b = run_fwd(c, x, w16), run_fwd(c, x, w16)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int16), b[1].view(torch.int16))
    a, b = run_dx(c, dy, w16t), run_dx(c, dy, w16t)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int16), b[1].view(torch.int16))
    assert torch.equal(run_dw(c, x, dy).view(torch.int32), run_dw(c, x, dy).view(torch.int32))


# ---------------------------------------------------------------------------- max pool
def run_pool(x):
    """x [N, C, D, H, W] (CPU fp32) -> y rows, y16 rows, idx rows (device)"""
    N, C, D, H, W = x.shape
    Do, Ho, Wo = (D - 1) // 2 + 1, (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xd = operand(cl(x), F32)
    n = N * Do * Ho * Wo
    y, y16, idx = Out((n, C)), Out((n, C), BF16), Out((n, C), torch.uint8, fill=7)
    _lib().vitae_maxpool3d_fwd(xd.data_ptr(), y.ptr(), y16.ptr(), idx.ptr(), N, D, H, W, C, _stream())
    torch.cuda.synchronize()
    return y.intact(), y16.intact(), idx.intact(), (Do, Ho, Wo)


def run_pool_bwd(dy, idx, shape):
    N, C, D, H, W = shape
    dyd = operand(cl(dy), F32)
    dx, dx16 = Out((N * D * H * W, C)), Out((N * D * H * W, C), BF16)
    _lib().vitae_maxpool3d_bwd(dyd.data_ptr(), idx.data_ptr(), dx.ptr(), dx16.ptr(), N, D, H, W, C, _stream())
    torch.cuda.synchronize()
    return dx.intact(), dx16.intact()


def torch_tap_index(flat_idx, shape, ovol):
    """torch's flat input index per output -> the tap (kd 3 + kh) 3 + kw of the window"""
    N, C, D, H, W = shape
    d, h, w = flat_idx // (H * W), (flat_idx // W) % H, flat_idx % W
    od = torch.arange(ovol[0]).view(1, 1, -1, 1, 1)
    oh = torch.arange(ovol[1]).view(1, 1, 1, -1, 1)
    ow = torch.arange(ovol[2]).view(1, 1, 1, 1, -1)
    return ((d - (2 * od - 1)) * 3 + (h - (2 * oh - 1))) * 3 + (w - (2 * ow - 1))


POOL_SHAPES = [(2, 8, 5, 6, 7), (1, 8, 4, 4, 4), (2, 8, 1, 1, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize('shape', POOL_SHAPES)
@pytest.mark.parametrize('family', ['gauss', 'negative', 'constant', 'ties'])
def test_maxpool_matches_torch(shape, family):
    g = torch.Generator().manual_seed(51)
    if family == 'gauss':
        x = torch.randn(shape, generator=g)
    elif family == 'negative':                                        # a zero pad would win here
        x = -1.0 - torch.rand(shape, generator=g)
    elif family == 'constant':
        x = torch.full(shape, 2.5)
    else:
        x = torch.randint(0, 3, shape, generator=g).to(F32)           # many ties: the first maximum in (d, h, w) order
    y, y16, idx, ovol = run_pool(x)
    ty, tidx = F.max_pool3d(x.double(), 3, 2, 1, return_indices=True)
    assert torch.equal(uncl(y.double().cpu(), shape[0], ovol), ty)
    assert torch.equal(y16.view(torch.int16), y.to(BF16).view(torch.int16))
    if family == 'negative':
        assert bool((y < 0).all())
    want = torch_tap_index(tidx, shape, ovol)
    assert torch.equal(uncl(idx.cpu().long(), shape[0], ovol), want)
    # the gradient on integers equals torch's exactly: every dy goes where torch's index sends it
    dy = torch.randint(-3, 4, ty.shape, generator=g).to(F32)
    xr = x.double().requires_grad_(True)
    F.max_pool3d(xr, 3, 2, 1).backward(dy.double())
    dx, dx16 = run_pool_bwd(dy, idx, shape)
    assert torch.equal(uncl(dx.double().cpu(), shape[0], shape[2:]), xr.grad)
    assert torch.equal(dx16.view(torch.int16), dx.to(BF16).view(torch.int16))


@pytest.mark.gpu
def test_maxpool_nan_propagates():
    shape = (1, 8, 5, 6, 7)
    g = torch.Generator().manual_seed(52)
    x = torch.randn(shape, generator=g)
    x[0, 3, 2, 3, 4] = float('nan')
    x[0, 5, 0, 0, 0] = float('nan'); x[0, 5, 0, 0, 1] = float('nan')   # two in one window: torch keeps the last one it meets
    y, _, idx, ovol = run_pool(x)
    ty, tidx = F.max_pool3d(x, 3, 2, 1, return_indices=True)
    got = uncl(y.cpu(), 1, ovol)
    assert torch.equal(torch.isnan(got), torch.isnan(ty)) and int(torch.isnan(ty).sum()) > 1
    assert torch.equal(got[~torch.isnan(ty)], ty[~torch.isnan(ty)])
    assert torch.equal(uncl(idx.cpu().long(), 1, ovol), torch_tap_index(tidx, shape, ovol))


# ---------------------------------------------------------------------------- rows-mean
@pytest.mark.gpu
@pytest.mark.parametrize('N,S,C', [(4, 54, 32), (2, 1, 4), (3, 7, 512)])
def test_rows_mean_exact_on_integers(N, S, C):
    g = torch.Generator().manual_seed(61)
    x = (torch.randint(-3, 4, (N, S, C), generator=g) * S).to(F32)     # multiples of S: the mean is an integer
    xd = operand(x, F32)
    y, y16 = Out((N, C)), Out((N, C), BF16)
    _lib().vitae_rows_mean_fwd(xd.data_ptr(), y.ptr(), y16.ptr(), N, S, C, _stream())
    torch.cuda.synchronize()
    assert torch.equal(y.intact().double().cpu(), x.double().mean(1))
    assert torch.equal(y16.intact().view(torch.int16), y.t.to(BF16).view(torch.int16))
    dy = (torch.randint(-3, 4, (N, C), generator=g) * S).to(F32)
    dyd = operand(dy, F32)
    dx, dx16 = Out((N, S, C)), Out((N, S, C), BF16)
    _lib().vitae_rows_mean_bwd(dyd.data_ptr(), dx.ptr(), dx16.ptr(), N, S, C, _stream())
    torch.cuda.synchronize()
    assert torch.equal(dx.intact().double().cpu(), (dy.double() / S)[:, None, :].expand(N, S, C))
    assert torch.equal(dx16.intact().view(torch.int16), dx.t.to(BF16).view(torch.int16))


# ---------------------------------------------------------------------------- BatchNorm (+ residual) (+ ReLU)
def bn_tail_ref(x, res, w, b, relu, eps, dt):
    """-> y, mean, rstd, unbiased variance (two-pass)"""
    x, w, b = x.to(dt), w.to(dt), b.to(dt)
    R = x.shape[0]
    mean = x.mean(0)
    d = x - mean
    q = (d * d).sum(0)
    rstd = (q / R + eps).rsqrt()
    y = d * (rstd * w) + b
    if res is not None:
        y = y + res.to(dt)
    return (y.clamp_min(0) if relu else y), mean, rstd, q / max(R - 1, 1)


def bn_tail_bwd_ref(dy, x, y_given, w, mean, rstd, relu, dt):
    dy, x, w, mean, rstd = dy.to(dt), x.to(dt), w.to(dt), mean.to(dt), rstd.to(dt)
    R = x.shape[0]
    g = dy * (y_given > 0).to(dt) if relu else dy
    xh = (x - mean) * rstd
    dx = w * rstd * (g - g.sum(0) / R - xh * ((g * xh).sum(0) / R))
    return dx, g, (g * xh), g


def torch_bn_tail(x, res, w, b, relu, eps, rm, rv):
    rm, rv = rm.clone(), rv.clone()
    y = F.batch_norm(x, rm, rv, w, b, True, MOM, eps)
    if res is not None:
        y = y + res
    var, mean = torch.var_mean(x, 0, unbiased=False)
    return (F.relu(y) if relu else y), mean, (var + eps).rsqrt(), rm, rv


def _ratio(num, den):
    inf, zero = torch.full_like(num, float('inf')), torch.zeros_like(num)
    return torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num == 0, zero, inf))


def col_err(a, ref, scale=None):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float(_ratio((a - ref).abs().amax(0), ref.abs().amax(0) if scale is None else scale.double().cpu()).max())


def vec_err(a, ref, den):
    return float(_ratio((a.detach().double().cpu() - ref.double()).abs(), den.double()).max())


def bn_inputs(R, C, family, seed):
    g = torch.Generator().manual_seed(seed)
    if family == 'plain':
        x = 0.3 + 2.0 * torch.randn(R, C, generator=g)
    else:                                                             # offset: mean 1000, deviation 1
        x = 1000.0 * (1 - 2 * (torch.arange(C) % 2)).float() + torch.randn(R, C, generator=g)
    res = torch.randn(R, C, generator=g)
    w = 0.5 + torch.rand(C, generator=g)
    b = 0.3 * torch.randn(C, generator=g)
    dy = torch.randn(R, C, generator=g)
    rm, rv = torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    return x, res, w, b, dy, rm, rv


BN_SHAPES = [(2, 4), (31, 8), (100, 64), (97, 64), (1000, 4), (130, 128), (1100, 128)]      # one split, several, a ragged last


@pytest.mark.gpu
@pytest.mark.parametrize('family', ['plain', 'offset'])
@pytest.mark.parametrize('relu,has_res', [(1, 0), (1, 1), (0, 0), (0, 1)])
@pytest.mark.parametrize('R,C', BN_SHAPES)
def test_bn_tail_forward_and_backward(R, C, relu, has_res, family):
    lib, st = _lib(), _stream()
    x, res, w, b, dy, rm0, rv0 = bn_inputs(R, C, family, 71)
    if not has_res:
        res = None
    label = f'bn_tail R={R} C={C} relu={relu} res={has_res} {family}'
    xd, wd, bd = operand(x, F32), operand(w, F32), operand(b, F32)
    resd = operand(res, F32) if has_res else None
    y, y16, mean, rstd = Out((R, C)), Out((R, C), BF16), Out((C,)), Out((C,))
    rm, rv, nbt = Out((C,)), Out((C,)), torch.full((1,), 5, dtype=torch.int64, device='cuda')
    rm.t.copy_(rm0); rv.t.copy_(rv0)
    nws = lib.vitae_bn1d_split_ws_floats(R, C)
    ws = Out((nws,), fill=float('nan'))
    lib.vitae_bn_tail_fwd_split(xd.data_ptr(), resd.data_ptr() if has_res else None, wd.data_ptr(), bd.data_ptr(), y.ptr(), y16.ptr(), mean.ptr(),
                                rstd.ptr(), rm.ptr(), rv.ptr(), nbt.data_ptr(), R, C, EPS_BN, MOM, relu, ws.ptr(), st)
    torch.cuda.synchronize()
    for o in (y, y16, mean, rstd, rm, rv, ws):
        o.intact()
    assert int(nbt) == 6
    y64, m64, r64, uv64 = bn_tail_ref(x, res, w, b, relu, EPS_BN, F64)
    f32s = [bn_tail_ref(x, res, w, b, relu, EPS_BN, F32), torch_bn_tail(x, res, w, b, relu, EPS_BN, rm0, rv0)]
    within(label + ' y', col_err(y.t, y64), max(col_err(f[0], y64) for f in f32s))
    assert torch.equal(y16.t.view(torch.int16), y.t.to(BF16).view(torch.int16))
    std64 = 1 / r64
    within(label + ' mean', vec_err(mean.t, m64, m64.abs() + std64), max(vec_err(f[1], m64, m64.abs() + std64) for f in f32s))
    within(label + ' rstd', vec_err(rstd.t, r64, r64.abs()), max(vec_err(f[2], r64, r64.abs()) for f in f32s))
    # running statistics: error in units of the sum of the absolute addends
    rm64, rmden = (1 - MOM) * rm0.double() + MOM * m64, (1 - MOM) * rm0.double().abs() + MOM * m64.abs()
    rv64, rvden = (1 - MOM) * rv0.double() + MOM * uv64, (1 - MOM) * rv0.double().abs() + MOM * uv64.abs()
    t = f32s[1]
    e32m = max(vec_err(t[3], rm64, rmden), vec_err((1 - MOM) * rm0 + MOM * f32s[0][1], rm64, rmden))
    e32v = max(vec_err(t[4], rv64, rvden), vec_err((1 - MOM) * rv0 + MOM * f32s[0][3], rv64, rvden))
    within(label + ' running_mean', vec_err(rm.t, rm64, rmden), e32m)
    within(label + ' running_var', vec_err(rv.t, rv64, rvden), e32v)

    # backward, fed by the forward's own outputs; the mask is y > 0 of the y the kernel is given
    dyd = operand(dy, F32)
    dx, dx16, dres = Out((R, C)), Out((R, C), BF16), Out((R, C))
    dw0, db0 = torch.randn(C), torch.randn(C)
    dw, db = Out((C,)), Out((C,))
    dw.t.copy_(dw0); db.t.copy_(db0)
    ws2 = Out((nws,), fill=float('nan'))
    lib.vitae_bn_tail_bwd_split(dyd.data_ptr(), xd.data_ptr(), y.ptr() if relu else None, wd.data_ptr(), mean.ptr(), rstd.ptr(), dx.ptr(), dx16.ptr(),
                                dres.ptr() if has_res else None, dw.ptr(), db.ptr(), R, C, relu, ws2.ptr(), st)
    torch.cuda.synchronize()
    for o in (dx, dx16, dres, dw, db, ws2):
        o.intact()
    yk = y.t.cpu()
    dx64, g64, dwt64, dbt64 = bn_tail_bwd_ref(dy, x, yk, w, m64, r64, relu, F64)
    if has_res:
        assert torch.equal(dres.t.cpu(), g64.float())                # the masked gradient itself
    else:
        dres.untouched()
    dx32, _, dwt32, dbt32 = bn_tail_bwd_ref(dy, x, yk, w, f32s[0][1], f32s[0][2], relu, F32)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    F.batch_norm(xr, None, None, wr, br, True, MOM, EPS_BN).backward(g64.float())
    scale = w.double().abs() * r64 * g64.abs().amax(0)
    within(label + ' dx', col_err(dx.t, dx64, scale), max(col_err(dx32, dx64, scale), col_err(xr.grad, dx64, scale)))
    assert torch.equal(dx16.t.view(torch.int16), dx.t.to(BF16).view(torch.int16))
    dw64, dwden = dw0.double() + dwt64.sum(0), dw0.double().abs() + dwt64.abs().sum(0)
    db64, dbden = db0.double() + dbt64.sum(0), db0.double().abs() + dbt64.abs().sum(0)
    within(label + ' dw', vec_err(dw.t, dw64, dwden), max(vec_err(dw0 + dwt32.sum(0), dw64, dwden), vec_err(dw0 + wr.grad, dw64, dwden)))
    within(label + ' db', vec_err(db.t, db64, dbden), max(vec_err(db0 + dbt32.sum(0), db64, dbden), vec_err(db0 + br.grad, db64, dbden)))


@pytest.mark.gpu
@pytest.mark.parametrize('relu,has_res', [(1, 0), (1, 1), (0, 0), (0, 1)])
@pytest.mark.parametrize('R,C', [(2, 4), (97, 64), (1100, 128)])
def test_bn_tail_eval(R, C, relu, has_res):
    x, res, w, b, _, rm, rv = bn_inputs(R, C, 'plain', 81)
    res = res if has_res else None
    ops = [operand(t, F32) for t in (x, w, b, rm, rv)]
    resd = operand(res, F32) if has_res else None
    y, y16 = Out((R, C)), Out((R, C), BF16)
    _lib().vitae_bn_tail_eval(ops[0].data_ptr(), resd.data_ptr() if has_res else None, ops[1].data_ptr(), ops[2].data_ptr(), ops[3].data_ptr(),
                              ops[4].data_ptr(), y.ptr(), y16.ptr(), R, C, EPS_BN, relu, _stream())
    torch.cuda.synchronize()

    def ref(dt):
        v = (x.to(dt) - rm.to(dt)) * (rv.to(dt) + EPS_BN).rsqrt() * w.to(dt) + b.to(dt)
        v = v + res.to(dt) if has_res else v
        return v.clamp_min(0) if relu else v

    t32 = F.batch_norm(x, rm, rv, w, b, False, MOM, EPS_BN)
    t32 = t32 + res if has_res else t32
    t32 = F.relu(t32) if relu else t32
    within(f'bn_tail_eval R={R} C={C} relu={relu} res={has_res}', col_err(y.intact(), ref(F64)), max(col_err(ref(F32), ref(F64)), col_err(t32, ref(F64))))
    assert torch.equal(y16.intact().view(torch.int16), y.t.to(BF16).view(torch.int16))
