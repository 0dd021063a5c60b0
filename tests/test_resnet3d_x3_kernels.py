"""The split-operand convolutions of the fp32x3 route (csrc/conv3d.hip's OpX3 instances) through the C ABI, where they can go wrong.

Every fp32 operand enters the bf16 MFMA as hi = bf16(v), lo = bf16(v - hi); a product is hi.hi + hi.lo + lo.hi.

Exact on integers (forward, input gradient, weight gradient).  With integer operands hi and lo are integers, so as long as the
absolute values of the three terms sum to less than 2^24 per output (asserted on the operands, from their CPU split) every partial
sum is exact in fp32 and the result must EQUAL  sum (x w - x_lo w_lo)  evaluated in float64:
  lo_row     the row operand (x, dy) odd with |v| < 2^11 (lo != 0), the other |v| <= 7 (lo == 0): the result is float64's convolution;
             pins hi.hi and lo.hi
  lo_other   the roles swapped: pins hi.lo
  both       both operands in [257, 511] (9 bits: lo != 0 for the odd half), reductions of at most 48 addends: only the dropped
             lo.lo term separates the result from float64's
For the weight gradient both operands are "row" operands; the same three kinds, lo_row = dy wide, lo_other = x wide.

Per element against float64: |err| <= 2^-14 sum |a||b| on Gaussian, offset (N(100, 1)) and mixed-sign-magnitude operands.  bf16's
unit round-off is 2^-8, so a split operand is carried to 2^-16; the three neglected pieces x_lo w_lo, e_x w, x e_w are each at most
2^-16 |x||w|, a 128-value fp32 chain adds at most 2^-17.  The bf16 kernels sit near 2^-8 and a build that drops a cross term near
2^-10 of sum |a||b|: both fail.  ``RATIO`` lines are printed (run with -s).

Operands sit between NaN-filled guards, outputs and workspaces have sentinels behind them, repeats are bit-equal, every refusal
leaves the outputs untouched."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
GUARD, SENT = 64, 7.25
BOUND = 2.0 ** -14
EXACT = 2 ** 24


def conv_case(N, vol, cin, cout, k, s, p):
    return dict(N=N, vol=vol, Cin=cin, Cout=cout, k=(k,) * 3 if isinstance(k, int) else k, s=s, p=(p,) * 3 if isinstance(p, int) else p)


V = (5, 6, 7)
CASES = {
    'k1s2_8_36': conv_case(2, V, 8, 36, 1, (2, 2, 2), 0),                 # K = 8; 72 rows; a ragged second column tile
    'k1s2_12_4': conv_case(2, V, 12, 4, 1, (2, 2, 2), 0),
    'k3_4_4': conv_case(2, V, 4, 4, 3, (1, 1, 1), 1),                     # K = 108: no multiple of 16; 420 rows
    'k3_8_36': conv_case(2, V, 8, 36, 3, (1, 1, 1), 1),                   # K = 216: a flush
    'k3_12_36': conv_case(2, V, 12, 36, 3, (1, 1, 1), 1),                 # K = 324: Cin no power of two, 16-byte gathers
    'k3_1_4': conv_case(2, V, 1, 4, 3, (1, 1, 1), 1),                     # K = 27, scalar gathers
    'k3s2_8_4': conv_case(2, V, 8, 4, 3, (2, 2, 2), 1),                   # -> (3, 3, 4): 72 rows
    'k3s2_4_36': conv_case(2, V, 4, 36, 3, (2, 2, 2), 1),
    'k7_1_36': conv_case(2, V, 1, 36, 7, (1, 2, 2), 3),                   # the stem: K = 343, 120 rows
    'k7_4_4': conv_case(2, V, 4, 4, 7, (1, 2, 2), 3),                     # K = 1372: eleven flushes
}
CASE_IDS = list(CASES)
# reductions of at most 48 addends in all three products (kind 'both')
SHORT = {
    'k1_8_36': conv_case(1, (2, 3, 4), 8, 36, 1, (1, 1, 1), 0),           # K = 8, K' = 36, M = 24
    'k3_1_4': conv_case(1, (2, 2, 3), 1, 4, 3, (1, 1, 1), 1),             # K = 27, M = 12, at most 12 voxels x 4 channels
    'k3s2_1_4': conv_case(1, (3, 3, 4), 1, 4, 3, (2, 2, 2), 1),           # K = 27, M = 8, at most 8 outputs x 4 channels per voxel
}
BIG_WGRAD = conv_case(2, (13, 13, 13), 4, 4, 1, (1, 1, 1), 0)             # 4394 rows: two chunks


def out_vol(c):
    return tuple((c['vol'][i] + 2 * c['p'][i] - c['k'][i]) // c['s'][i] + 1 for i in range(3))


def geo_args(c):
    return (c['N'], *c['vol'], c['Cin'], c['Cout'], *c['k'], *c['s'], *c['p'])


def shapes(c):
    return (c['N'], c['Cin'], *c['vol']), (c['Cout'], c['Cin'], *c['k']), (c['N'], c['Cout'], *out_vol(c))


def split(t):
    hi = t.float().to(BF16).double()
    return hi, (t.double() - hi).float().to(BF16).double()


def wide(shape, g, bits=11):
    """odd integers with |v| < 2^bits: more bits than bf16 holds"""
    return ((2 * torch.randint(0, 2 ** (bits - 1), shape, generator=g) + 1) * (2 * torch.randint(0, 2, shape, generator=g) - 1)).to(F32)


def narrow(shape, g):
    return torch.randint(-7, 8, shape, generator=g).to(F32)


def nine_bits(shape, g):
    return torch.randint(257, 512, shape, generator=g).to(F32)


def int_operands(c, kind, which, seed, bits=11):
    """-> x, w, dy for the product `which` ('fwd' | 'dx' | 'dw'); the operand the product does not read is None"""
    g = torch.Generator().manual_seed(seed)
    sx, sw, sy = shapes(c)
    first, second = {'fwd': (sx, sw), 'dx': (sy, sw), 'dw': (sy, sx)}[which]      # (row operand, other operand)
    if kind == 'both':
        a, b = nine_bits(first, g), nine_bits(second, g)
    elif kind == 'lo_row':
        a, b = wide(first, g, bits), narrow(second, g)
    else:
        a, b = narrow(first, g), wide(second, g, bits)
    small, big = (b, a) if kind == 'lo_row' else (a, b)
    if kind != 'both':
        assert bool((split(small)[1] == 0).all()) and bool((split(big)[1] != 0).any())
    else:
        assert bool((split(a)[1] != 0).any()) and bool((split(b)[1] != 0).any())
    return {'fwd': (a, b, None), 'dx': (None, b, a), 'dw': (b, None, a)}[which]


def _native(fn):
    """torch's own CPU convolution with oneDNN off (its fp32 stem weight gradient corrupts the heap in this torch build)"""
    def wrapped(*a, **k):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            with torch.backends.mkldnn.flags(enabled=False):
                return fn(*a, **k)
    return wrapped


@_native
def ref_fwd(x, w, c):
    return F.conv3d(x.double(), w.double(), None, c['s'], c['p'])


@_native
def ref_dx(dy, w, c):
    return torch.nn.grad.conv3d_input((c['N'], c['Cin'], *c['vol']), w.double(), dy.double(), c['s'], c['p'])


@_native
def ref_dw(x, dy, c):
    return torch.nn.grad.conv3d_weight(x.double(), (c['Cout'], c['Cin'], *c['k']), dy.double(), c['s'], c['p'])


def x3_expectation(ref, a, b, c):
    """-> (sum (a b - a_lo b_lo) in float64, sum of the absolute values of the three terms): what the kernel must give on integers,
    and the figure that has to stay below 2^24 for that"""
    (ah, al), (bh, bl) = split(a), split(b)
    want = ref(a, b, c) - ref(al, bl, c)
    mass = ref(ah.abs(), bh.abs() + bl.abs(), c) + ref(al.abs(), bh.abs(), c)
    return want, float(mass.max())


def cl(t):
    """[N, C, D, H, W] -> channels-last rows [N D H W, C]"""
    return t.permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1]).contiguous()


def uncl(rows, N, vol):
    return rows.reshape(N, *vol, rows.shape[-1]).permute(0, 4, 1, 2, 3).contiguous()


# ---------------------------------------------------------------------------- CPU
def test_abi_declares_the_x3_entry_points():
    from vit_ae_plus_plus_amd import _abi
    for name in ('vitae_conv3d_fwd_x3', 'vitae_conv3d_bwd_input_x3', 'vitae_conv3d_bwd_weight_x3', 'vitae_conv3d_pack_weight_x3',
                 'vitae_conv3d_packed_elems_x3', 'vitae_to_channels_last_f32'):
        assert name in _abi.PROTOS, name
    assert _abi.PROTOS['vitae_conv3d_fwd_x3'][1] == _abi.PROTOS['vitae_conv3d_fwd'][1]
    assert _abi.PROTOS['vitae_conv3d_bwd_input_x3'][1] == _abi.PROTOS['vitae_conv3d_bwd_input'][1]
    assert _abi.PROTOS['vitae_conv3d_bwd_weight_x3'][1] == _abi.PROTOS['vitae_conv3d_bwd_weight'][1]
    assert _abi.CONSTS['VITAE_CONV3D_PACK_FORM_X3'] == 4
    lib = _abi.lib
    assert lib.vitae_conv3d_packed_elems_x3(64, 1, 7, 7, 7, 0) == 2 * 64 * 352
    assert lib.vitae_conv3d_packed_elems_x3(8, 4, 3, 3, 3, 1) == 2 * 4 * 224
    assert lib.vitae_conv3d_packed_elems_x3(8, 4, 3, 9, 3, 1) == 0
    # the table's host side: the two-plane forms count twice the elements; every other new value of the form word is refused
    row = (4096, 8192, 8, 4, 3, 3, 3)
    for form, groups in ((0, 8 * 112 // 8), (4, 2 * 8 * 112 // 8), (5, 2 * 4 * 224 // 8)):
        t = np.array([row + (form,)] * 40, dtype=np.int64)
        t[:, 1] += 16 * np.arange(40)
        assert lib.vitae_conv3d_pack_multi_chunks(t.ctypes.data, 40) == -(-40 * groups * 8 // _abi.CONSTS['VITAE_CONV3D_PACK_CHUNK']), form
    for form in (2, 3, 6, 7, 8, -1):
        t = np.array([row + (form,)], dtype=np.int64)
        assert lib.vitae_conv3d_pack_multi_chunks(t.ctypes.data, 1) == 0, form


def test_cases_cover_the_paths():
    K = {n: c['Cin'] * int(np.prod(c['k'])) for n, c in CASES.items()}
    M = {n: c['N'] * int(np.prod(out_vol(c))) for n, c in CASES.items()}
    assert {c['Cin'] for c in CASES.values()} == {1, 4, 8, 12} and {c['Cout'] for c in CASES.values()} == {4, 36}
    assert any(k % 16 and k > 128 for k in K.values()) and any(k < 16 for k in K.values()) and max(K.values()) == 1372
    assert any(m < 128 for m in M.values()) and any(m > 128 and m % 128 for m in M.values())
    assert BIG_WGRAD['N'] * int(np.prod(out_vol(BIG_WGRAD))) == 4394
    for c in SHORT.values():                                         # 'both': at most 48 addends, so 48 (2^18 + 2 x 2^9 x 2) < 2^24
        sx, sw, sy = shapes(c)
        one = torch.ones
        assert max(float(ref_fwd(one(sx), one(sw), c).max()), float(ref_dx(one(sy), one(sw), c).max()), float(ref_dw(one(sx), one(sy), c).max())) <= 48
    assert 48 * (512 * 512 + 2 * 512 * 2) < EXACT


def test_the_split_carries_sixteen_bits_and_the_expectation_is_the_three_terms():
    g = torch.Generator().manual_seed(5)
    v = torch.randn(4096, generator=g) * torch.logspace(-6, 6, 4096)
    hi, lo = split(v)
    assert float(((hi + lo - v.double()).abs() / v.double().abs()).max()) <= 2.0 ** -16
    c = SHORT['k3_1_4']
    x, w, _ = int_operands(c, 'both', 'fwd', 1)
    want, mass = x3_expectation(ref_fwd, x, w, c)
    (xh, xl), (wh, wl) = split(x), split(w)
    assert torch.equal(want, ref_fwd(xh, wh, c) + ref_fwd(xh, wl, c) + ref_fwd(xl, wh, c)) and mass < EXACT
    assert not torch.equal(want, ref_fwd(x, w, c))                    # the dropped term is visible


# ---------------------------------------------------------------------------- GPU plumbing
def _lib():
    from vit_ae_plus_plus_amd import _abi
    return _abi.lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def operand(t, dtype=F32):
    """A device copy of t between two NaN-filled guard regions (a read outside the operand poisons the result); 16-byte aligned."""
    n = t.numel()
    buf = torch.full((n + 2 * GUARD,), float('nan'), dtype=dtype, device='cuda')
    view = buf[GUARD:GUARD + n].view(t.shape)
    view.copy_(t.to(dtype))
    view._guard = buf
    assert view.data_ptr() % 16 == 0
    return view


class Out:
    """An output (or workspace) with sentinels behind it; `fill` is what an element nobody wrote shows."""

    def __init__(self, shape, dtype=F32, fill=SENT):
        n = int(np.prod(shape))
        self.n, self.fill = n, fill
        self.buf = torch.full((n + GUARD,), fill, dtype=dtype, device='cuda')
        self.buf[n:] = SENT
        self.t = self.buf[:n].view(shape)

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        assert bool((self.buf[self.n:] == SENT).all()), 'sentinels behind an output were overwritten'
        return self.t

    def untouched(self):
        self.intact()
        assert bool((self.buf[:self.n] == self.fill).all()), 'a refused call wrote to its output'


def dev_pack(w, transposed):
    lib = _lib()
    geo = (*w.shape, transposed)
    n = lib.vitae_conv3d_packed_elems_x3(*geo)
    wd = operand(w)
    out = Out((n,), BF16)
    lib.vitae_conv3d_pack_weight_x3(wd.data_ptr(), out.ptr(), *geo, _stream())
    torch.cuda.synchronize()
    return operand(out.intact().float().cpu(), BF16)                 # between NaN guards, as every operand


def run_fwd(c, x, wpk, want=('f32', 'bf16')):
    M = c['N'] * int(np.prod(out_vol(c)))
    xd = operand(cl(x))
    y = Out((M, c['Cout'])) if 'f32' in want else None
    y16 = Out((M, c['Cout']), BF16) if 'bf16' in want else None
    _lib().vitae_conv3d_fwd_x3(xd.data_ptr(), wpk.data_ptr(), y.ptr() if y else None, y16.ptr() if y16 else None, *geo_args(c), _stream())
    torch.cuda.synchronize()
    return (y.intact() if y else None), (y16.intact() if y16 else None)


def run_dx(c, dy, wpkt, want=('f32', 'bf16'), base=None):
    Vx = c['N'] * int(np.prod(c['vol']))
    dyd = operand(cl(dy))
    dx = Out((Vx, c['Cin'])) if 'f32' in want else None
    dx16 = Out((Vx, c['Cin']), BF16) if 'bf16' in want else None
    if base is not None:
        dx.t.copy_(base)
    _lib().vitae_conv3d_bwd_input_x3(dyd.data_ptr(), wpkt.data_ptr(), dx.ptr() if dx else None, dx16.ptr() if dx16 else None,
                                     0 if base is None else 1, *geo_args(c), _stream())
    torch.cuda.synchronize()
    return (dx.intact() if dx else None), (dx16.intact() if dx16 else None)


def run_dw(c, x, dy, accumulate=None):
    lib = _lib()
    xd, dyd = operand(cl(x)), operand(cl(dy))
    n = lib.vitae_conv3d_wgrad_ws_floats(*geo_args(c))
    ws = Out((n,), fill=float('nan'))
    dw = Out((c['Cout'], c['Cin'], *c['k']))
    if accumulate is not None:
        dw.t.copy_(accumulate)
    lib.vitae_conv3d_bwd_weight_x3(dyd.data_ptr(), xd.data_ptr(), dw.ptr(), ws.ptr(), n, 0 if accumulate is None else 1, *geo_args(c), _stream())
    torch.cuda.synchronize()
    ws.intact()
    assert not bool(torch.isnan(ws.t).any()), 'a workspace element was never written'
    return dw.intact()


def rows_to(t, c, which):
    vol = out_vol(c) if which == 'y' else c['vol']
    return uncl(t.double().cpu(), c['N'], vol)


def run_product(c, which, x, w, dy, **kw):
    """-> the fp32 result in torch layout (float64, CPU), its bf16 copy or None, and the reference function with its two operands"""
    if which == 'fwd':
        y, y16 = run_fwd(c, x, dev_pack(w, 0), **kw)
        return rows_to(y, c, 'y'), (y, y16), (ref_fwd, x, w)
    if which == 'dx':
        dx, dx16 = run_dx(c, dy, dev_pack(w, 1), **kw)
        return rows_to(dx, c, 'x'), (dx, dx16), (ref_dx, dy, w)
    dw = run_dw(c, x, dy, **kw)
    return dw.double().cpu(), (dw, None), (ref_dw, x, dy)


# ---------------------------------------------------------------------------- packing, input layout
@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(4, 1, 7, 7, 7), (8, 4, 3, 3, 3), (36, 12, 3, 3, 3), (36, 8, 1, 1, 1)])
def test_two_plane_packing(shape):
    """hi + lo against the weight per element (2^-16 |w|), the zero tails, and the table launch bit-equal to the single one"""
    lib = _lib()
    g = torch.Generator().manual_seed(1)
    w = torch.randn(shape, generator=g) * torch.logspace(-3, 3, int(np.prod(shape))).view(shape)
    co, ci = shape[:2]
    taps = int(np.prod(shape[2:]))
    wd = operand(w)
    singles = []
    for tr in (0, 1):
        got = dev_pack(w, tr).cpu()
        singles.append(got)
        w3 = w.reshape(co, ci, taps)
        m = w3.permute(1, 2, 0).reshape(ci, taps * co) if tr else w3.permute(0, 2, 1).reshape(co, taps * ci)
        K = m.shape[1]
        kp = (K + 15) // 16 * 16
        planes = got.view(m.shape[0], 2, kp)
        hi, lo = planes[:, 0, :K].double(), planes[:, 1, :K].double()
        assert torch.equal(planes[:, 0, :K].view(torch.int16), m.to(BF16).view(torch.int16)), (shape, tr)      # hi is the bf16 route's operand
        assert bool(((hi + lo - m.double()).abs() <= 2.0 ** -16 * m.double().abs()).all()), (shape, tr)
        assert bool((planes[:, :, K:].view(torch.int16) == 0).all()), 'the tail of a plane is not zero'
    # one table: both two-plane forms and, between them, the single-plane forward form (forms 4, 0, 5)
    sizes = [singles[0].numel(), lib.vitae_conv3d_packed_elems(*shape, 0), singles[1].numel()]
    outs = [Out((n,), BF16) for n in sizes]
    table = np.array([(wd.data_ptr(), o.ptr(), *shape, form) for o, form in zip(outs, (4, 0, 5))], dtype=np.int64)
    nc = int(lib.vitae_conv3d_pack_multi_chunks(table.ctypes.data, 3))
    assert nc == -(-sum(sizes) // 4096)
    chunks = np.zeros((nc, 2), dtype=np.int32)
    lib.vitae_conv3d_pack_multi_chunk_list(table.ctypes.data, 3, chunks.ctypes.data, nc)
    td, cd = torch.from_numpy(table.copy()).cuda(), torch.from_numpy(chunks.copy()).cuda()
    lib.vitae_conv3d_pack_weights_multi(table.ctypes.data, td.data_ptr(), 3, chunks.ctypes.data, cd.data_ptr(), nc, _stream())
    torch.cuda.synchronize()
    assert torch.equal(outs[0].intact().cpu().view(torch.int16), singles[0].view(torch.int16))
    assert torch.equal(outs[2].intact().cpu().view(torch.int16), singles[1].view(torch.int16))
    one = Out((sizes[1],), BF16)
    lib.vitae_conv3d_pack_weight(wd.data_ptr(), one.ptr(), *shape, 0, _stream())
    torch.cuda.synchronize()
    assert torch.equal(outs[1].intact().view(torch.int16), one.intact().view(torch.int16))


@pytest.mark.gpu
def test_channels_last_f32_bit_for_bit():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 3, 4, 5, 6, generator=g)
    for j, v in enumerate((float('nan'), float('inf'), -0.0, 1e-40)):      # a copy keeps every bit pattern
        x.view(-1)[11 * j + 3] = v
    xd = operand(x)
    out = Out((2 * 4 * 5 * 6, 3))
    _lib().vitae_to_channels_last_f32(xd.data_ptr(), out.ptr(), 2, 3, 4, 5, 6, _stream())
    torch.cuda.synchronize()
    assert torch.equal(out.intact().cpu().view(torch.int32), cl(x).view(torch.int32))


# ---------------------------------------------------------------------------- exact on integers
def assert_exact(c, kind, which, seed, bits=11):
    x, w, dy = int_operands(c, kind, which, seed, bits)
    got, (f32, b16), (ref, a, b) = run_product(c, which, x, w, dy)
    want, mass = x3_expectation(ref, a, b, c)
    assert mass < EXACT, (kind, which, mass)
    assert torch.equal(got, want), (kind, which, float((got - want).abs().max()))
    if kind != 'both':
        assert torch.equal(want, ref(a, b, c))                        # one lo is zero: float64's convolution itself
    if b16 is not None:
        assert torch.equal(b16.view(torch.int16), f32.to(BF16).view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['fwd', 'dx', 'dw'])
@pytest.mark.parametrize('name', CASE_IDS)
def test_exact_on_integers_one_operand_wide(name, which):
    for i, kind in enumerate(('lo_row', 'lo_other')):
        assert_exact(CASES[name], kind, which, 11 + i)


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['fwd', 'dx', 'dw'])
@pytest.mark.parametrize('name', list(SHORT))
def test_exact_on_integers_both_operands_wide(name, which):
    assert_exact(SHORT[name], 'both', which, 13)


@pytest.mark.gpu
def test_wgrad_two_chunks_exact_and_repeatable():
    c = BIG_WGRAD
    assert _lib().vitae_conv3d_wgrad_ws_floats(*geo_args(c)) == 2 * 4 * 4
    for i, kind in enumerate(('lo_row', 'lo_other')):
        x, _, dy = int_operands(c, kind, 'dw', 17 + i, bits=9)
        want, mass = x3_expectation(ref_dw, x, dy, c)
        assert mass < EXACT
        dw = run_dw(c, x, dy)
        assert torch.equal(dw.double().cpu(), want) and torch.equal(want, ref_dw(x, dy, c))
        assert torch.equal(run_dw(c, x, dy).view(torch.int32), dw.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['k3_4_4', 'k3s2_8_4'])
def test_accumulate_adds_to_what_the_output_held(name):
    c = CASES[name]
    x, w, _ = int_operands(c, 'lo_row', 'fwd', 21)
    _, _, dy = int_operands(c, 'lo_row', 'dx', 22)
    g = torch.Generator().manual_seed(23)
    dx, _ = run_dx(c, dy, dev_pack(w, 1))
    held = torch.randint(-5, 6, dx.shape, generator=g).to(F32)
    dx2, dx216 = run_dx(c, dy, dev_pack(w, 1), base=held.cuda())
    assert torch.equal(dx2.double().cpu(), dx.double().cpu() + held.double())
    assert torch.equal(dx216.view(torch.int16), dx2.to(BF16).view(torch.int16))
    x, _, dy = int_operands(c, 'lo_row', 'dw', 24)
    dw = run_dw(c, x, dy)
    base = torch.randint(-5, 6, dw.shape, generator=g).to(F32)
    assert torch.equal(run_dw(c, x, dy, accumulate=base.cuda()).double().cpu(), dw.double().cpu() + base.double())


@pytest.mark.gpu
def test_only_one_output_requested_gives_the_same_bits():
    c = CASES['k3_4_4']
    g = torch.Generator().manual_seed(3)
    sx, sw, sy = shapes(c)
    x, w, dy = torch.randn(sx, generator=g), torch.randn(sw, generator=g), torch.randn(sy, generator=g)
    wpk, wpkt = dev_pack(w, 0), dev_pack(w, 1)
    y, y16 = run_fwd(c, x, wpk)
    assert torch.equal(run_fwd(c, x, wpk, want=('f32',))[0], y) and torch.equal(run_fwd(c, x, wpk, want=('bf16',))[1], y16)
    dx, dx16 = run_dx(c, dy, wpkt)
    assert torch.equal(run_dx(c, dy, wpkt, want=('f32',))[0], dx) and torch.equal(run_dx(c, dy, wpkt, want=('bf16',))[1], dx16)


# ---------------------------------------------------------------------------- per element
def family(kind, shape, g):
    if kind == 'gauss':
        return torch.randn(shape, generator=g)
    if kind == 'offset':
        return 100.0 + torch.randn(shape, generator=g)
    return torch.randn(shape, generator=g) * 10.0 ** (6 * torch.rand(shape, generator=g) - 3)      # mixed signs, six decades


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['gauss', 'offset', 'mixed'])
@pytest.mark.parametrize('name', CASE_IDS)
def test_per_element_against_float64(name, kind):
    c = CASES[name]
    g = torch.Generator().manual_seed(31)
    x, w, dy = (family(kind, s, g) for s in shapes(c))
    for which in ('fwd', 'dx', 'dw'):
        got, _, (ref, a, b) = run_product(c, which, x, w, dy)
        want, den = ref(a, b, c), ref(a.abs(), b.abs(), c)
        num = (got - want).abs()
        live = den > 0
        assert bool((num[~live] == 0).all())
        e = float((num[live] / den[live]).max())
        print(f'RATIO conv_{which}_x3 {name} {kind}: e={e:.3e} = {e / BOUND:.3f} of 2^-14')
        assert e <= BOUND, (name, kind, which, e)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['k3_12_36', 'k7_4_4', 'k3s2_4_36'])
def test_repeats_are_bit_equal(name):
    c = CASES[name]
    g = torch.Generator().manual_seed(41)
    x, w, dy = (family('gauss', s, g) for s in shapes(c))
    wpk, wpkt = dev_pack(w, 0), dev_pack(w, 1)
    a, b = run_fwd(c, x, wpk), run_fwd(c, x, wpk)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int16), b[1].view(torch.int16))
    a, b = run_dx(c, dy, wpkt), run_dx(c, dy, wpkt)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int16), b[1].view(torch.int16))
    assert torch.equal(run_dw(c, x, dy).view(torch.int32), run_dw(c, x, dy).view(torch.int32))


# ---------------------------------------------------------------------------- refusals
def bad_geometries():
    c = CASES['k3_8_36']
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
    src = operand(torch.zeros(1 << 16))
    wpk = operand(torch.zeros(1 << 16), BF16)
    out, out16, ws = Out((1 << 16,)), Out((1 << 16,), BF16), Out((1 << 18,))
    s, p, o, o16, w_ = src.data_ptr(), wpk.data_ptr(), out.ptr(), out16.ptr(), ws.ptr()
    for label, c in bad_geometries():
        ga = geo_args(c)
        assert dll.vitae_conv3d_fwd_x3(s, p, o, o16, *ga, st) in (-1, -2), label
        assert dll.vitae_conv3d_bwd_input_x3(s, p, o, o16, 0, *ga, st) in (-1, -2), label
        assert dll.vitae_conv3d_bwd_weight_x3(s, s, o, w_, 1 << 18, 0, *ga, st) in (-1, -2), label
    c = CASES['k3_8_36']
    ga = geo_args(c)
    need = dll.vitae_conv3d_wgrad_ws_floats(*ga)
    assert 0 < need <= 1 << 18
    assert dll.vitae_conv3d_bwd_weight_x3(s, s, o, w_, need - 1, 0, *ga, st) == -1                                   # workspace too small
    for args in ((None, p, o, o16), (s, None, o, o16), (s, p, None, None)):
        assert dll.vitae_conv3d_fwd_x3(*args, *ga, st) == -1
        assert dll.vitae_conv3d_bwd_input_x3(*args, 0, *ga, st) == -1
    assert dll.vitae_conv3d_bwd_input_x3(s, p, None, o16, 1, *ga, st) == -1                                          # accumulate needs dx
    for args in ((None, s, o, w_), (s, None, o, w_), (s, s, None, w_), (s, s, o, None)):
        assert dll.vitae_conv3d_bwd_weight_x3(*args, need, 0, *ga, st) == -1
    # misaligned operands: the vector gathers and the planes need 16 bytes
    for args in ((s + 4, p, o, o16), (s, p + 2, o, o16), (s, p + 8, o, o16), (s, p, o + 4, o16), (s, p, o, o16 + 2)):
        assert dll.vitae_conv3d_fwd_x3(*args, *ga, st) == -2
        assert dll.vitae_conv3d_bwd_input_x3(*args, 0, *ga, st) == -2
    for args in ((s + 4, s, o, w_), (s, s + 8, o, w_), (s, s, o + 4, w_), (s, s, o, w_ + 4)):
        assert dll.vitae_conv3d_bwd_weight_x3(*args, need, 0, *ga, st) == -2
    assert dll.vitae_conv3d_pack_weight_x3(None, o16, 8, 8, 3, 3, 3, 0, st) == -1
    assert dll.vitae_conv3d_pack_weight_x3(s, None, 8, 8, 3, 3, 3, 0, st) == -1
    assert dll.vitae_conv3d_pack_weight_x3(s, o16, 6, 8, 3, 3, 3, 0, st) == -2
    assert dll.vitae_conv3d_pack_weight_x3(s, o16, 8, 8, 3, 9, 3, 0, st) == -2
    assert dll.vitae_conv3d_pack_weight_x3(s, o16 + 2, 8, 8, 3, 3, 3, 0, st) == -2
    assert dll.vitae_to_channels_last_f32(None, o, 1, 1, 2, 2, 2, st) == -1
    assert dll.vitae_to_channels_last_f32(s, None, 1, 1, 2, 2, 2, st) == -1
    assert dll.vitae_to_channels_last_f32(s, o, 1, 0, 2, 2, 2, st) == -1
    # a table whose two-plane entry is misaligned or carries an unknown form
    for dest, form, rc in ((o16 + 8, 4, -2), (o16, 2, -1), (o16, 6, -1)):
        table = np.array([(s, dest, 8, 8, 3, 3, 3, form)], dtype=np.int64)
        chunks = np.zeros((1, 2), dtype=np.int32)
        td, cd = torch.from_numpy(table.copy()).cuda(), torch.from_numpy(chunks.copy()).cuda()
        assert dll.vitae_conv3d_pack_weights_multi(table.ctypes.data, td.data_ptr(), 1, chunks.ctypes.data, cd.data_ptr(), 1, st) == rc
    torch.cuda.synchronize()
    for t in (out, out16, ws):
        t.untouched()
