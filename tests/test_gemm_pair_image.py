"""The paired Linear-backward launch as ONE kernel image (csrc/gemm_ws64.hip: gemm_ws64_pair_kernel without template arguments).

The rows of either half's tile (64: tile 5, 128: tile 7) and the row sums are run-time properties of the launch, every body exists
once in the image, and a body carries only the epilogue instantiations of its operand form (csrc/gemm_bt.hpp, BT_KINDS_*): whatever
the set leaves out runs the generic kind 7.  Through the C ABI, with the tiles forced as tests/test_gemm_ws128x64.py forces them
(vitae_gemm_glds_set_bt_tile, VITAE_PAIR_TILES) and the input gradient's split forced with VITAE_BT_SPLIT (read per call under a
forced tile).

Shape: 130 token rows (padded to 192), a layer 128 -> 384.  130 rows end inside the last tile at both row counts (three 64-row
tiles, two 128-row tiles, the second with its upper fragment rows outside); the input gradient reduces over 384 = 6 k-tiles, so
splits 1 and 3 are both legal (two k-tiles per range); the weight gradient reduces over 192 = 3 k-tiles and is never split.

What pair_glds_call / gemm_call assert on EVERY launch below: the split-K tickets are zero again afterwards, the sentinels behind
the workspace and around every output (the rows in front of the first and behind the last row, the columns behind the width where a
leading dimension leaves a gap) are untouched.
"""
import pytest
import torch

from test_gemm_kernels import (BF16, CONSTS, bt_mode, lib, elem_err, epilogue_ref, exact_problem, family, gelu_checks, gelu_scale,  # noqa: F401
                               gemm_call, gemm_ref, ints, pad_rows, pair_glds_call, plain32, rne, strides, within)

pytestmark = pytest.mark.gpu
M, MPAD, N, K = 130, 192, 384, 128
TILES = ['55', '57', '75', '77']             # first digit: the input gradient's tile id, second: the weight gradient's
SPLITS = (1, 3)
DGELU, MASK = CONSTS['VITAE_EPI_DGELU'], CONSTS['VITAE_EPI_RELU_MASK']
A16, DV = CONSTS['VITAE_EPI_AUX_BF16'], CONSTS['VITAE_EPI_AUX_DERIV']


def operands(kind):
    """-> dy [M, N], w [N, K], x [M, K], old_dx [M, K], old_dw [N, K], h16 [M, K] (bf16-exact aux), ycs0 [N]"""
    if kind == 'ints':
        dy, w, x = ints((M, N), 4, 31), ints((N, K), 4, 32), ints((M, K), 4, 33)
    else:
        dy = rne(family('scales', M, 8, N, seed=N)[0])                     # rows of very different scales
        w, x = rne(family('plain', N, 8, K, seed=3)[0]), rne(family('plain', M, 8, K, seed=4)[0])
    return dy, w, x, ints((M, K), 8, 34), ints((N, K), 8, 35), ints((M, K), 24, 36) / 8, ints((N,), 8, 37)


def epilogue(name, old_dx, h16):
    """the input gradient's epilogue -> (keywords of gemm_call, keywords of pair_glds_call)"""
    if name == 'none':
        return {}, {}
    if name == 'accumulate':
        return dict(old=old_dx), dict(old_dx=old_dx)
    e = DGELU | A16 | (DV if name == 'dgelu16-saved' else 0)               # the step's form: aux holds GELU' / aux holds the pre-activation
    return dict(epi=e, aux=h16), dict(epi=e, aux=h16)


EPILOGUES = ['none', 'accumulate', 'dgelu16-saved', 'dgelu16']
_alone = {}


def force(bt_mode, monkeypatch, tile, split=0, pair_tiles=None):
    bt_mode(tile)
    monkeypatch.setenv('VITAE_BT_SPLIT', str(split))
    if pair_tiles:
        monkeypatch.setenv('VITAE_PAIR_TILES', pair_tiles)


def dgrad_alone(lib, bt_mode, monkeypatch, kind, tile, split, epi):
    """the input gradient as a launch of its own on the forced tile and split: computed once per key"""
    key = ('d', kind, tile, split, epi)
    if key not in _alone:
        dll = lib.load()
        dy, w, x, old_dx, old_dw, h16, ycs0 = operands(kind)
        force(bt_mode, monkeypatch, tile, split)
        assert dll.vitae_gemm_glds_bt_choice(1, 0, M, K, N) == tile and dll.vitae_gemm_glds_pick_split_k_form(1, 0, M, K, N) == split
        _alone[key] = gemm_call(lib, 'glds', dy, w.t().contiguous(), 'dgrad', c16=True, split=split, **epilogue(epi, old_dx, h16)[0])
    return _alone[key]


def wgrad_alone(lib, bt_mode, monkeypatch, kind, tile, accumulate):
    key = ('w', kind, tile, accumulate)
    if key not in _alone:
        dll = lib.load()
        dy, w, x, old_dx, old_dw, h16, ycs0 = operands(kind)
        force(bt_mode, monkeypatch, tile)
        assert dll.vitae_gemm_glds_bt_choice(0, 0, N, K, MPAD) == tile and dll.vitae_gemm_glds_pick_split_k_form(0, 0, N, K, MPAD) == 1
        _alone[key] = gemm_call(lib, 'glds', pad_rows(dy, MPAD).t().contiguous(), pad_rows(x, MPAD).t().contiguous(), 'wgrad', c16=True,
                                old=old_dw if accumulate else None)
    return _alone[key]


def pair(lib, bt_mode, monkeypatch, kind, tiles, split, epi, rowsums, accumulate):
    dy, w, x, old_dx, old_dw, h16, ycs0 = operands(kind)
    force(bt_mode, monkeypatch, 5 if tiles == '55' else 7, split, tiles)
    return pair_glds_call(lib, dy, w, x, MPAD, dx16=True, dw16=True, old_dw=old_dw if accumulate else None,
                          dycs0=ycs0 if rowsums else None, split=split, **epilogue(epi, old_dx, h16)[1])


@pytest.mark.parametrize('tiles', TILES)
def test_pair_equals_the_standalone_launches_bitwise(lib, bt_mode, monkeypatch, tiles):
    """every (rows of the input gradient, rows of the weight gradient) x row sums off / on x split 1 / 3 x epilogue x dW accumulate
    off / on: dx, dx16, dW, dW16 are bit for bit what the two stand-alone launches on the same tiles give.  The row sums (the bias
    gradient: unordered float atomics) against float64 with the GEMM tests' bound — they are a product with a vector of ones."""
    t1, t2 = int(tiles[0]), int(tiles[1])
    dy, ycs0 = operands('rounded')[0], operands('rounded')[6]
    ones = torch.ones(1, M)
    c64, den = gemm_ref(dy.t(), ones, bias=None, old=ycs0[:, None])
    e32 = [elem_err(p, c64, den) for p in plain32(dy.t(), ones, old=ycs0[:, None])]
    for split in SPLITS:
        for epi in EPILOGUES:
            dx = dgrad_alone(lib, bt_mode, monkeypatch, 'rounded', t1, split, epi)
            for accumulate in (False, True):
                dw = wgrad_alone(lib, bt_mode, monkeypatch, 'rounded', t2, accumulate)
                for rowsums in (False, True):
                    o = pair(lib, bt_mode, monkeypatch, 'rounded', tiles, split, epi, rowsums, accumulate)
                    what = (tiles, split, epi, accumulate, rowsums)
                    assert torch.equal(o.dx, dx.C) and torch.equal(o.dx16, dx.C16), what
                    assert torch.equal(o.dw, dw.C) and torch.equal(o.dw16, dw.C16), what
                    if rowsums:
                        within(f'pair image {what} row sums', elem_err(o.dycs.view(-1, 1), c64, den), *e32)


@pytest.mark.parametrize('tiles', TILES)
def test_pair_exact_on_integers(lib, bt_mode, monkeypatch, tiles):
    """operands of |v| <= 4 (every partial sum is an integer below 2^24): dx, dW and the row sums are the int64 products for every
    combination — the saved-derivative GELU' is a product with an eighth of an integer, exact as well — and three launches at
    split 3 are bitwise equal"""
    dy, w, x, old_dx, old_dw, h16, ycs0 = operands('ints')
    dxw, dww = (dy.double() @ w.double()), (dy.double().t() @ x.double())
    assert float(dxw.abs().max()) * 3 + 8 < 2 ** 24 and float(dww.abs().max()) + 8 < 2 ** 24
    want_dx = {'none': dxw, 'accumulate': dxw + old_dx.double(), 'dgelu16-saved': dxw * h16.double()}
    for split in SPLITS:
        for epi in ('none', 'accumulate', 'dgelu16-saved'):
            for accumulate in (False, True):
                for rowsums in (False, True):
                    o = pair(lib, bt_mode, monkeypatch, 'ints', tiles, split, epi, rowsums, accumulate)
                    what = (tiles, split, epi, accumulate, rowsums)
                    assert torch.equal(o.dx, want_dx[epi].float()) and torch.equal(o.dx16, o.dx.to(BF16)), what
                    assert torch.equal(o.dw, (dww + old_dw.double()).float() if accumulate else dww.float()), what
                    assert torch.equal(o.dw16, o.dw.to(BF16)), what
                    if rowsums:
                        assert torch.equal(o.dycs.view(-1), (ycs0.double() + dy.double().sum(0)).float()), what
    runs = [pair(lib, bt_mode, monkeypatch, 'rounded', tiles, 3, 'dgelu16', True, True) for _ in range(3)]
    for r in runs[1:]:
        assert all(torch.equal(getattr(r, k), getattr(runs[0], k)) for k in ('dx', 'dx16', 'dw', 'dw16'))


@pytest.mark.parametrize('tiles', ['55', '77'])
@pytest.mark.parametrize('aux16', [False, True])
def test_pair_epilogue_outside_the_set_runs_the_generic_kind(lib, bt_mode, monkeypatch, tiles, aux16):
    """the ReLU mask (kind 5) is in no body's set of the pair image: through vitae_linear_bwd_pair_glds it runs kind 7 at either
    row count and aux type, unsplit and split, and gives the exact masked product; the weight gradient beside it is untouched by it"""
    dy, w, x, old_dx, old_dw, h16, ycs0 = operands('ints')
    dxw, dww = (dy.double() @ w.double()).float(), (dy.double().t() @ x.double()).float()
    mask = ints((M, K), 2, 38)
    for split in SPLITS:
        force(bt_mode, monkeypatch, 5 if tiles == '55' else 7, split, tiles)
        o = pair_glds_call(lib, dy, w, x, MPAD, dx16=True, epi=MASK | (A16 if aux16 else 0), aux=mask, dycs0=ycs0, split=split)
        assert torch.equal(o.dx, torch.where(mask > 0, dxw, torch.zeros(()))) and torch.equal(o.dx16, o.dx.to(BF16))
        assert torch.equal(o.dw, dww) and torch.equal(o.dycs.view(-1), (ycs0.double() + dy.double().sum(0)).float())
    # GELU' from an fp32 aux and the fp32 saved derivative are IN the set (a caller without bf16 activations): the same bounds
    s = gelu_scale(N)
    force(bt_mode, monkeypatch, 5 if tiles == '55' else 7, 1, tiles)
    d = pair_glds_call(lib, dy, w * s, x, MPAD, epi=DGELU, aux=h16, dx16=True)
    gelu_checks(f'pair image {tiles} dgelu', h16, dgelu=d.dx, acc=(dxw.double() * s).float())
    assert torch.equal(d.dx16, d.dx.to(BF16)) and torch.equal(d.dw, dww)


@pytest.mark.parametrize('tile', [5, 7])
def test_standalone_epilogues_outside_the_form_sets(lib, bt_mode, monkeypatch, tile):
    """the stand-alone kernels carry the set of their operand form; a launch outside it — GELU' and the ReLU mask in the forward
    form, a residual, the ReLU mask and GELU in the input-gradient form, a residual in the weight-gradient form — runs kind 7: the
    values and bounds of test_gemm_kernels.test_epilogues_on_exact_preactivations, ragged 130 x 68 / 72 tiles, leading dimensions
    with gaps (the columns behind the width stay sentinels)"""
    GELU = CONSTS['VITAE_EPI_GELU']
    Kr = 128
    force(bt_mode, monkeypatch, tile)
    call = lambda *a, **kw: gemm_call(lib, 'glds', *a, **kw)
    # forward form, 130 x 68
    Mf, Nf = 130, 68
    assert lib.load().vitae_gemm_glds_bt_choice(1, 1, Mf, Nf, Kr) == tile
    a, b, bias, res, old, prod = exact_problem(Mf, Nf, Kr, 91)
    s = gelu_scale(Kr)
    acc = (prod * s).float()
    h = ints((Mf, Nf), 24, 92) / 8
    ld = strides('fwd', Mf, Nf, Kr, 8)
    gelu_checks(f'tile {tile} fwd dgelu', h, dgelu=call(a, b * s, epi=DGELU, aux=h, ld=ld).C, acc=acc)
    gelu_checks(f'tile {tile} fwd dgelu aux16', h, dgelu=call(a, b * s, epi=DGELU | A16, aux=h, c16=True, ld=ld).C, acc=acc)
    assert torch.equal(call(a, b * s, epi=DGELU | DV, aux=h, ld=ld).C, (acc.double() * h.double()).float())
    assert torch.equal(call(a, b * s, epi=MASK, aux=h, ld=ld).C, torch.where(h > 0, acc, torch.zeros(())))
    assert torch.equal(call(a, b * s, epi=MASK | A16, aux=h, ld=ld).C, torch.where(h > 0, acc, torch.zeros(())))
    # input-gradient form, 130 x 72
    Md, Nd = 130, 72
    assert lib.load().vitae_gemm_glds_bt_choice(1, 0, Md, Nd, Kr) == tile
    a, b, bias, res, old, prod = exact_problem(Md, Nd, Kr, 93)
    acc = (prod * s).float()
    h = ints((Md, Nd), 24, 94) / 8
    ld = strides('dgrad', Md, Nd, Kr, 8)
    assert torch.equal(call(a, b, 'dgrad', bias=bias, res=res, ld=ld).C, epilogue_ref(prod, bias, res).float())
    assert torch.equal(call(a, b * s, 'dgrad', epi=MASK | A16, aux=h, c16=True, ld=ld).C, torch.where(h > 0, acc, torch.zeros(())))
    pre = (prod * s + (bias / 8).double()).float()
    g = call(a, b * s, 'dgrad', bias=bias / 8, epi=GELU, ld=ld)
    assert torch.equal(g.aux, pre)
    gelu_checks(f'tile {tile} dgrad gelu', pre, y=g.C)
    # weight-gradient form, 136 x 72
    Mw, Nw = 136, 72
    assert lib.load().vitae_gemm_glds_bt_choice(0, 0, Mw, Nw, Kr) == tile
    a, b, bias, res, old, prod = exact_problem(Mw, Nw, Kr, 95)
    assert torch.equal(call(a, b, 'wgrad', res=res, ld=strides('wgrad', Mw, Nw, Kr, 8)).C, epilogue_ref(prod, None, res).float())
