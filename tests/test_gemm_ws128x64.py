"""The wave-specialised 128 x 64 tile (id 7, csrc/gemm_ws64.hip: gemm_ws64_body with BM = 128) through the C ABI with the tile
forced (vitae_gemm_glds_set_bt_tile(7); the bt_mode fixture restores the planner), stand-alone and inside the paired launch.

Shapes.  The library admits a row-contiguous operand only with a multiple of 8 rows (16-byte DMA chunks), and the paired backward
only with an output width that is a multiple of 64 (it is the input gradient's reduction).  So the ragged case M = 130, N = 68
runs as it stands in the forward form, as 130 x 72 in the input-gradient form (B row-contiguous) and as 136 x 72 in the
weight-gradient form (both row-contiguous): every one of them still ends inside the second fragment of a wave and inside a column
tile.  The pair runs rows = 130 (padded to 192) on widths 192 x 72 and 128 x 192; the row sums run through the pair on 192 output
features (rows of both fragments, and a second row tile whose upper half lies outside the matrix).

Accumulation order.  The tile keeps ONE accumulator per fragment (its two fragments are the two independent MFMA chains): the even /
odd pair per fragment of the 64 x 64 tile does not fit the 128 registers of two workgroups per CU next to the row-sum accumulator.
An output element is therefore summed in k order, not even-slices-then-odd: against tile 5 the test asserts the float64 bound of
tests/test_gemm_kernels.py, not bit equality.
"""
import pytest
import torch

from test_gemm_kernels import (BF16, F64, FORMS, GUARD, SENT, bt_mode, C, lib, exact_problem, epilogue_ref, gemm_call, gelu_checks,  # noqa: F401
                               gelu_scale, glds_exact, ints, pair_glds_call, pad_rows, rne, rounding_case, family, strides)

gpu = pytest.mark.gpu
pytestmark = gpu
TILE = 7
# the ragged shape per operand form (module docstring)
RAGGED = {'fwd': (130, 68), 'dgrad': (130, 72), 'wgrad': (136, 72)}


def on_tile(lib, bt_mode, form, M, N, K):
    bt_mode(TILE)
    akc, bkc = FORMS[form]
    assert lib.load().vitae_gemm_glds_bt_choice(akc, bkc, M, N, K) == TILE


@pytest.mark.parametrize('form', ['fwd', 'dgrad', 'wgrad'])
@pytest.mark.parametrize('case', ['ragged', 'second-fragment-outside', 'seven-k-tiles'])
def test_exact_on_integers(lib, bt_mode, form, case):
    """ragged tails in both dimensions at the minimum of two k-tiles; M = 64: the second fragment of every wave entirely outside
    the matrix; K = 448: seven k-tiles on three stages, the ring wraps with an odd count.  Plain, bf16 copy, bias + residual +
    accumulate (the generic epilogue 7) and out_colsum: the integer answer, bit for bit."""
    M, N, K = {'ragged': RAGGED[form] + (128,), 'second-fragment-outside': (64, 64, 128), 'seven-k-tiles': (128, 64, 448)}[case]
    on_tile(lib, bt_mode, form, M, N, K)
    glds_exact(lib, form, M, N, K, (1,), seed=7 + K)
    if case == 'ragged':
        glds_exact(lib, form, M, N, K, (1,), seed=8 + K, ld=strides(form, M, N, K, 8))


@pytest.mark.parametrize('form', ['fwd', 'dgrad', 'wgrad'])
@pytest.mark.parametrize('split', [2, 4])
def test_split_k_exact_and_reproducible(lib, bt_mode, form, split):
    """M = 256, N = 128, K = 512 at forced splits 2 and 4: the integer answer, three launches bitwise equal.  Every launch gets a
    fresh workspace whose tickets gemm_call requires to be zero again afterwards: a ticket left behind fails there."""
    M, N, K = 256, 128, 512
    on_tile(lib, bt_mode, form, M, N, K)
    a, b, bias, res, old, prod = glds_exact(lib, form, M, N, K, (split,), seed=70 + split)
    fa, fb = (rne(t) for t in family('scales', M, N, K, seed=split)[:2])
    outs = [gemm_call(lib, 'glds', fa, fb, form, split=split).C for _ in range(3)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert torch.equal(gemm_call(lib, 'glds', a, b, form, split=split).C, prod.float())


def test_every_epilogue_kind(lib, C, bt_mode):
    """kinds 0 - 6 and the generic 7 at M = 130, N = 68, K = 128 (forward form), aux as fp32 and as bf16, with and without the bf16
    copy, out_colsum; against the float64 values with the bounds of test_gemm_kernels.test_epilogues_on_exact_preactivations"""
    GELU, DGELU, MASK, RELU = C['VITAE_EPI_GELU'], C['VITAE_EPI_DGELU'], C['VITAE_EPI_RELU_MASK'], C['VITAE_EPI_RELU']
    A16, DV = C['VITAE_EPI_AUX_BF16'], C['VITAE_EPI_AUX_DERIV']
    M, N, K = 130, 68, 128
    on_tile(lib, bt_mode, 'fwd', M, N, K)
    a, b, bias, res, old, prod = exact_problem(M, N, K, 81)
    call = lambda *args, **kw: gemm_call(lib, 'glds', *args, **kw)
    # 0 plain (bias), 1 + residual, 2 + old C, 7 residual + old C; the bf16 copy beside C and alone; column sums of the stored result
    assert torch.equal(call(a, b, bias=bias).C, epilogue_ref(prod, bias).float())
    assert torch.equal(call(a, b, bias=bias, res=res).C, epilogue_ref(prod, bias, res).float())
    assert torch.equal(call(a, b, old=old).C, epilogue_ref(prod, None, None, old).float())
    cs0 = ints((N,), 8, 88)
    full = epilogue_ref(prod, bias, res, old)
    o = call(a, b, bias=bias, res=res, old=old, colsum=cs0, c16=True)
    assert torch.equal(o.C, full.float()) and torch.equal(o.C16, o.C.to(BF16))
    assert torch.equal(o.colsum.view(-1), (cs0.double() + full.sum(0)).float())
    assert torch.equal(call(a, b, bias=bias, res=res, c32=False, c16=True).C16, epilogue_ref(prod, bias, res).float().to(BF16))
    # 3 GELU, 4 GELU', 5 ReLU mask, 6 ReLU on exact pre-activations
    s = gelu_scale(K)
    bs, biass = b * s, bias / 8
    pre = (prod * s + biass.double()).float()
    acc = (prod * s).float()
    ld = strides('fwd', M, N, K, 8)
    lab = f'tile 7 {M}x{N}x{K}'
    g = call(a, bs, bias=biass, epi=GELU, ld=ld)
    assert torch.equal(g.aux, pre), 'the saved pre-activation is the exact value'
    gelu_checks(lab, pre, y=g.C)
    gd = call(a, bs, bias=biass, epi=GELU | DV)
    assert torch.equal(gd.C, g.C)
    gelu_checks(lab + ' saved', pre, dsaved=gd.aux)
    g16 = call(a, bs, bias=biass, epi=GELU | A16, c16=True, ld=ld)
    assert torch.equal(g16.aux, pre.to(BF16)) and torch.equal(g16.C16, g16.C.to(BF16)) and torch.equal(g16.C, g.C)
    only16 = call(a, bs, bias=biass, epi=GELU | A16, c32=False, c16=True)
    assert torch.equal(only16.aux, g16.aux) and torch.equal(only16.C16, g16.C16)
    h = ints((M, N), 24, 82) / 8
    h16 = rne(h)
    gelu_checks(lab, h, dgelu=call(a, bs, epi=DGELU, aux=h, ld=ld).C, acc=acc)
    gelu_checks(lab + ' aux16', h16, dgelu=call(a, bs, epi=DGELU | A16, aux=h16, c16=True).C, acc=acc)
    assert torch.equal(call(a, bs, epi=DGELU | DV, aux=h).C, (acc.double() * h.double()).float())
    masked = torch.where(h > 0, acc, torch.zeros(()))
    assert torch.equal(call(a, bs, epi=MASK, aux=h).C, masked)
    m16 = call(a, bs, epi=MASK | A16, aux=h16, c16=True)
    assert torch.equal(m16.C, torch.where(h16 > 0, acc, torch.zeros(()))) and torch.equal(m16.C16, m16.C.to(BF16))
    assert torch.equal(call(a, bs, epi=MASK, aux=h, res=res).C, (masked.double() + res).float())       # (generic: an activation + residual)
    r = call(a, bs, bias=biass, epi=RELU, c16=True)
    assert torch.equal(r.C, pre.clamp_min(0)) and torch.equal(r.C16, r.C.to(BF16))


def test_sqacc_share_exact(lib, bt_mode):
    """the gradient norm's share of a weight-gradient launch (one atomic per workgroup): sum(dw_stored^2) exactly, through the single
    slot and the spread slots, without and with accumulate"""
    dll = lib.load()
    M, N, K = 136, 72, 128
    on_tile(lib, bt_mode, 'wgrad', M, N, K)
    a, b, old = ints((M, K), 1, 140), ints((N, K), 1, 141), ints((M, N), 8, 142)
    prod = a.double() @ b.double().t()
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
        assert float(slots.sum()) == want and bool((sq[n_slots * stride:] == SENT).all())


def standalone_halves(lib, bt_mode, dy, w, x, Mpad, t1, t2):
    """the two halves of a Linear's backward as launches of their own on tiles t1 / t2"""
    bt_mode(t1)
    dx = gemm_call(lib, 'glds', dy, w.t().contiguous(), 'dgrad', c16=True)
    bt_mode(t2)
    dw = gemm_call(lib, 'glds', pad_rows(dy, Mpad).t().contiguous(), pad_rows(x, Mpad).t().contiguous(), 'wgrad', c16=True)
    return dx, dw


@pytest.mark.parametrize('N,K', [(192, 72), (128, 192)])
@pytest.mark.parametrize('tiles', ['55', '57', '75', '77'])
def test_pair_equals_the_standalone_launches(lib, bt_mode, monkeypatch, N, K, tiles):
    """one Linear's backward at 130 token rows (padded to 192), every combination of row counts for the two halves (first digit: the
    input gradient's tile, second: the weight gradient's): bitwise what the two stand-alone launches give on rounded random
    operands, without and with the row sums (the bias gradient: another kernel instantiation), and the integer answer"""
    dll = lib.load()
    M, Mpad = 130, 192
    t1, t2 = int(tiles[0]), int(tiles[1])
    monkeypatch.setenv('VITAE_PAIR_TILES', tiles)
    dy = rne(family('scales', M, 8, N, seed=N)[0])                         # [M, N], rows of very different scales
    w, x = rne(family('plain', N, 8, K, seed=3)[0]), rne(family('plain', M, 8, K, seed=4)[0])
    assert dy.shape == (M, N) and w.shape == (N, K) and x.shape == (M, K)
    dx, dw = standalone_halves(lib, bt_mode, dy, w, x, Mpad, t1, t2)
    bt_mode(5 if tiles == '55' else TILE)
    assert dll.vitae_gemm_glds_bt_choice(1, 0, M, K, N) in (5, TILE)
    for rowsums in (False, True):
        o = pair_glds_call(lib, dy, w, x, Mpad, dx16=True, dw16=True, dycs0=torch.zeros(N) if rowsums else None)
        assert torch.equal(o.dx, dx.C) and torch.equal(o.dx16, dx.C16), (tiles, rowsums)
        assert torch.equal(o.dw, dw.C) and torch.equal(o.dw16, dw.C16), (tiles, rowsums)
    # integers: exact, row sums included
    dyi, wi, xi = ints((M, N), 4, 11), ints((N, K), 4, 12), ints((M, K), 4, 13)
    ycs0, cs0 = ints((N,), 8, 14), ints((K,), 8, 15)
    dxw, dww = dyi.double() @ wi.double(), dyi.double().t() @ xi.double()
    oi = pair_glds_call(lib, dyi, wi, xi, Mpad, dxcs0=cs0, dycs0=ycs0)
    assert torch.equal(oi.dx, dxw.float()) and torch.equal(oi.dw, dww.float())
    assert torch.equal(oi.dxcs.view(-1), (cs0.double() + dxw.sum(0)).float())
    assert torch.equal(oi.dycs.view(-1), (ycs0.double() + dyi.double().sum(0)).float())


def test_row_sums_of_both_fragments(lib, bt_mode):
    """RS: the weight-gradient half with row sums of A = dy^T on 192 output features — rows of the first and of the second fragment
    of every wave, and a second row tile whose upper 64 rows lie outside; integer operands whose sums differ from row to row"""
    M, Mpad, N, K = 130, 192, 192, 72
    bt_mode(TILE)
    dy = ints((M, N), 4, 21) + (torch.arange(N) % 7).float()[None, :]      # a different sum for every output feature
    w, x = ints((N, K), 4, 22), ints((M, K), 4, 23)
    ycs0 = ints((N,), 8, 24)
    o = pair_glds_call(lib, dy, w, x, Mpad, dycs0=ycs0)
    assert torch.equal(o.dycs.view(-1), (ycs0.double() + dy.double().sum(0)).float())
    assert torch.equal(o.dw, (dy.double().t() @ x.double()).float())


@pytest.mark.parametrize('form', ['fwd', 'dgrad', 'wgrad'])
@pytest.mark.parametrize('split', [1, 2])
def test_rounding_within_the_float64_bound(lib, bt_mode, form, split):
    """M = 192, N = 128, K = 256 on rounded random operands: not bit equality with tile 5 (one accumulator per fragment, module
    docstring) but the per-element float64 bound that tile 5 is held to in test_gemm_kernels.test_gemm_glds_rounding"""
    M, N, K = 192, 128, 256
    on_tile(lib, bt_mode, form, M, N, K)
    for fam in ('plain', 'scales', 'cancel'):
        rounding_case(lib, 'glds', {}, 'bf16', fam, form, M, N, K, split=split, pre16=True, label=f'glds/t7/{form}/{fam}/s{split}')
