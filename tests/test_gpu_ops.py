"""GPU parity, kernel by kernel: each C-ABI launcher of libvitae_hip.so against the plain fp32
PyTorch (CPU) statement of the same op / the oracle function that restates the reference.
Tolerances: fp32-MFMA path ~1e-5 relative (accumulation order), bf16-MFMA path ~1e-2 of the output
scale (operands rounded to 8 mantissa bits)."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import mae_ref as R   # the checker


@pytest.fixture(scope='module')
def lib():
    from vit_ae_plus_plus_amd._abi import lib as L
    L.load()
    return L


@pytest.fixture(scope='module')
def C():
    from vit_ae_plus_plus_amd._abi import CONSTS
    return CONSTS


_KEEP = []


def dev(t):
    """Device copy that stays alive until the end of the test (launches are asynchronous: a temporary
    passed as ``dev(x).data_ptr()`` must not be recycled by the caching allocator before the kernel ran)."""
    d = t.detach().clone().contiguous().cuda()
    _KEEP.append(d)
    return d


@pytest.fixture(autouse=True)
def _release_device_copies():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def st():
    return torch.cuda.current_stream().cuda_stream


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def gen(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


# --------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize('prec,tol', [(0, 2e-5), (1, 2e-2), (2, 2e-5)])   # 2 = VITAE_PREC_BF16X3: split operands, fp32-grade
@pytest.mark.parametrize('M,N,K', [(440, 2304, 768), (37, 48, 128), (868, 512, 2048), (64, 64, 32), (130, 72, 4096)])
def test_linear_fwd_bwd(lib, C, prec, tol, M, N, K):
    x, w, b = gen(M, K, seed=1), gen(N, K, seed=2, scale=K ** -0.5), gen(N, seed=3)
    res = gen(M, N, seed=4)
    xd, wd, bd, rd = dev(x), dev(w), dev(b), dev(res)
    ws = torch.empty(1 << 22, device='cuda')
    # forward + bias + residual, with and without split-K
    for split in (1, lib.vitae_gemm_pick_split_k(M, N, K), 3):
        if split * M * N > ws.numel():
            continue
        y = torch.empty(M, N, device='cuda')
        lib.vitae_linear_fwd(prec, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), M, N, K, 0, None,
                             rd.data_ptr(), split, ws.data_ptr(), st())
        assert rel_err(y, F.linear(x, w, b) + res) < tol, f'split {split}'
    # GELU epilogue (aux = pre-activation)
    y, aux = torch.empty(M, N, device='cuda'), torch.empty(M, N, device='cuda')
    lib.vitae_linear_fwd(prec, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), M, N, K, C['VITAE_EPI_GELU'],
                         aux.data_ptr(), None, 1, None, st())
    pre = F.linear(x, w, b)
    assert rel_err(aux, pre) < tol and rel_err(y, F.gelu(pre)) < tol
    # dgrad with the GELU-derivative epilogue: dx = (dy @ W) * gelu'(h)
    dy = gen(M, N, seed=5)
    h = gen(M, K, seed=6)
    dyd, hd = dev(dy), dev(h)
    dx = torch.empty(M, K, device='cuda')
    split = lib.vitae_gemm_pick_split_k(M, K, N)
    lib.vitae_linear_bwd_input(prec, dyd.data_ptr(), wd.data_ptr(), dx.data_ptr(), M, N, K, C['VITAE_EPI_DGELU'],
                               hd.data_ptr(), 0, split, ws.data_ptr(), st())
    hh = h.clone().requires_grad_(True)
    F.gelu(hh).backward(dy @ w)
    assert rel_err(dx, hh.grad) < tol
    # VITAE_EPI_AUX_DERIV: the forward saves GELU'(pre-activation), the backward multiplies by it — bit for bit what evaluating
    # GELU' in the backward gives (same expression on the same fp32 value)
    DV = C['VITAE_EPI_AUX_DERIV']
    y2, auxg = torch.empty(M, N, device='cuda'), torch.empty(M, N, device='cuda')
    lib.vitae_linear_fwd(prec, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y2.data_ptr(), M, N, K, C['VITAE_EPI_GELU'] | DV,
                         auxg.data_ptr(), None, 1, None, st())
    pp = pre.clone().requires_grad_(True)
    F.gelu(pp).sum().backward()
    assert torch.equal(y2, y) and rel_err(auxg, pp.grad) < max(tol, 1e-5)
    hg = hh.detach().clone().requires_grad_(True)
    F.gelu(hg).sum().backward()
    gd = dev(hg.grad)
    dx3 = torch.empty(M, K, device='cuda')
    lib.vitae_linear_bwd_input(prec, dyd.data_ptr(), wd.data_ptr(), dx3.data_ptr(), M, N, K, C['VITAE_EPI_DGELU'] | DV,
                               gd.data_ptr(), 0, split, ws.data_ptr(), st())
    assert rel_err(dx3, hh.grad) < tol
    # dgrad accumulate
    base = gen(M, K, seed=7)
    dx2 = dev(base)
    lib.vitae_linear_bwd_input(prec, dyd.data_ptr(), wd.data_ptr(), dx2.data_ptr(), M, N, K, 0, None, 1, 1, None, st())
    assert rel_err(dx2, base + dy @ w) < tol
    # wgrad (+ accumulate) and bias grad
    dw = torch.empty(N, K, device='cuda')
    split = lib.vitae_gemm_pick_split_k(N, K, M)
    lib.vitae_linear_bwd_weight(prec, dyd.data_ptr(), xd.data_ptr(), dw.data_ptr(), M, N, K, 0, split, ws.data_ptr(), st())
    assert rel_err(dw, dy.t() @ x) < tol
    lib.vitae_linear_bwd_weight(prec, dyd.data_ptr(), xd.data_ptr(), dw.data_ptr(), M, N, K, 1, 1, None, st())
    assert rel_err(dw, 2 * (dy.t() @ x)) < tol
    db = torch.zeros(N, device='cuda')
    lib.vitae_colsum_accum(dyd.data_ptr(), N, db.data_ptr(), M, N, st())
    assert rel_err(db, dy.sum(0)) < 2e-5


@pytest.mark.parametrize('b16', [0, 1])
@pytest.mark.parametrize('M,N,K', [(440, 2304, 768), (37, 48, 128), (868, 512, 2048), (64, 64, 64), (130, 72, 4096),
                                   (432, 768, 16384), (868, 16384, 512)])
def test_gemm_bf16_pipeline(lib, C, b16, M, N, K):
    """vitae_gemm_bf16 in its three operand forms (fwd KC/KC, dgrad KC/row, wgrad row/row), fp32 or bf16 B."""
    tol = 2e-2
    x, w, b, res = gen(M, K, seed=1), gen(N, K, seed=2, scale=K ** -0.5), gen(N, seed=3), gen(M, N, seed=4)
    xd, wd, bd, rd = dev(x), dev(w), dev(b), dev(res)
    w16 = wd.to(torch.bfloat16); _KEEP.append(w16)
    wp = w16 if b16 else wd
    ws = torch.empty(1 << 24, device='cuda')
    for split in (1, lib.vitae_gemm_bf16_pick_split_k(M, N, K)):
        y = torch.full((M, N), float('nan'), device='cuda')
        lib.vitae_gemm_bf16(1, 1, xd.data_ptr(), K, wp.data_ptr(), K, b16, y.data_ptr(), N, M, N, K, bd.data_ptr(), rd.data_ptr(),
                            N, 0, None, 0, 0, split, ws.data_ptr(), None, st())
        assert rel_err(y, F.linear(x, w, b) + res) < tol, f'fwd split {split}'
    y, aux = torch.empty(M, N, device='cuda'), torch.empty(M, N, device='cuda')
    lib.vitae_gemm_bf16(1, 1, xd.data_ptr(), K, wp.data_ptr(), K, b16, y.data_ptr(), N, M, N, K, bd.data_ptr(), None, 0,
                        C['VITAE_EPI_GELU'], aux.data_ptr(), N, 0, 1, None, None, st())
    pre = F.linear(x, w, b)
    assert rel_err(aux, pre) < tol and rel_err(y, F.gelu(pre)) < tol
    dy = gen(M, N, seed=5)
    dyd = dev(dy)
    dx = torch.full((M, K), float('nan'), device='cuda')
    split = lib.vitae_gemm_bf16_pick_split_k(M, K, N)
    db = torch.zeros(N, device='cuda')
    lib.vitae_gemm_bf16(1, 0, dyd.data_ptr(), N, wp.data_ptr(), K, b16, dx.data_ptr(), K, M, K, N, None, None, 0, 0, None, 0, 0,
                        split, ws.data_ptr(), db.data_ptr(), st())
    assert rel_err(dx, dy @ w) < tol, 'dgrad'
    assert rel_err(db, dy.sum(0)) < 2e-5, 'bias gradient riding on the dgrad'
    if not b16:
        dw = torch.full((N, K), float('nan'), device='cuda')
        split = lib.vitae_gemm_bf16_pick_split_k(N, K, M)
        lib.vitae_gemm_bf16(0, 0, dyd.data_ptr(), N, xd.data_ptr(), K, 0, dw.data_ptr(), K, N, K, M, None, None, 0, 0, None, 0, 0,
                            split, ws.data_ptr(), None, st())
        assert rel_err(dw, dy.t() @ x) < tol, 'wgrad'
        lib.vitae_gemm_bf16(0, 0, dyd.data_ptr(), N, xd.data_ptr(), K, 0, dw.data_ptr(), K, N, K, M, None, None, 0, 0, None, 0, 1,
                            1, None, None, st())
        assert rel_err(dw, 2 * (dy.t() @ x)) < tol, 'wgrad accumulate'


@pytest.mark.parametrize('M,N,K', [(440, 2304, 768), (868, 512, 2048), (440, 768, 3072), (37, 48, 128), (868, 16384, 512)])
def test_linear_bwd_pair_bf16(lib, C, M, N, K):
    """dgrad + wgrad + bias grad of one Linear in a single launch."""
    x, w, dy, h = gen(M, K, seed=1), gen(N, K, seed=2, scale=K ** -0.5), gen(M, N, seed=5), gen(M, K, seed=6)
    xd, wd, dyd, hd_ = dev(x), dev(w), dev(dy), dev(h)
    w16 = wd.to(torch.bfloat16); _KEEP.append(w16)
    dx, dw, db = torch.full((M, K), float('nan'), device='cuda'), torch.full((N, K), float('nan'), device='cuda'), torch.zeros(N, device='cuda')
    lib.vitae_linear_bwd_pair_bf16(dyd.data_ptr(), w16.data_ptr(), xd.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(), M, N, K,
                                   C['VITAE_EPI_DGELU'], hd_.data_ptr(), 0, 0, st())
    hh = h.clone().requires_grad_(True)
    F.gelu(hh).backward(dy @ w)
    assert rel_err(dx, hh.grad) < 2e-2 and rel_err(dw, dy.t() @ x) < 2e-2 and rel_err(db, dy.sum(0)) < 2e-5
    lib.vitae_linear_bwd_pair_bf16(dyd.data_ptr(), w16.data_ptr(), xd.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(), M, N, K,
                                   0, None, 1, 1, st())
    assert rel_err(dx, hh.grad + dy @ w) < 2e-2 and rel_err(dw, 2 * (dy.t() @ x)) < 2e-2


@pytest.mark.parametrize('M,N,K', [(440, 2304, 768), (868, 512, 2048), (440, 768, 3072), (868, 16384, 512), (100, 64, 64)])
def test_linear_bwd_pair_glds(lib, C, M, N, K):
    """bf16-operand backward of one Linear (LDS-DMA kernels): dx, bf16 dx, colsum(dx), dW."""
    Mp = (M + 63) // 64 * 64
    x, w, dy, h = gen(M, K, seed=1), gen(N, K, seed=2, scale=K ** -0.5), gen(M, N, seed=5), gen(M, K, seed=6)
    x16 = torch.zeros(Mp, K, dtype=torch.bfloat16, device='cuda'); x16[:M] = x.cuda().to(torch.bfloat16)
    dy16 = torch.zeros(Mp, N, dtype=torch.bfloat16, device='cuda'); dy16[:M] = dy.cuda().to(torch.bfloat16)
    w16 = w.cuda().to(torch.bfloat16)
    hd_ = dev(h)
    dx, dx16 = torch.full((M, K), float('nan'), device='cuda'), torch.zeros(M, K, dtype=torch.bfloat16, device='cuda')
    dw, cs = torch.full((N, K), float('nan'), device='cuda'), torch.zeros(K, device='cuda')
    dw16 = torch.zeros(N, K, dtype=torch.bfloat16, device='cuda')
    dycs = torch.zeros(N, device='cuda')
    split = lib.vitae_linear_bwd_pair_pick_split_k(M, Mp, N, K)
    ws = torch.zeros(max(1, lib.vitae_gemm_glds_ws_floats(M, K, max(split, 3))), device='cuda')
    lib.vitae_linear_bwd_pair_glds(dy16.data_ptr(), w16.data_ptr(), x16.data_ptr(), dx.data_ptr(), dx16.data_ptr(), dw.data_ptr(), dw16.data_ptr(),
                                   M, Mp, N, K, C['VITAE_EPI_DGELU'], hd_.data_ptr(), cs.data_ptr(), dycs.data_ptr(), 0, 0, split, ws.data_ptr(), ws.numel(), st())
    dyr, wr, xr = dy16[:M].float().cpu(), w16.float().cpu(), x16[:M].float().cpu()
    hh = h.clone().requires_grad_(True)
    F.gelu(hh).backward(dyr @ wr)
    assert rel_err(dx, hh.grad) < 2e-3 and rel_err(dw, dyr.t() @ xr) < 2e-3
    assert torch.equal(dx16, dx.to(torch.bfloat16)) and rel_err(cs, dx.sum(0)) < 1e-4
    assert torch.equal(dw16, dw.to(torch.bfloat16))
    assert rel_err(dycs, dyr.sum(0)) < 1e-5                      # bias gradient from the wgrad workgroups
    assert int(ws[:C['VITAE_GLDS_TICKETS']].abs().sum()) == 0      # tickets handed back
    # forced 3-way split of the dgrad reduction: same numbers as the unsplit launch up to fp32 summation order
    lib.vitae_linear_bwd_pair_glds(dy16.data_ptr(), w16.data_ptr(), x16.data_ptr(), dx.data_ptr(), None, dw.data_ptr(), None,
                                   M, Mp, N, K, 0, None, None, None, 0, 1, 3 if N >= 192 else 1, ws.data_ptr(), ws.numel(), st())
    assert rel_err(dx, dyr @ wr) < 2e-3 and rel_err(dw, 2 * (dyr.t() @ xr)) < 2e-3
    d1 = dx.clone()
    lib.vitae_linear_bwd_pair_glds(dy16.data_ptr(), w16.data_ptr(), x16.data_ptr(), dx.data_ptr(), None, dw.data_ptr(), None,
                                   M, Mp, N, K, 0, None, None, None, 0, 0, 3 if N >= 192 else 1, ws.data_ptr(), ws.numel(), st())
    assert torch.equal(dx, d1)                                      # split order is fixed -> bitwise reproducible
    # dx_accumulate: dx += dy16 @ W16 (decoder_embed adds into the predictor's latent gradient)
    lib.vitae_linear_bwd_pair_glds(dy16.data_ptr(), w16.data_ptr(), x16.data_ptr(), dx.data_ptr(), None, dw.data_ptr(), None,
                                   M, Mp, N, K, 0, None, None, None, 1, 0, split, ws.data_ptr(), ws.numel(), st())
    assert rel_err(dx, 2 * (dyr @ wr)) < 2e-3 and rel_err(dw, dyr.t() @ xr) < 2e-3


@pytest.mark.parametrize('M,N,K', [(440, 2304, 768), (432, 768, 16384), (868, 16384, 512), (100, 72, 128)])
def test_gemm_glds_forward_forms(lib, C, M, N, K):
    x, w, b, res = gen(M, K, seed=1), gen(N, K, seed=2, scale=K ** -0.5), gen(N, seed=3), gen(M, N, seed=4)
    x16, w16 = x.cuda().to(torch.bfloat16), w.cuda().to(torch.bfloat16)
    bd, rd = dev(b), dev(res)
    ref = F.linear(x16.float().cpu(), w16.float().cpu(), b)
    for split in (1, lib.vitae_gemm_glds_pick_split_k(M, N, K), 2):
        ws = torch.zeros(max(1, lib.vitae_gemm_glds_ws_floats(M, N, split)), device='cuda')
        y, y16, cs = torch.full((M, N), float('nan'), device='cuda'), torch.zeros(M, N, dtype=torch.bfloat16, device='cuda'), torch.zeros(N, device='cuda')
        lib.vitae_gemm_glds(1, 1, x16.data_ptr(), K, w16.data_ptr(), K, y.data_ptr(), N, y16.data_ptr(), N, M, N, K, bd.data_ptr(),
                            rd.data_ptr(), N, 0, None, 0, 0, split, ws.data_ptr(), cs.data_ptr(), st())
        assert rel_err(y, ref + res) < 2e-3, f'split {split}'
        assert torch.equal(y16, y.to(torch.bfloat16)) and rel_err(cs, y.sum(0)) < 1e-4
    y16, aux = torch.zeros(M, N, dtype=torch.bfloat16, device='cuda'), torch.empty(M, N, device='cuda')
    lib.vitae_gemm_glds(1, 1, x16.data_ptr(), K, w16.data_ptr(), K, None, 0, y16.data_ptr(), N, M, N, K, bd.data_ptr(), None, 0,
                        C['VITAE_EPI_GELU'], aux.data_ptr(), N, 0, 1, None, None, st())
    assert rel_err(aux, ref) < 2e-3 and rel_err(y16.float(), F.gelu(ref)) < 1e-2


@pytest.mark.parametrize('M,N,K', [(440, 768, 3072), (3472, 2048, 512), (868, 16384, 512), (100, 72, 132)])
def test_gemm_bf16x3_error_against_float64(lib, C, M, N, K):
    """The split-operand mode (hi.hi + hi.lo + lo.hi on the bf16 MFMA) against the float64 product: its error sits with the
    exact-fp32 MFMA's (a few 1e-6 of the output scale), three orders under the one-term bf16 product — in all four operand layouts
    (the wide 64 x 128 tile at the large shapes)."""
    assert C['VITAE_PREC_BF16X3'] == 2
    a, b = gen(M, K, seed=11), gen(N, K, seed=12)
    ref = a.double() @ b.double().t()
    ws = torch.empty(1 << 22, device='cuda')
    errs = {}
    for prec in (0, 1, 2):
        c = torch.empty(M, N, device='cuda')
        lib.vitae_gemm(prec, 1, 1, dev(a).data_ptr(), K, dev(b).data_ptr(), K, c.data_ptr(), N, M, N, K, None, None, 0, 0, None, 0,
                       0, 1, ws.data_ptr(), st())
        errs[prec] = rel_err(c, ref)
    assert errs[2] < 1e-5 and errs[2] < errs[1] / 100 and errs[0] < 4e-6, errs   # observed 4.5e-6 / 2.7e-3 / 2.1e-6 at K = 3072
    at, bt = a.t().contiguous(), b.t().contiguous()
    for akc, bkc in ((1, 0), (0, 1), (0, 0)):
        c = torch.empty(M, N, device='cuda')
        lib.vitae_gemm(2, akc, bkc, dev(a if akc else at).data_ptr(), K if akc else M, dev(b if bkc else bt).data_ptr(),
                       K if bkc else N, c.data_ptr(), N, M, N, K, None, None, 0, 0, None, 0, 0, 1, ws.data_ptr(), st())
        assert rel_err(c, ref) < 1e-5, (akc, bkc)


@pytest.mark.parametrize('form', ['fwd', 'dgrad', 'wgrad'])
@pytest.mark.parametrize('M,N,K', [(440, 768, 3072), (868, 2048, 512), (300, 264, 196), (130, 72, 68), (2304, 768, 440)])
def test_gemm_wsx3(lib, C, form, M, N, K):
    """vitae_gemm_wsx3 (fp32 operands split into bf16 hi + lo by the producer waves of a wave-specialised workgroup): against the
    float64 product in every operand form — reduction lengths that are not multiples of 64 (zero-filled tail), ragged tiles,
    in-launch split-K (bitwise reproducible, tickets handed back), epilogues (bias + residual + column sums, exact-erf GELU with
    the saved pre-activation, GELU', accumulate) and the row sums of A beside a weight gradient."""
    akc, bkc = {'fwd': (1, 1), 'dgrad': (1, 0), 'wgrad': (0, 0)}[form]
    if form == 'wgrad':
        M = M // 4 * 4            # row-contiguous operands move in 16-byte groups of rows
    a, b = gen(M, K, seed=31), gen(N, K, seed=32, scale=K ** -0.5)
    ref = a.double() @ b.double().t()
    A = dev(a if akc else a.t().contiguous()); B = dev(b if bkc else b.t().contiguous())
    lda, ldb = (K if akc else M), (K if bkc else N)
    ws = torch.zeros(lib.vitae_gemm_glds_ws_floats(M, N, 8) + 64, device='cuda')

    def run(c, bias=None, res=None, epi=0, aux=None, acc=0, split=1, cs=None, rs=None):
        lib.vitae_gemm_wsx3(akc, bkc, A.data_ptr(), lda, B.data_ptr(), ldb, c.data_ptr(), N, M, N, K, None if bias is None else bias.data_ptr(),
                            None if res is None else res.data_ptr(), N, epi, None if aux is None else aux.data_ptr(), N, acc, split, ws.data_ptr(),
                            None if cs is None else cs.data_ptr(), None if rs is None else rs.data_ptr(), st())
    nan = lambda: torch.full((M, N), float('nan'), device='cuda')
    c = nan(); run(c)
    assert rel_err(c, ref) < 1e-5                                    # observed 2-5e-6: the fp32 MFMA's own class
    # split-K inside the launch: same values up to summation order, reproducible, tickets back to zero
    outs = []
    split = max(2, min(4, (K + 63) // 64 // 2))
    for _ in range(2):
        c2 = nan(); run(c2, split=split); outs.append(c2)
    assert rel_err(outs[0], ref) < 1e-5 and torch.equal(outs[0], outs[1])
    assert int(ws[:C['VITAE_GLDS_TICKETS']].abs().sum()) == 0
    # bias + residual + column sums; accumulate on top
    bias, res, old = gen(N, seed=33), gen(M, N, seed=34), gen(M, N, seed=35)
    cs = torch.zeros(N, device='cuda')
    c = nan(); run(c, bias=dev(bias), res=dev(res), cs=cs)
    want = ref + bias.double() + res.double()
    assert rel_err(c, want) < 1e-5 and rel_err(cs, c.sum(0)) < 1e-5
    c = dev(old); run(c, acc=1)
    assert rel_err(c, ref + old.double()) < 1e-5
    # GELU (exact erf) with the saved pre-activation, then GELU' of it
    pre = nan(); c = nan(); run(c, bias=dev(bias), epi=C['VITAE_EPI_GELU'], aux=pre)
    assert rel_err(pre, ref + bias.double()) < 1e-5 and rel_err(c, F.gelu((ref + bias.double()).float())) < 1e-5
    h = gen(M, N, seed=36)
    hh = h.clone().double().requires_grad_(True)
    F.gelu(hh).backward(ref)
    c = nan(); run(c, epi=C['VITAE_EPI_DGELU'], aux=dev(h))
    assert rel_err(c, hh.grad) < 1e-5
    # the same pair through the saved derivative (VITAE_EPI_AUX_DERIV)
    DV = C['VITAE_EPI_AUX_DERIV']
    pg = (ref + bias.double()).float().clone().requires_grad_(True)
    F.gelu(pg).sum().backward()
    der = nan(); c2 = nan(); run(c2, bias=dev(bias), epi=C['VITAE_EPI_GELU'] | DV, aux=der)
    assert rel_err(der, pg.grad) < 3e-5 and rel_err(c2, F.gelu((ref + bias.double()).float())) < 1e-5     # (GELU' of a 5e-6-accurate pre-activation: observed 1.4e-5)
    c = nan(); run(c, epi=C['VITAE_EPI_DGELU'] | DV, aux=dev(h))
    assert rel_err(c, ref * h.double()) < 1e-5
    if form == 'wgrad':
        rs = torch.zeros(M, device='cuda')
        c = nan(); run(c, rs=rs)
        assert rel_err(rs, a.double().sum(1)) < 1e-5


@pytest.mark.parametrize('M,N,ld', [(440, 2304, 2304), (868, 16384, 16384), (6944, 512, 512), (33, 48, 64), (130, 70, 70), (5, 4, 4)])
def test_colsum_accum(lib, M, N, ld):
    """Bias gradients of the fp32 schedules (out[n] += sum_m dy[m, n]): the 16-byte form and the scalar fallback (N % 4 != 0), a row
    stride wider than the row, accumulation into what is already there."""
    dy = gen(M, ld, seed=21)
    base = gen(N, seed=22)
    out = dev(base)
    lib.vitae_colsum_accum(dev(dy).data_ptr(), ld, out.data_ptr(), M, N, st())
    want = base.double() + dy[:, :N].double().sum(0)
    assert float((out.double().cpu() - want).abs().max()) < 2e-5 * max(1.0, float(want.abs().max()))


def test_gemm_bf16_asymmetric(lib):
    a = torch.eye(64)
    b = torch.arange(64 * 64, dtype=torch.float32).reshape(64, 64) / 128.0
    ad, bd = dev(a), dev(b)
    y = torch.empty(64, 64, device='cuda')
    lib.vitae_gemm_bf16(1, 1, ad.data_ptr(), 64, bd.data_ptr(), 64, 0, y.data_ptr(), 64, 64, 64, 64, None, None, 0, 0, None, 0, 0, 1,
                        None, None, st())
    assert rel_err(y, b.t()) < 5e-3
    lib.vitae_gemm_bf16(1, 0, ad.data_ptr(), 64, bd.data_ptr(), 64, 0, y.data_ptr(), 64, 64, 64, 64, None, None, 0, 0, None, 0, 0, 1,
                        None, None, st())
    assert rel_err(y, b) < 5e-3          # B read as (k, n): y = I @ b
    lib.vitae_gemm_bf16(0, 0, bd.data_ptr(), 64, ad.data_ptr(), 64, 0, y.data_ptr(), 64, 64, 64, 64, None, None, 0, 0, None, 0, 0, 1,
                        None, None, st())
    assert rel_err(y, b.t()) < 5e-3      # A read as (m, k) = b[k, m]: y = b^T @ I


def test_gemm_asymmetric_layout(lib):
    """A = I against an asymmetric B catches transposed C writes (cdna guide §3)."""
    M = N = K = 64
    a = torch.eye(64)
    b = torch.arange(64 * 64, dtype=torch.float32).reshape(64, 64) / 100.0
    y = torch.empty(M, N, device='cuda')
    ad, bd = dev(a), dev(b)
    for prec in (0, 1):
        lib.vitae_linear_fwd(prec, ad.data_ptr(), bd.data_ptr(), None, y.data_ptr(), M, N, K, 0, None, None, 1,
                             None, st())
        assert rel_err(y, b.t()) < (1e-6 if prec == 0 else 5e-3)


def test_gemm_rejects_bad_shapes(lib):
    from vit_ae_plus_plus_amd._abi import VitaeError
    x = torch.zeros(8, 6, device='cuda')
    with pytest.raises(VitaeError):
        lib.vitae_linear_fwd(0, x.data_ptr(), x.data_ptr(), None, x.data_ptr(), 8, 8, 6, 0, None, None, 1, None, st())


# --------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize('M,D', [(440, 768), (868, 512), (33, 48), (7, 1024)])
def test_layernorm(lib, M, D):
    x, w, b, dy = gen(M, D, seed=1, scale=2.0) + 0.3, gen(D, seed=2) + 1.0, gen(D, seed=3), gen(M, D, seed=4)
    xd, wd, bd, dyd = dev(x), dev(w), dev(b), dev(dy)
    y, mean, rstd = torch.empty(M, D, device='cuda'), torch.empty(M, device='cuda'), torch.empty(M, device='cuda')
    y16 = torch.empty(M, D, dtype=torch.bfloat16, device='cuda')
    lib.vitae_layernorm_fwd(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), y16.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                            M, D, 1e-6, st())
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = F.layer_norm(xr, (D,), wr, br, 1e-6)
    ref.backward(dy)
    assert rel_err(y, ref) < 1e-5
    assert torch.equal(y16, y.to(torch.bfloat16))
    base = gen(M, D, seed=5)
    for accum in (0, 1):
        dx = dev(base)
        dw, db = torch.zeros(D, device='cuda'), torch.zeros(D, device='cuda')
        dx16 = torch.empty(M, D, dtype=torch.bfloat16, device='cuda')
        cs = torch.zeros(D, device='cuda')
        lib.vitae_layernorm_bwd(dyd.data_ptr(), xd.data_ptr(), wd.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                dx.data_ptr(), dw.data_ptr(), db.data_ptr(), dx16.data_ptr(), cs.data_ptr(), M, D, accum, st())
        assert rel_err(dx, xr.grad + (base if accum else 0)) < 2e-5
        assert torch.equal(dx16, dx.to(torch.bfloat16)) and rel_err(cs, dx.sum(0)) < 2e-5
        assert rel_err(dw, wr.grad) < 2e-5 and rel_err(db, br.grad) < 2e-5


@pytest.mark.parametrize('M,D', [(440, 768), (868, 512), (3464, 768), (6916, 512), (9, 256), (4100, 1024)])
def test_layernorm_bwd_partial_records(lib, M, D):
    """The atomic-free LayerNorm backward: dx / dx16 as the atomic kernel, parameter gradients and colsum(dx) through partial
    records + vitae_ln_grad_reduce (two instances in one reduce launch, one of them without a column sum); += into the targets;
    bitwise reproducible."""
    x, w, dy = gen(M, D, seed=1, scale=2.0) + 0.3, gen(D, seed=2) + 1.0, gen(M, D, seed=4)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), torch.zeros(D, requires_grad=True)
    F.layer_norm(xr, (D,), wr, br, 1e-6).backward(dy)
    xd, wd, dyd = dev(x), dev(w), dev(dy)
    mean = xd.mean(1).contiguous()
    rstd = (xd.var(1, unbiased=False) + 1e-6).rsqrt().contiguous()
    G = lib.vitae_layernorm_bwd_part_records(M)
    assert 1 <= G <= max(1, (M + 7) // 8)
    base = gen(M, D, seed=5)
    outs = []
    for rep in range(2):
        dx, dx2 = dev(base), torch.empty(M, D, device='cuda')
        dx16 = torch.empty(M, D, dtype=torch.bfloat16, device='cuda')
        parts = [torch.full((G * 3 * D,), float('nan'), device='cuda') for _ in range(2)]
        lib.vitae_layernorm_bwd_part(dyd.data_ptr(), xd.data_ptr(), wd.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                                     parts[0].data_ptr(), dx16.data_ptr(), M, D, 1, st())
        lib.vitae_layernorm_bwd_part(dyd.data_ptr(), xd.data_ptr(), wd.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx2.data_ptr(),
                                     parts[1].data_ptr(), None, M, D, 0, st())
        dw, db, cs = (torch.ones(2, D, device='cuda') for _ in range(3))      # the reduce ADDS to what is there
        u64 = lambda v: np.array(v, dtype=np.uint64)
        a_p, a_w, a_b = u64([t.data_ptr() for t in parts]), u64([dw[0].data_ptr(), dw[1].data_ptr()]), u64([db[0].data_ptr(), db[1].data_ptr()])
        a_c = u64([cs[0].data_ptr(), 0])
        a_g, a_d = np.array([G, G], dtype=np.int32), np.array([D, D], dtype=np.int32)
        lib.vitae_ln_grad_reduce(2, a_p.ctypes.data, a_w.ctypes.data, a_b.ctypes.data, a_c.ctypes.data, a_g.ctypes.data, a_d.ctypes.data, st())
        torch.cuda.synchronize()
        outs.append((dx.clone(), dx2.clone(), dw.clone(), db.clone(), cs.clone()))
        assert rel_err(dx, xr.grad + base) < 2e-5 and rel_err(dx2, xr.grad) < 2e-5
        assert torch.equal(dx16, dx.to(torch.bfloat16))
        for i in range(2):
            assert rel_err(dw[i] - 1, wr.grad) < 2e-5 and rel_err(db[i] - 1, br.grad) < 2e-5
        assert rel_err(cs[0] - 1, dx.sum(0)) < 2e-5 and torch.equal(cs[1], torch.ones(D, device='cuda'))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------- attention
@pytest.mark.parametrize('B,N,H,hd', [(8, 55, 12, 64), (4, 217, 16, 32), (2, 17, 3, 16), (1, 130, 2, 64), (2, 70, 2, 128),
                                      (1, 433, 2, 64), (1, 1729, 2, 32)])       # patch-8 sequence lengths
def test_sdpa(lib, B, N, H, hd):
    D = H * hd
    qkv, do = gen(B, N, 3 * D, seed=1), gen(B, N, D, seed=2)
    qr = qkv.clone().requires_grad_(True)
    q, k, v = qr.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    att = ((q @ k.transpose(-2, -1)) * hd ** -0.5).softmax(-1)
    ref = (att @ v).transpose(1, 2).reshape(B, N, D)
    ref.backward(do)
    qd, dod = dev(qkv), dev(do)
    o, lse = torch.empty(B, N, D, device='cuda'), torch.empty(B * H * N, device='cuda')
    lib.vitae_sdpa_fwd(qd.data_ptr(), o.data_ptr(), lse.data_ptr(), B, N, H, hd, st())
    assert rel_err(o, ref) < 1e-5
    dqkv, delta = torch.zeros(B, N, 3 * D, device='cuda'), torch.empty(B * H * N, device='cuda')
    lib.vitae_sdpa_bwd(qd.data_ptr(), o.data_ptr(), dod.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), delta.data_ptr(),
                       B, N, H, hd, st())
    assert rel_err(dqkv, qr.grad) < 2e-5


@pytest.mark.parametrize('B,N,H,hd', [(8, 55, 12, 64), (4, 217, 16, 32), (2, 17, 3, 32), (1, 130, 2, 64), (1, 300, 1, 32),
                                      (2, 433, 12, 64), (1, 1729, 16, 32),      # patch 8 (config.ini:33): encoder / decoder sequences
                                      (1, 513, 2, 32), (1, 300, 2, 64)])   # the last two exceed the one-launch backward's LDS budget
def test_sdpa_mfma_bf16(lib, B, N, H, hd):
    D = H * hd
    qkv, do = gen(B, N, 3 * D, seed=1), gen(B, N, D, seed=2)
    qr = qkv.clone().requires_grad_(True)
    q, k, v = qr.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    att = ((q @ k.transpose(-2, -1)) * hd ** -0.5).softmax(-1)
    ref = (att @ v).transpose(1, 2).reshape(B, N, D)
    ref.backward(do)
    ref_lse = torch.logsumexp((q @ k.transpose(-2, -1)) * hd ** -0.5, -1).detach()   # [B,H,N]
    qd, dod = dev(qkv), dev(do)
    o, lse = torch.full((B, N, D), float('nan'), device='cuda'), torch.empty(B * H * N, device='cuda')
    o16 = torch.empty(B, N, D, dtype=torch.bfloat16, device='cuda')
    lib.vitae_sdpa_mfma_fwd(qd.data_ptr(), o.data_ptr(), o16.data_ptr(), lse.data_ptr(), B, N, H, hd, st())
    assert torch.equal(o16, o.to(torch.bfloat16))
    assert rel_err(o, ref) < 2e-2
    assert float((lse.cpu().reshape(B, H, N) - ref_lse).abs().max()) < 3e-2
    dqkv, delta = torch.full((B, N, 3 * D), float('nan'), device='cuda'), torch.empty(B * H * N, device='cuda')
    g16 = torch.empty(B, N, 3 * D, dtype=torch.bfloat16, device='cuda')
    cs = torch.zeros(3 * D, device='cuda')
    lib.vitae_sdpa_mfma_bwd(qd.data_ptr(), o.data_ptr(), dod.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), g16.data_ptr(),
                            cs.data_ptr(), delta.data_ptr(), B, N, H, hd, st())
    assert torch.equal(g16, dqkv.to(torch.bfloat16))
    assert rel_err(cs, dqkv.reshape(-1, 3 * D).sum(0)) < 1e-5
    g = qr.grad.reshape(B, N, 3, D)
    got = dqkv.cpu().reshape(B, N, 3, D)
    for i, name in enumerate('qkv'):
        assert rel_err(got[:, :, i], g[:, :, i]) < 3e-2, name


def test_sdpa_large_logits(lib):
    """Online-softmax rescale path: one key dominates from a late tile."""
    B, N, H, hd = 1, 100, 1, 32
    qkv = gen(B, N, 3 * hd, seed=3)
    qkv[0, 5, :hd] *= 30
    qkv[0, 77, hd:2 * hd] = qkv[0, 5, :hd] / 10
    q, k, v = qkv.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    ref = (((q @ k.transpose(-2, -1)) * hd ** -0.5).softmax(-1) @ v).transpose(1, 2).reshape(B, N, hd)
    o, lse = torch.empty(B, N, hd, device='cuda'), torch.empty(N, device='cuda')
    qd = dev(qkv)
    lib.vitae_sdpa_fwd(qd.data_ptr(), o.data_ptr(), lse.data_ptr(), B, N, H, hd, st())
    assert rel_err(o, ref) < 1e-5


# --------------------------------------------------------------------------- masking / assembly
@pytest.mark.parametrize('B,L,keep', [(8, 216, 54), (2, 64, 16), (2, 1728, 432), (3, 288, 72)])
def test_random_masking(lib, B, L, keep):
    noise = torch.rand(B, L, generator=torch.Generator().manual_seed(L))
    noise[0, 3] = noise[0, 9]   # a tie: stable order keeps index 3 first
    ids_keep, ids_restore, mask = R.masking_from_noise(noise, keep)
    sh = torch.empty(B, L, dtype=torch.int32, device='cuda')
    rs = torch.empty(B, L, dtype=torch.int32, device='cuda')
    rs64 = torch.empty(B, L, dtype=torch.int64, device='cuda')
    mk = torch.empty(B, L, device='cuda')
    lib.vitae_random_masking(dev(noise).data_ptr(), sh.data_ptr(), rs.data_ptr(), mk.data_ptr(), rs64.data_ptr(), B, L, keep,
                             st())
    assert torch.equal(rs64.cpu(), torch.argsort(torch.argsort(noise, dim=1, stable=True), dim=1))
    assert torch.equal(rs.cpu().long(), rs64.cpu())
    assert torch.equal(sh.cpu().long(), torch.argsort(noise, dim=1, stable=True))
    rank = torch.argsort(torch.argsort(noise, dim=1, stable=True), dim=1)
    assert torch.equal(mk.cpu(), (rank >= keep).float()) and float(mk.sum()) == B * (L - keep)
    if not (noise[0, 3] == noise[0, 9] and (rank[0, 3] < keep) != (rank[0, 9] < keep)):
        assert torch.equal(mk.cpu(), mask)   # the oracle's (reference's) mask


@pytest.mark.parametrize('C_,vol,p', [(4, (32, 32, 32), 16), (2, (16, 16, 16), 4), (1, (32, 16, 8), 8)])
def test_gather_patches_and_assemble(lib, C_, vol, p):
    B, D, Dd = 2, 48, 32
    cfg = R.RefConfig(volume_size=vol, patch_size=p, in_chans=C_, embed_dim=D, depth=1, num_heads=3,
                      decoder_embed_dim=Dd, decoder_depth=1, decoder_num_heads=2)
    L, P = cfg.num_patches, cfg.patch_dim
    keep = max(1, L // 4)
    x = gen(B, C_, *vol, seed=1)
    noise = torch.rand(B, L, generator=torch.Generator().manual_seed(2))
    ids_keep, ids_restore, mask = R.masking_from_noise(noise, keep)
    ids_shuffle = torch.argsort(noise, dim=1)
    sh = ids_shuffle.int().cuda()
    rows = torch.empty(B * keep, P, device='cuda')
    rows16 = torch.empty(B * keep, P, dtype=torch.bfloat16, device='cuda')
    lib.vitae_gather_patches(dev(x).data_ptr(), sh.data_ptr(), rows.data_ptr(), rows16.data_ptr(), B, C_, *vol, p, keep, st())
    assert torch.equal(rows16, rows.to(torch.bfloat16))
    # conv-order rows: unfold the volume the way Conv3d's weight is flattened
    g = cfg.grid
    pat = x.reshape(B, C_, g[0], p, g[1], p, g[2], p).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B, L, P)
    ref = torch.gather(pat, 1, ids_keep.unsqueeze(-1).expand(-1, -1, P)).reshape(B * keep, P)
    assert torch.equal(rows.cpu(), ref)
    # encoder assembly fwd/bwd
    tok, cls, pos = gen(B * keep, D, seed=3), gen(D, seed=4), gen(L + 1, D, seed=5)
    xs = torch.empty(B, keep + 1, D, device='cuda')
    lib.vitae_encoder_assemble_fwd(dev(tok).data_ptr(), dev(cls).data_ptr(), dev(pos).data_ptr(), sh.data_ptr(),
                                   xs.data_ptr(), B, L, keep, D, st())
    ref = torch.cat([(cls + pos[0]).expand(B, 1, D),
                     tok.reshape(B, keep, D) + pos[1:][ids_keep]], 1)
    assert torch.allclose(xs.cpu(), ref, atol=1e-6)
    dxs = gen(B, keep + 1, D, seed=6)
    dtok, dcls = torch.empty(B * keep, D, device='cuda'), torch.zeros(D, device='cuda')
    lib.vitae_encoder_assemble_bwd(dev(dxs).data_ptr(), dtok.data_ptr(), None, dcls.data_ptr(), B, keep, D, st())
    assert torch.equal(dtok.cpu(), dxs[:, 1:].reshape(B * keep, D))
    assert torch.allclose(dcls.cpu(), dxs[:, 0].sum(0), atol=1e-5)
    # decoder assembly fwd/bwd against the oracle's cat/gather formulation (vit_autoenc.py:184-190)
    e, mt, dpos = gen(B, keep + 1, Dd, seed=7), gen(Dd, seed=8), gen(L + 1, Dd, seed=9)
    er, mtr = e.clone().requires_grad_(True), mt.clone().requires_grad_(True)
    x_ = torch.cat([er[:, 1:], mtr.reshape(1, 1, Dd).repeat(B, L - keep, 1)], 1)
    x_ = torch.gather(x_, 1, ids_restore.unsqueeze(-1).repeat(1, 1, Dd))
    ref = torch.cat([er[:, :1], x_], 1) + dpos
    dxd = gen(B, L + 1, Dd, seed=10)
    ref.backward(dxd)
    xd = torch.empty(B, L + 1, Dd, device='cuda')
    rs = ids_restore.int().cuda()
    lib.vitae_decoder_assemble_fwd(dev(e).data_ptr(), dev(mt).data_ptr(), dev(dpos).data_ptr(), rs.data_ptr(), xd.data_ptr(),
                                   B, L, keep, Dd, st())
    assert torch.allclose(xd.cpu(), ref.detach(), atol=1e-6)
    de, dmt = torch.empty(B, keep + 1, Dd, device='cuda'), torch.zeros(Dd, device='cuda')
    de16 = torch.zeros(B, keep + 1, Dd, dtype=torch.bfloat16, device='cuda')
    lib.vitae_decoder_assemble_bwd(dev(dxd).data_ptr(), sh.data_ptr(), de.data_ptr(), de16.data_ptr(), dmt.data_ptr(), B, L, keep, Dd,
                                   st())
    assert torch.allclose(de.cpu(), er.grad, atol=1e-6) and torch.equal(de16, de.to(torch.bfloat16))
    assert rel_err(dmt, mtr.grad) < 1e-5


# --------------------------------------------------------------------------- loss chain
@pytest.mark.parametrize('C_,vol,p', [(4, (32, 32, 32), 16), (2, (16, 16, 16), 4), (1, (24, 16, 8), 8), (4, (48, 24, 40), 8),
                                      (1, (16, 48, 80), 16), (4, (16, 32, 96), 16), (4, (8, 40, 136), 8)])
def test_loss_chain(lib, C, C_, vol, p):
    from vit_ae_plus_plus_amd.engine import gaussian_taps_host
    B = 2
    cfg = R.RefConfig(volume_size=vol, patch_size=p, in_chans=C_, embed_dim=48, depth=1, num_heads=3,
                      decoder_embed_dim=32, decoder_depth=1, decoder_num_heads=2)
    L, P = cfg.num_patches, cfg.patch_dim
    V = vol[0] * vol[1] * vol[2]
    imgs = gen(B, C_, *vol, seed=1)
    predfull = gen(B, L + 1, P, seed=2, scale=0.5)
    mask = (torch.rand(B, L, generator=torch.Generator().manual_seed(3)) < 0.75).float()
    mask[:, 0] = 1
    edge_w, g_up = 0.37, 0.5
    pr = predfull.clone().requires_grad_(True)
    trace = {}
    losses = R.loss_terms(imgs, pr[:, 1:, :], mask, cfg, edge_w, trace=trace)
    (losses[0] * g_up).backward()
    hp = torch.zeros(C['VITAE_HP_COUNT'], device='cuda')
    hp[C['VITAE_HP_G_RECON']], hp[C['VITAE_HP_G_EDGE']], hp[C['VITAE_HP_EDGE_W']] = g_up, edge_w * g_up, edge_w
    acc = torch.zeros(C['VITAE_ACC_COUNT'], dtype=torch.float64, device='cuda')
    pd, im, mk = dev(predfull), dev(imgs), dev(mask)
    pp, pbs = pd.data_ptr() + P * 4, (L + 1) * P
    lib.vitae_recon_loss_fwd(pp, pbs, im.data_ptr(), mk.data_ptr(), acc.data_ptr(), B, C_, *vol, p, st())
    pv = torch.empty(B, C_, *vol, device='cuda')
    lib.vitae_unpatchify(pp, pbs, pv.data_ptr(), B, C_, *vol, p, st())
    assert torch.equal(pv.cpu(), R.unpatchify(predfull[:, 1:, :], p, cfg.grid))
    taps = gaussian_taps_host(2.0)
    tmp, bl = torch.empty_like(im), torch.empty_like(im)
    lib.vitae_gauss_blur_fwd(im.data_ptr(), tmp.data_ptr(), bl.data_ptr(), taps.ctypes.data, len(taps), B * C_, *vol, st())
    assert rel_err(bl, trace['blurred']) < 1e-5
    et, ep = torch.empty(B, *vol, device='cuda'), torch.empty(B, *vol, device='cuda')
    lib.vitae_sobel_edge_fwd(bl.data_ptr(), et.data_ptr(), None, None, B, C_, *vol, st())
    lib.vitae_sobel_edge_fwd(pv.data_ptr(), ep.data_ptr(), et.data_ptr(), acc.data_ptr(), B, C_, *vol, st())
    assert rel_err(et, trace['edge_target']) < 1e-5 and rel_err(ep, trace['edge_pred']) < 1e-5
    # blur + Sobel of the target in ONE launch (csrc/loss_fused.hip; 4 channels): what the training step's target branch runs
    if lib.vitae_target_edge_supported(C_, len(taps), *vol):
        et1 = torch.full((B, *vol), float('nan'), device='cuda')
        lib.vitae_target_edge(im.data_ptr(), et1.data_ptr(), taps.ctypes.data, len(taps), B, C_, *vol, st())
        assert rel_err(et1, trace['edge_target']) < 1e-5, rel_err(et1, trace['edge_target'])
    else:
        assert C_ != 4
    out = torch.zeros(4, device='cuda')
    msum = float(mask.sum())
    lib.vitae_loss_finalize(acc.data_ptr(), hp.data_ptr(), out.data_ptr(), msum, B * V, st())
    ref = torch.stack([l.detach() for l in losses])
    assert torch.allclose(out.cpu(), ref, rtol=2e-5, atol=1e-6), (out.cpu(), ref)
    dpred = torch.zeros(B, L + 1, P, device='cuda')
    dG = torch.empty(B * C_ * 3 * V, device='cuda')
    lib.vitae_recon_loss_bwd(pp, pbs, im.data_ptr(), mk.data_ptr(), hp.data_ptr(), dpred.data_ptr() + P * 4, msum, B, C_, *vol,
                             p, st())
    dpred16 = torch.zeros(B, L + 1, P, dtype=torch.bfloat16, device='cuda')
    lib.vitae_sobel_edge_bwd(pv.data_ptr(), ep.data_ptr(), et.data_ptr(), hp.data_ptr(), dG.data_ptr(), dpred.data_ptr() + P * 4,
                             dpred16.data_ptr() + P * 2, pbs, B, C_, *vol, p, st())
    assert float(dpred[:, 0].abs().max()) == 0.0
    assert rel_err(dpred, pr.grad) < 3e-5
    assert torch.equal(dpred16, dpred.to(torch.bfloat16))
    # the one-pass forward the training step uses: same volume, edge map and sums as the three kernels above
    acc2 = torch.zeros(C['VITAE_ACC_COUNT'], dtype=torch.float64, device='cuda')
    pv2, ep2 = torch.empty_like(pv), torch.empty_like(ep)
    lib.vitae_loss_fwd_fused(pp, pbs, im.data_ptr(), mk.data_ptr(), et.data_ptr(), pv2.data_ptr(), ep2.data_ptr(), acc2.data_ptr(),
                             B, C_, *vol, p, st())
    assert torch.equal(pv2, pv) and rel_err(ep2, trace['edge_pred']) < 1e-5
    assert torch.allclose(acc2[:2].cpu(), acc[:2].cpu(), rtol=1e-5)
    # the one-pass backward (recon + edge) the training step uses
    dfu = torch.zeros(B, L + 1, P, device='cuda')
    dfu16 = torch.zeros(B, L + 1, P, dtype=torch.bfloat16, device='cuda')
    lib.vitae_loss_bwd_fused(pp, pv.data_ptr(), im.data_ptr(), mk.data_ptr(), ep.data_ptr(), et.data_ptr(), hp.data_ptr(),
                             dG.data_ptr(), dfu.data_ptr() + P * 4, dfu16.data_ptr() + P * 2, None, pbs, msum, B, C_, *vol, p, st())
    assert float(dfu[:, 0].abs().max()) == 0.0
    assert rel_err(dfu, pr.grad) < 3e-5
    assert torch.equal(dfu16, dfu.to(torch.bfloat16))
    # forward sums and gradient in ONE pass (csrc/loss_fused.hip; 4 channels): the fused training step's loss chain
    if lib.vitae_loss_fwd_bwd_supported(C_, *vol, p):
        acc3 = torch.zeros(C['VITAE_ACC_COUNT'], dtype=torch.float64, device='cuda')
        d1 = torch.zeros(B, L + 1, P, device='cuda')
        d116 = torch.zeros(B, L + 1, P, dtype=torch.bfloat16, device='cuda')
        flag = torch.zeros(1, device='cuda')
        lib.vitae_loss_fwd_bwd(pp, pbs, im.data_ptr(), mk.data_ptr(), et.data_ptr(), hp.data_ptr(), d1.data_ptr() + P * 4,
                               d116.data_ptr() + P * 2, flag.data_ptr(), acc3.data_ptr(), msum, B, C_, *vol, p, st())
        assert torch.allclose(acc3[:2].cpu(), acc[:2].cpu(), rtol=1e-5), (acc3[:2], acc[:2])
        assert float(d1[:, 0].abs().max()) == 0.0 and float(flag) == 0.0
        assert rel_err(d1, pr.grad) < 3e-5, rel_err(d1, pr.grad)
        assert torch.equal(d116, d1.to(torch.bfloat16))
        # bf16 gradient only (what the bf16 step asks for): the same bits, the same sums, no fp32 store
        d216 = torch.zeros(B, L + 1, P, dtype=torch.bfloat16, device='cuda')
        acc4 = torch.zeros(C['VITAE_ACC_COUNT'], dtype=torch.float64, device='cuda')
        lib.vitae_loss_fwd_bwd(pp, pbs, im.data_ptr(), mk.data_ptr(), et.data_ptr(), hp.data_ptr(), None,
                               d216.data_ptr() + P * 2, flag.data_ptr(), acc4.data_ptr(), msum, B, C_, *vol, p, st())
        assert torch.equal(d216, d116) and torch.equal(acc4[:2], acc3[:2]) and float(flag) == 0.0
    else:
        assert C_ != 4


def test_sobel_kat_and_nan_semantics(lib):
    """centre components (-32, 96, 288), |g| = 305.26056; zero input -> NaN gradient."""
    x = torch.arange(27, dtype=torch.float32).reshape(1, 1, 3, 3, 3)
    e = torch.empty(1, 3, 3, 3, device='cuda')
    lib.vitae_sobel_edge_fwd(dev(x).data_ptr(), e.data_ptr(), None, None, 1, 1, 3, 3, 3, st())
    assert abs(float(e[0, 1, 1, 1]) - 305.26056) < 1e-3
    assert rel_err(e, R.sobel_magnitude(x)) < 1e-6
    # constant volume: interior gradient magnitude is exactly 0 -> d sqrt = 0/0 = NaN, as in the reference
    vol, p = (16, 16, 16), 8
    P, L = p ** 3, 8
    hp = torch.zeros(16, device='cuda'); hp[6:9] = 1.0
    pv = torch.ones(1, 1, *vol, device='cuda')
    ep, et = torch.empty(1, *vol, device='cuda'), torch.zeros(1, *vol, device='cuda')
    lib.vitae_sobel_edge_fwd(pv.data_ptr(), ep.data_ptr(), None, None, 1, 1, *vol, st())
    pred = torch.ones(1, L, P, device='cuda')
    mk = torch.ones(1, L, device='cuda')
    d = torch.zeros(1, L, P, device='cuda')
    flag = torch.zeros(1, device='cuda')
    lib.vitae_loss_bwd_fused(pred.data_ptr(), pv.data_ptr(), pv.data_ptr(), mk.data_ptr(), ep.data_ptr(), et.data_ptr(),
                             hp.data_ptr(), None, d.data_ptr(), None, flag.data_ptr(), L * P, 8.0, 1, 1, *vol, p, st())
    xr = torch.ones(1, 1, *vol, requires_grad=True)
    (R.sobel_magnitude(xr) ** 2).mean().backward()
    ref = xr.grad[0, 0]
    got = R.unpatchify(d.cpu(), p, (2, 2, 2))[0, 0]
    assert torch.equal(torch.isnan(got), torch.isnan(ref)) and bool(torch.isnan(ref).any())
    assert bool(torch.isnan(flag).all())        # the early non-finite flag the in-backward optimiser keys its skip on


def test_one_pass_loss_nan_semantics_and_flag(lib, C):
    """csrc/loss_fused.hip on a constant 4-channel prediction: |grad| = 0 in the interior -> the reference's sqrt backward gives
    0/0 = NaN there; the one-pass kernel must produce NaN at exactly the same voxels and raise the non-finite flag."""
    vol, p, B = (16, 16, 32), 8, 1
    L, P = (vol[0] // p) * (vol[1] // p) * (vol[2] // p), p ** 3 * 4
    cfg = R.RefConfig(volume_size=vol, patch_size=p, in_chans=4, embed_dim=48, depth=1, num_heads=3, decoder_embed_dim=32,
                      decoder_depth=1, decoder_num_heads=2)
    hp = torch.zeros(C['VITAE_HP_COUNT'], device='cuda')
    hp[C['VITAE_HP_G_RECON']], hp[C['VITAE_HP_G_EDGE']] = 1.0, 1.0
    pred = torch.ones(B, L, P, device='cuda')
    imgs = gen(B, 4, *vol, seed=5)
    mk = torch.ones(B, L, device='cuda')
    et = torch.zeros(B, *vol, device='cuda')
    d = torch.zeros(B, L, P, device='cuda')
    flag = torch.zeros(1, device='cuda')
    acc = torch.zeros(C['VITAE_ACC_COUNT'], dtype=torch.float64, device='cuda')
    assert lib.vitae_loss_fwd_bwd_supported(4, *vol, p)
    lib.vitae_loss_fwd_bwd(pred.data_ptr(), L * P, dev(imgs).data_ptr(), mk.data_ptr(), et.data_ptr(), hp.data_ptr(), d.data_ptr(), None,
                           flag.data_ptr(), acc.data_ptr(), float(L), B, 4, *vol, p, st())
    xr = torch.ones(B, 4, *vol, requires_grad=True)
    (R.sobel_magnitude(xr) ** 2).mean().backward()
    got = R.unpatchify(d.cpu(), p, cfg.grid)
    assert torch.equal(torch.isnan(got), torch.isnan(xr.grad)) and bool(torch.isnan(xr.grad).any())
    assert bool(torch.isnan(flag).all())
    # and a generic prediction leaves the flag alone
    flag.zero_()
    pred2 = dev(gen(B, L, P, seed=6))
    lib.vitae_loss_fwd_bwd(pred2.data_ptr(), L * P, dev(imgs).data_ptr(), mk.data_ptr(), et.data_ptr(), hp.data_ptr(), d.data_ptr(), None,
                           flag.data_ptr(), acc.data_ptr(), float(L), B, 4, *vol, p, st())
    assert float(flag) == 0.0 and bool(torch.isfinite(d).all())


def test_one_pass_loss_kernels_do_not_depend_on_the_piece_map(lib, C, monkeypatch):
    """csrc/loss_fused.hip: which XCD walks which pieces of the volume (VITAE_LOSS_XCD / VITAE_TARGET_XCD, read at every launch) only
    changes where halos are found — gradient and edge map bit for bit, the loss sums to the order of their atomics.  Ragged geometry:
    two x-tiles, a z-tile count that is not a multiple of 8 x-tiles (the grid is rounded up), three batch elements."""
    vol, p, B = (40, 24, 72), 8, 3
    L, P = (vol[0] // p) * (vol[1] // p) * (vol[2] // p), p ** 3 * 4
    hp = torch.zeros(C['VITAE_HP_COUNT'], device='cuda')
    hp[C['VITAE_HP_G_RECON']], hp[C['VITAE_HP_G_EDGE']] = 1.0, 0.5
    pred, imgs = dev(gen(B, L, P, seed=11)), dev(gen(B, 4, *vol, seed=12))
    mk = (dev(gen(B, L, seed=13)) > 0).float()
    taps = np.array([0.0088, 0.0271, 0.0651, 0.1216, 0.1769, 0.2010, 0.1769, 0.1216, 0.0651, 0.0271, 0.0088], dtype=np.float32)
    outs = {}
    for xcd in ('0', '1'):
        monkeypatch.setenv('VITAE_LOSS_XCD', xcd); monkeypatch.setenv('VITAE_TARGET_XCD', xcd)
        et = torch.full((B, *vol), float('nan'), device='cuda')
        lib.vitae_target_edge(imgs.data_ptr(), et.data_ptr(), taps.ctypes.data, len(taps), B, 4, *vol, st())
        d = torch.full((B, L, P), float('nan'), device='cuda')
        d16 = torch.empty(B, L, P, dtype=torch.bfloat16, device='cuda')
        acc = torch.zeros(C['VITAE_ACC_COUNT'], dtype=torch.float64, device='cuda')
        lib.vitae_loss_fwd_bwd(pred.data_ptr(), L * P, imgs.data_ptr(), mk.data_ptr(), et.data_ptr(), hp.data_ptr(), d.data_ptr(), d16.data_ptr(),
                               None, acc.data_ptr(), float(mk.sum()), B, 4, *vol, p, st())
        torch.cuda.synchronize()
        outs[xcd] = (et, d, d16, acc)
    assert bool(torch.isfinite(outs['1'][0]).all()) and bool(torch.isfinite(outs['1'][1]).all())
    for a, b in zip(outs['0'][:3], outs['1'][:3]):
        assert torch.equal(a, b)
    assert rel_err(outs['1'][3], outs['0'][3]) < 1e-12


# --------------------------------------------------------------------------- predictor pieces
@pytest.mark.parametrize('Rr,D', [(220, 768), (1760, 768), (7, 24), (130, 100)])
def test_bn1d_relu(lib, Rr, D):
    x, w, b, dy = gen(Rr, D, seed=1) * 2 + 0.5, gen(D, seed=2) + 1, gen(D, seed=3) * 0.1, gen(Rr, D, seed=4)
    bn = torch.nn.BatchNorm1d(D)
    with torch.no_grad():
        bn.weight.copy_(w); bn.bias.copy_(b)
    xr = x.clone().requires_grad_(True)
    ref = F.relu(bn(xr))
    ref.backward(dy)
    y, sm, sr = torch.empty(Rr, D, device='cuda'), torch.empty(D, device='cuda'), torch.empty(D, device='cuda')
    rm, rv = torch.zeros(D, device='cuda'), torch.ones(D, device='cuda')
    nbt = torch.zeros((), dtype=torch.int64, device='cuda')
    xd, wd, bd = dev(x), dev(w), dev(b)
    y16 = torch.empty(Rr, D, dtype=torch.bfloat16, device='cuda')
    lib.vitae_bn1d_relu_fwd(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), y16.data_ptr(), sm.data_ptr(), sr.data_ptr(),
                            rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(), Rr, D, 1e-5, 0.1, st())
    assert rel_err(y, ref) < 1e-5 and int(nbt) == 1 and torch.equal(y16, y.to(torch.bfloat16))
    assert rel_err(rm, bn.running_mean) < 1e-5 and rel_err(rv, bn.running_var) < 1e-5
    dx, dw, db = torch.empty(Rr, D, device='cuda'), torch.zeros(D, device='cuda'), torch.zeros(D, device='cuda')
    dx16 = torch.empty(Rr, D, dtype=torch.bfloat16, device='cuda')
    lib.vitae_bn1d_relu_bwd(dev(dy).data_ptr(), xd.data_ptr(), y.data_ptr(), wd.data_ptr(), sm.data_ptr(), sr.data_ptr(),
                            dx.data_ptr(), dx16.data_ptr(), dw.data_ptr(), db.data_ptr(), Rr, D, st())
    assert torch.equal(dx16, dx.to(torch.bfloat16))
    assert rel_err(dx, xr.grad) < 2e-5 and rel_err(dw, bn.weight.grad) < 2e-5 and rel_err(db, bn.bias.grad) < 2e-5


@pytest.mark.parametrize('Rr,D', [(1760, 768), (1732, 768), (100, 64), (33, 24)])
def test_bn1d_relu_row_split(lib, Rr, D):
    """vitae_bn1d_relu_{fwd,bwd}_split (rows split over workgroups, two launches each) against nn.BatchNorm1d + ReLU and against the
    one-strip-per-workgroup kernels; a column mean 100x its deviation (the statistics are merged with Chan's update)."""
    x, w, b, dy = gen(Rr, D, seed=1) * 2 + 0.5, gen(D, seed=2) + 1, gen(D, seed=3) * 0.1, gen(Rr, D, seed=4)
    x[:, 0] = 200.0 + 2.0 * gen(Rr, seed=9)
    bn = torch.nn.BatchNorm1d(D)
    with torch.no_grad():
        bn.weight.copy_(w); bn.bias.copy_(b)
    xr = x.clone().double().requires_grad_(True)
    bn = bn.double()
    ref = F.relu(bn(xr))
    ref.backward(dy.double())
    ws = torch.empty(int(lib.vitae_bn1d_split_ws_floats(Rr, D)), device='cuda')
    xd, wd, bd, dyd = dev(x), dev(w), dev(b), dev(dy)
    outs = {}
    for split in (True, False):
        y, sm, sr = torch.empty(Rr, D, device='cuda'), torch.empty(D, device='cuda'), torch.empty(D, device='cuda')
        rm, rv = torch.zeros(D, device='cuda'), torch.ones(D, device='cuda')
        nbt = torch.zeros((), dtype=torch.int64, device='cuda')
        y16 = torch.empty(Rr, D, dtype=torch.bfloat16, device='cuda')
        fa = (xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), y16.data_ptr(), sm.data_ptr(), sr.data_ptr(), rm.data_ptr(), rv.data_ptr(),
              nbt.data_ptr(), Rr, D, 1e-5, 0.1)
        if split:
            lib.vitae_bn1d_relu_fwd_split(*fa, ws.data_ptr(), st())
        else:
            lib.vitae_bn1d_relu_fwd(*fa, st())
        dx, dw, db = torch.empty(Rr, D, device='cuda'), torch.zeros(D, device='cuda'), torch.zeros(D, device='cuda')
        dx16 = torch.empty(Rr, D, dtype=torch.bfloat16, device='cuda')
        ba = (dyd.data_ptr(), xd.data_ptr(), y.data_ptr(), wd.data_ptr(), sm.data_ptr(), sr.data_ptr(), dx.data_ptr(), dx16.data_ptr(), dw.data_ptr(),
              db.data_ptr(), Rr, D)
        if split:
            lib.vitae_bn1d_relu_bwd_split(*ba, ws.data_ptr(), st())
        else:
            lib.vitae_bn1d_relu_bwd(*ba, st())
        assert int(nbt) == 1 and torch.equal(y16, y.to(torch.bfloat16)) and torch.equal(dx16, dx.to(torch.bfloat16))
        outs[split] = (y, rm, rv, dx, dw, db)
    y, rm, rv, dx, dw, db = outs[True]
    assert rel_err(y, ref) < 2e-5 and rel_err(rm, bn.running_mean) < 1e-6 and rel_err(rv, bn.running_var) < 1e-5
    assert rel_err(dx, xr.grad) < 5e-5 and rel_err(dw, bn.weight.grad) < 5e-5 and rel_err(db, bn.bias.grad) < 2e-5
    for a, c in zip(outs[True], outs[False]):
        assert rel_err(a, c) < 5e-5


def test_cosine_loss(lib, C):
    Rr, D, w, g_up = 220, 768, 0.001, 0.5
    p1, p2, z1, z2 = (gen(Rr, D, seed=s) for s in (1, 2, 3, 4))
    a, b = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
    ref = R.contrastive_loss(a, b, z1, z2, w)
    (ref * g_up).backward()
    hp = torch.zeros(C['VITAE_HP_COUNT'], device='cuda')
    hp[C['VITAE_HP_CONTR_W']], hp[C['VITAE_HP_G_CONTR']] = w, w * g_up
    acc = torch.zeros(C['VITAE_ACC_COUNT'], dtype=torch.float64, device='cuda')
    out = torch.zeros(1, device='cuda')
    d = [dev(t) for t in (p1, z2, p2, z1)]
    lib.vitae_cosine_loss_fwd(*(t.data_ptr() for t in d), acc.data_ptr(), hp.data_ptr(), out.data_ptr(), Rr, D, st())
    assert abs(float(out) - float(ref)) < 1e-9 + 1e-5 * abs(float(ref))
    dp1, dp2 = torch.empty(Rr, D, device='cuda'), torch.empty(Rr, D, device='cuda')
    lib.vitae_cosine_loss_bwd(*(t.data_ptr() for t in d), hp.data_ptr(), dp1.data_ptr(), dp2.data_ptr(), Rr, D, st())
    assert rel_err(dp1, a.grad) < 1e-5 and rel_err(dp2, b.grad) < 1e-5
    # bf16 copies (the predictor's GEMM operands), with and without the fp32 gradients; more rows than 4 x 256 workgroups cover at once
    for Rb in (Rr, 1760):
        pz = [dev(gen(Rb, D, seed=s)) for s in (5, 6, 7, 8)]
        f1, f2 = torch.empty(Rb, D, device='cuda'), torch.empty(Rb, D, device='cuda')
        lib.vitae_cosine_loss_bwd(*(t.data_ptr() for t in pz), hp.data_ptr(), f1.data_ptr(), f2.data_ptr(), Rb, D, st())
        for with_f32 in (True, False):
            g1, g2 = torch.full((Rb, D), float('nan'), device='cuda'), torch.full((Rb, D), float('nan'), device='cuda')
            h1, h2 = torch.empty(Rb, D, dtype=torch.bfloat16, device='cuda'), torch.empty(Rb, D, dtype=torch.bfloat16, device='cuda')
            lib.vitae_cosine_loss_bwd_bf16(*(t.data_ptr() for t in pz), hp.data_ptr(), g1.data_ptr() if with_f32 else None,
                                           g2.data_ptr() if with_f32 else None, h1.data_ptr(), h2.data_ptr(), Rb, D, st())
            assert torch.equal(h1, f1.to(torch.bfloat16)) and torch.equal(h2, f2.to(torch.bfloat16))
            if with_f32:
                assert torch.equal(g1, f1) and torch.equal(g2, f2)
        acc.zero_()
        lib.vitae_cosine_loss_fwd(*(t.data_ptr() for t in pz), acc.data_ptr(), hp.data_ptr(), out.data_ptr(), Rb, D, st())
        want = R.contrastive_loss(pz[0].cpu(), pz[2].cpu(), pz[3].cpu(), pz[1].cpu(), w)
        assert abs(float(out) - float(want)) < 1e-9 + 1e-5 * abs(float(want))
    # round 6: the scalar leaves with the last workgroup of the forward launch (vector widths) — the arrival counter is back at zero
    # afterwards, so a second call on the same block (sum slot cleared, nothing else) gives the same scalar; a width outside the
    # vector forms (and an unaligned operand) takes the two-launch path
    assert int(acc.view(torch.int32)[2 * C['VITAE_ACC_TICKET_C']]) == 0
    first = float(out)
    acc[C['VITAE_ACC_COS']] = 0
    out.fill_(7.0)
    lib.vitae_cosine_loss_fwd(*(t.data_ptr() for t in pz), acc.data_ptr(), hp.data_ptr(), out.data_ptr(), Rb, D, st())
    assert float(out) == pytest.approx(first, rel=1e-6)
    for Dw in (256, 512, 1024, 320):
        pz = [dev(gen(37, Dw, seed=s)) for s in (9, 10, 11, 12)]
        acc.zero_(); out.fill_(7.0)
        lib.vitae_cosine_loss_fwd(*(t.data_ptr() for t in pz), acc.data_ptr(), hp.data_ptr(), out.data_ptr(), 37, Dw, st())
        want = R.contrastive_loss(pz[0].cpu(), pz[2].cpu(), pz[3].cpu(), pz[1].cpu(), w)
        assert abs(float(out) - float(want)) < 1e-9 + 1e-5 * abs(float(want)), Dw


# --------------------------------------------------------------------------- optimiser
def test_adamw_and_gradnorm(lib, C):
    n = 100003
    p0, g1, g2 = gen(n, seed=1), gen(n, seed=2) * 0.01, gen(n, seed=3) * 0.01
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([ref], lr=3e-4, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05)
    ref64 = p0.double().requires_grad_(True)                    # the same steps in float64: what both fp32 results are measured against
    opt64 = torch.optim.AdamW([ref64], lr=3e-4, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05)
    npad = (n + 3) // 4 * 4
    p, m, v = torch.zeros(npad, device='cuda'), torch.zeros(npad, device='cuda'), torch.zeros(npad, device='cuda')
    sh = torch.zeros(npad, dtype=torch.bfloat16, device='cuda')
    p[:n] = p0.cuda()
    hp = torch.zeros(C['VITAE_HP_COUNT'], device='cuda')
    acc = torch.zeros(C['VITAE_ACC_COUNT'], dtype=torch.float64, device='cuda')
    gn = torch.zeros(1, device='cuda')
    for t, g in enumerate((g1, g2), 1):
        ref.grad = g.clone()
        opt.step()
        ref64.grad = g.double()
        opt64.step()
        gd = torch.zeros(npad, device='cuda'); gd[:n] = g.cuda()
        hp[C['VITAE_HP_LR']], hp[C['VITAE_HP_BETA1']], hp[C['VITAE_HP_BETA2']], hp[C['VITAE_HP_EPS']] = 3e-4, 0.9, 0.95, 1e-8
        hp[C['VITAE_HP_BC1']], hp[C['VITAE_HP_BC2']], hp[C['VITAE_HP_GRAD_MUL']] = 1 - 0.9 ** t, 1 - 0.95 ** t, 1.0
        acc.zero_()
        lib.vitae_grad_sqnorm(gd.data_ptr(), n, acc.data_ptr(), gn.data_ptr(), st())
        assert abs(float(gn) - float(g.norm())) < 1e-5 * float(g.norm())
        lib.vitae_adamw_step(p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), sh.data_ptr(), n, hp.data_ptr(), gn.data_ptr(), 0.05, st())
        assert rel_err(p[:n], ref) < 2e-6
        # ... and as a share of the UPDATE (max|ref| above is 4.5: an update 3 % wrong would pass it): within 3 x the error torch's
        # own fp32 AdamW makes against float64 on these inputs (tests/test_optimizer_kernels.py has the metric and the cases)
        upd = float((ref64.detach() - p0.double()).norm())
        e, e32 = float((p[:n].double().cpu() - ref64.detach()).norm()) / upd, float((ref.detach().double() - ref64.detach()).norm()) / upd
        assert e <= 3.0 * e32, (t, e, e32)
        assert torch.equal(sh[:n], p[:n].to(torch.bfloat16))
    # non-finite gradient norm -> step skipped (GradScaler.step semantics)
    before = p.clone()
    gn.fill_(float('inf'))
    lib.vitae_adamw_step(p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), None, n, hp.data_ptr(), gn.data_ptr(), 0.05, st())
    assert torch.equal(p, before)


def test_adamw_gated_by_the_accumulator(lib, C):
    """vitae_adamw_step_s16_acc (round 6): the finiteness gate read from the accumulator block — the same update as
    vitae_grad_norm_finalize + vitae_adamw_step_s16, and no update at all once any slot of the block is not finite."""
    n = 70_001
    npad = (n + 3) // 4 * 4
    gen_ = torch.Generator(device='cuda').manual_seed(11)
    hp = torch.zeros(C['VITAE_HP_COUNT'], device='cuda')
    hp[C['VITAE_HP_LR']], hp[C['VITAE_HP_BETA1']], hp[C['VITAE_HP_BETA2']], hp[C['VITAE_HP_EPS']], hp[C['VITAE_HP_GRAD_MUL']] = 3e-4, 0.9, 0.95, 1e-8, 1.0
    hp[C['VITAE_HP_BC1']], hp[C['VITAE_HP_BC2']] = 0.1, 0.05
    p0 = torch.randn(npad, device='cuda', generator=gen_) * 0.02
    g = torch.randn(npad, device='cuda', generator=gen_) * 0.01
    m0 = (torch.randn(npad, device='cuda', generator=gen_) * 0.01).bfloat16()
    v0 = (torch.rand(npad, device='cuda', generator=gen_) * 1e-4).bfloat16()
    acc = torch.zeros(C['VITAE_ACC_COUNT'], dtype=torch.float64, device='cuda')
    acc[C['VITAE_ACC_GRADSQ']] = 2.0
    acc[C['VITAE_ACC_SQ_BASE'] + 5 * C['VITAE_ACC_SQ_STRIDE']] = 7.0
    norm = torch.zeros(1, device='cuda')

    def run(gated_by_acc):
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        sh = torch.zeros(npad, dtype=torch.bfloat16, device='cuda')
        if gated_by_acc:
            rc = lib.vitae_adamw_step_s16_acc(p.data_ptr(), g.data_ptr(), 0, m.data_ptr(), v.data_ptr(), sh.data_ptr(), n, hp.data_ptr(),
                                              acc.data_ptr(), 0.05, st())
        else:
            lib.vitae_grad_norm_finalize(acc.data_ptr(), norm.data_ptr(), st())
            rc = lib.vitae_adamw_step_s16(p.data_ptr(), g.data_ptr(), 0, m.data_ptr(), v.data_ptr(), sh.data_ptr(), n, hp.data_ptr(),
                                          norm.data_ptr(), 0.05, st())
        assert rc == 0
        torch.cuda.synchronize()
        return p, m, v, sh

    a, b = run(True), run(False)
    assert float(norm) == pytest.approx(3.0)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not torch.equal(a[0], p0)
    for slot, bad in ((C['VITAE_ACC_GRADSQ'], float('nan')), (C['VITAE_ACC_SQ_BASE'] + 63 * C['VITAE_ACC_SQ_STRIDE'], float('inf'))):
        keep = float(acc[slot]); acc[slot] = bad
        a, b = run(True), run(False)
        assert torch.equal(a[0], p0) and torch.equal(a[1], m0) and torch.equal(a[2], v0) and torch.equal(b[0], p0)
        acc[slot] = keep
    with pytest.raises(Exception, match='INVALID_ARG'):
        lib.vitae_adamw_step_s16_acc(p0.data_ptr(), g.data_ptr(), 0, m0.data_ptr(), v0.data_ptr(), None, n, hp.data_ptr(), None, 0.0, st())


def test_adamw_bf16_moments(lib, C):
    """vitae_adamw_step_s16 / vitae_opt_tail(state_bf16=1) (round 6): both moments STORED in bf16, the step computed in fp32 from the
    stored values with the unrounded m_new / v_new in the parameter update — against exactly that arithmetic in torch, over four
    steps, with fp32 and with bf16 gradients; the parameters stay within fp32 round-off of the emulation and within 1e-3 of the
    update size of a plain fp32-state AdamW."""
    n = 100_003
    npad = (n + 3) // 4 * 4
    gen_ = torch.Generator(device='cuda').manual_seed(5)
    p0 = torch.randn(npad, device='cuda', generator=gen_) * 0.02
    lr, b1, b2, eps, wd = 3e-4, 0.9, 0.95, 1e-8, 0.05
    hp = torch.zeros(C['VITAE_HP_COUNT'], device='cuda')
    hp[C['VITAE_HP_LR']], hp[C['VITAE_HP_BETA1']], hp[C['VITAE_HP_BETA2']], hp[C['VITAE_HP_EPS']], hp[C['VITAE_HP_GRAD_MUL']] = lr, b1, b2, eps, 1.0
    # the kernel's coefficients: with a bias-correction slot >= 0 (as here: host-computed corrections) 1 - beta is formed in fp32 from
    # the fp32 beta (with bf16 gradients many results sit next to a bf16 rounding boundary, and the 2e-7 between fp32(1 - beta) and
    # 1 - fp32(beta) would flip a few per cent of them).  With a NEGATIVE slot it is the slot's fp32(1 - beta):
    # tests/test_optimizer_kernels.py runs the same emulation with those coefficients, at these tolerances.
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)
    omb1, omb2, b2f = float(f32(1.0) - f32(b1)), float(f32(1.0) - f32(b2)), float(f32(b2))
    for g_bf16 in (False, True):
        p, sh = p0.clone(), torch.zeros(npad, dtype=torch.bfloat16, device='cuda')
        m16, v16 = torch.zeros(npad, dtype=torch.bfloat16, device='cuda'), torch.zeros(npad, dtype=torch.bfloat16, device='cuda')
        rp, rm, rv = p0.clone(), torch.zeros(npad, device='cuda'), torch.zeros(npad, device='cuda')
        fp, fm, fv = p0.clone(), torch.zeros(npad, device='cuda'), torch.zeros(npad, device='cuda')       # plain fp32-state AdamW
        for t in range(1, 5):
            g = torch.randn(npad, device='cuda', generator=gen_) * 0.01
            if g_bf16:
                g16 = g.to(torch.bfloat16); g = g16.float()
            bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
            hp[C['VITAE_HP_BC1']], hp[C['VITAE_HP_BC2']] = bc1, bc2
            lib.vitae_adamw_step_s16(p.data_ptr(), (g16 if g_bf16 else g).data_ptr(), 1 if g_bf16 else 0, m16.data_ptr(), v16.data_ptr(), sh.data_ptr(),
                                     n, hp.data_ptr(), None, wd, st())
            for (qp, qm, qv, rnd) in ((rp, rm, rv, True), (fp, fm, fv, False)):
                mn = qm + omb1 * (g - qm)
                vn = b2f * qv + omb2 * g * g
                qp.mul_(1 - lr * wd).sub_((lr / bc1) * (mn / (vn.sqrt() / bc2 ** 0.5 + eps)))
                qm.copy_(mn.to(torch.bfloat16).float() if rnd else mn); qv.copy_(vn.to(torch.bfloat16).float() if rnd else vn)
            # (against the emulation: equal up to the few elements whose fp32 moment straddles a bf16 rounding boundary — there the
            # stored values differ by one ulp and so does a 2^-8 share of the next update)
            assert float((p[:n] - rp[:n]).norm()) < 5e-4 * float((rp[:n] - p0[:n]).norm())
            assert torch.equal(sh[:n], p[:n].to(torch.bfloat16))
            # stored moments: the emulation's value, up to one bf16 ulp where the fp32 results straddle a rounding boundary
            for got, want in ((m16, rm), (v16, rv)):
                d = got[:n].float() - want[:n]
                assert float(d.norm()) < 5e-4 * float(want[:n].norm()) and float((d != 0).float().mean()) < 2e-2
        upd = float((fp[:n] - p0[:n]).norm())
        assert float((p[:n] - fp[:n]).norm()) < 3e-3 * upd          # bf16 moments vs fp32 moments: a 2^-9-sized wobble of the update
    # the tail launcher with bf16 moments: the same arithmetic on its two segments (decayed, plain), the step count bumped
    nd, npl = 1024, 2048
    p, g = p0[:nd + npl].clone(), torch.randn(nd + npl, device='cuda', generator=gen_) * 0.01
    m16, v16 = torch.zeros(nd + npl, dtype=torch.bfloat16, device='cuda'), torch.zeros(nd + npl, dtype=torch.bfloat16, device='cuda')
    acc, gn = torch.zeros(C['VITAE_ACC_COUNT'], dtype=torch.float64, device='cuda'), torch.zeros(1, device='cuda')
    hp[C['VITAE_HP_BC1']], hp[C['VITAE_HP_BC2']], hp[C['VITAE_HP_STEP']] = 1 - b1, 1 - b2, 0.0
    lib.vitae_opt_tail(p.data_ptr(), g.data_ptr(), 0, m16.data_ptr(), v16.data_ptr(), 1, None, nd, npl, hp.data_ptr(), acc.data_ptr(), gn.data_ptr(), wd, st())
    want = p0[:nd + npl].clone()
    want[:nd] *= 1 - lr * wd
    mn, vn = (1 - b1) * g, (1 - b2) * g * g
    want -= (lr / (1 - b1)) * (mn / (vn.sqrt() / (1 - b2) ** 0.5 + eps))
    assert rel_err(p, want) < 2e-6 and abs(float(gn) - float(g.norm())) < 1e-5 * float(g.norm()) and float(hp[C['VITAE_HP_STEP']]) == 1.0
    assert torch.equal(m16, mn.to(torch.bfloat16)) and rel_err(v16.float(), vn) < 2.0 ** -8


def test_adamw_and_gradnorm_from_bf16_gradients(lib, C):
    """The bf16-gradient entry points (reduced gradients consumed from the all-reduce's wire buffer) equal the fp32
    ones applied to the same bf16-rounded values, bit for bit."""
    n = 100_003
    npad = (n + 3) // 4 * 4
    g = torch.Generator(device='cuda').manual_seed(3)
    p0 = torch.randn(npad, device='cuda', generator=g) * 0.02
    g16 = (torch.randn(npad, device='cuda', generator=g) * 0.01).to(torch.bfloat16)
    g32 = g16.float()
    hp = torch.zeros(C['VITAE_HP_COUNT'], device='cuda')
    hp[C['VITAE_HP_LR']], hp[C['VITAE_HP_BETA1']], hp[C['VITAE_HP_BETA2']], hp[C['VITAE_HP_EPS']] = 3e-4, 0.9, 0.95, 1e-8
    hp[C['VITAE_HP_BC1']], hp[C['VITAE_HP_BC2']], hp[C['VITAE_HP_GRAD_MUL']] = 0.1, 0.05, 1.0
    outs = []
    for bf in (False, True):
        p, m, v = p0.clone(), torch.zeros(npad, device='cuda'), torch.zeros(npad, device='cuda')
        sh = torch.zeros(npad, dtype=torch.bfloat16, device='cuda')
        acc = torch.zeros(C['VITAE_ACC_COUNT'], dtype=torch.float64, device='cuda')
        gn = torch.zeros(1, device='cuda')
        if bf:
            lib.vitae_grad_sqnorm_bf16(g16.data_ptr(), n, acc.data_ptr(), gn.data_ptr(), st())
            lib.vitae_adamw_step_bf16g(p.data_ptr(), g16.data_ptr(), m.data_ptr(), v.data_ptr(), sh.data_ptr(), n, hp.data_ptr(),
                                       gn.data_ptr(), 0.05, st())
        else:
            lib.vitae_grad_sqnorm(g32.data_ptr(), n, acc.data_ptr(), gn.data_ptr(), st())
            lib.vitae_adamw_step(p.data_ptr(), g32.data_ptr(), m.data_ptr(), v.data_ptr(), sh.data_ptr(), n, hp.data_ptr(),
                                 gn.data_ptr(), 0.05, st())
        outs.append((p, m, v, sh, gn.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert abs(float(outs[0][4]) - float(g32[:n].norm())) < 1e-5 * float(g32[:n].norm())


# --------------------------------------------------------------------------- bf16-input attention, bf16 pre-activation
def _bf(t):
    return t.to(torch.bfloat16)


@pytest.mark.parametrize('B,N,H,hd', [(8, 55, 12, 64), (4, 217, 16, 32), (2, 129, 16, 64), (1, 17, 4, 32), (2, 433, 4, 64), (1, 1729, 2, 32)])
def test_sdpa_mfma_bf16_input(lib, B, N, H, hd):
    """Attention forward + backward (one launch when the head fits LDS, the two streaming kernels at N = 433 / 1729) reading
    q | k | v from the bf16 copy the qkv GEMM writes: same results as the
    fp32-input kernels fed the bf16-rounded values (they round while staging; only q's softmax scale is applied after the rounding
    here), and the reference within the usual bf16 bounds."""
    D = H * hd
    qkv = _bf(gen(B, N, 3 * D, seed=1)).float()
    do = gen(B, N, D, seed=2)
    assert lib.vitae_sdpa_bwd_fused_fits(N, hd) == (0 if N > 256 else 1)
    qd, q16, dod = dev(qkv), dev(_bf(qkv)), dev(do)
    outs = []
    for bf in (False, True):
        o, lse = torch.full((B, N, D), float('nan'), device='cuda'), torch.empty(B * H * N, device='cuda')
        o16 = torch.empty(B, N, D, dtype=torch.bfloat16, device='cuda')
        g16 = torch.empty(B, N, 3 * D, dtype=torch.bfloat16, device='cuda')
        cs = torch.zeros(3 * D, device='cuda')
        if bf:
            lib.vitae_sdpa_mfma_fwd_bf16in(q16.data_ptr(), o.data_ptr(), o16.data_ptr(), lse.data_ptr(), B, N, H, hd, st())
            delta = torch.empty(B * H * N, device='cuda')
            lib.vitae_sdpa_mfma_bwd_bf16in(q16.data_ptr(), o.data_ptr(), dod.data_ptr(), lse.data_ptr(), None, g16.data_ptr(), cs.data_ptr(),
                                           delta.data_ptr(), B, N, H, hd, st())
        else:
            delta = torch.empty(B * H * N, device='cuda')
            lib.vitae_sdpa_mfma_fwd(qd.data_ptr(), o.data_ptr(), o16.data_ptr(), lse.data_ptr(), B, N, H, hd, st())
            lib.vitae_sdpa_mfma_bwd(qd.data_ptr(), o.data_ptr(), dod.data_ptr(), lse.data_ptr(), None, g16.data_ptr(), cs.data_ptr(),
                                    delta.data_ptr(), B, N, H, hd, st())
        outs.append((o.cpu(), lse.cpu(), g16.float().cpu(), cs.cpu()))
    (o0, l0, g0, c0), (o1, l1, g1, c1) = outs
    assert rel_err(o1, o0) < 1e-2 and float((l1 - l0).abs().max()) < 2e-2
    assert rel_err(g1, g0) < 2e-2 and rel_err(c1, c0) < 2e-2
    qr = qkv.clone().requires_grad_(True)
    q, k, v = qr.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    ref = (((q @ k.transpose(-2, -1)) * hd ** -0.5).softmax(-1) @ v).transpose(1, 2).reshape(B, N, D)
    ref.backward(do)
    assert rel_err(o1, ref) < 2e-2
    g, got = qr.grad.reshape(B, N, 3, D), g1.reshape(B, N, 3, D)
    for i, name in enumerate('qkv'):
        assert rel_err(got[:, :, i], g[:, :, i]) < 3e-2, name


@pytest.mark.parametrize('M,N,K', [(440, 3072, 768), (868, 2048, 512), (70, 512, 512)])
def test_gemm_bf16_saved_preactivation(lib, C, M, N, K):
    """VITAE_EPI_AUX_BF16: the fc1 epilogue saves its pre-activation in bf16 and the fc2 input gradient's GELU' reads that."""
    Mp = (M + 63) // 64 * 64
    x, w, bias = _bf(gen(M, K, seed=1)).float(), _bf(gen(N, K, seed=2, scale=K ** -0.5)).float(), gen(N, seed=3)
    x16 = torch.zeros(Mp, K, dtype=torch.bfloat16, device='cuda'); x16[:M] = _bf(x).cuda()
    w16 = dev(_bf(w))
    y16 = torch.zeros(Mp, N, dtype=torch.bfloat16, device='cuda')
    aux16 = torch.full((M, N), float('nan'), dtype=torch.bfloat16, device='cuda')
    lib.vitae_gemm_glds(1, 1, x16.data_ptr(), K, w16.data_ptr(), K, None, 0, y16.data_ptr(), N, M, N, K, dev(bias).data_ptr(), None, 0,
                        C['VITAE_EPI_GELU'] | C['VITAE_EPI_AUX_BF16'], aux16.data_ptr(), N, 0, 1, None, None, st())
    pre = x @ w.t() + bias
    assert rel_err(aux16.float(), pre) < 1e-2
    assert rel_err(y16[:M].float(), F.gelu(pre)) < 2e-2
    # backward of the NEXT Linear (fc2): dh = (dy @ W2) * gelu'(pre), pre read from the bf16 copy
    D2 = 256
    dy, w2 = _bf(gen(M, D2, seed=4)).float(), _bf(gen(D2, N, seed=5, scale=N ** -0.5)).float()
    dy16 = torch.zeros(Mp, D2, dtype=torch.bfloat16, device='cuda'); dy16[:M] = _bf(dy).cuda()
    dh16 = torch.zeros(Mp, N, dtype=torch.bfloat16, device='cuda')
    dw = torch.full((D2, N), float('nan'), device='cuda')
    sp = lib.vitae_linear_bwd_pair_pick_split_k(M, Mp, D2, N)
    ws = torch.zeros(max(1, lib.vitae_gemm_glds_ws_floats(M, N, max(sp, 1))), device='cuda')
    lib.vitae_linear_bwd_pair_glds(dy16.data_ptr(), dev(_bf(w2)).data_ptr(), y16.data_ptr(), None, dh16.data_ptr(), dw.data_ptr(), None,
                                   M, Mp, D2, N, C['VITAE_EPI_DGELU'] | C['VITAE_EPI_AUX_BF16'], aux16.data_ptr(), None, None, 0, 0, sp,
                                   ws.data_ptr(), ws.numel(), st())
    p = aux16.float().cpu().requires_grad_(True)
    F.gelu(p).backward(dy @ w2)
    assert rel_err(dh16[:M].float(), p.grad) < 2e-2
    assert rel_err(dw, dy.t() @ y16[:M].float().cpu()) < 1e-2
    # the same pair with the DERIVATIVE saved by the forward (VITAE_EPI_AUX_DERIV): GELU'(fp32 pre-activation) rounded once
    DV = C['VITAE_EPI_AUX_DERIV']
    der16 = torch.full((M, N), float('nan'), dtype=torch.bfloat16, device='cuda')
    y16b = torch.zeros(Mp, N, dtype=torch.bfloat16, device='cuda')
    lib.vitae_gemm_glds(1, 1, x16.data_ptr(), K, w16.data_ptr(), K, None, 0, y16b.data_ptr(), N, M, N, K, dev(bias).data_ptr(), None, 0,
                        C['VITAE_EPI_GELU'] | C['VITAE_EPI_AUX_BF16'] | DV, der16.data_ptr(), N, 0, 1, None, None, st())
    pg = pre.clone().requires_grad_(True)
    F.gelu(pg).sum().backward()
    assert torch.equal(y16b, y16) and rel_err(der16.float(), pg.grad) < 1e-2
    dh16b = torch.zeros(Mp, N, dtype=torch.bfloat16, device='cuda')
    lib.vitae_linear_bwd_pair_glds(dy16.data_ptr(), dev(_bf(w2)).data_ptr(), y16.data_ptr(), None, dh16b.data_ptr(), dw.data_ptr(), None,
                                   M, Mp, D2, N, C['VITAE_EPI_DGELU'] | C['VITAE_EPI_AUX_BF16'] | DV, der16.data_ptr(), None, None, 0, 0, sp,
                                   ws.data_ptr(), ws.numel(), st())
    assert rel_err(dh16b[:M].float(), (dy @ w2) * pg.grad) < 2e-2


@pytest.mark.parametrize('M,N,K', [(868, 2048, 512), (440, 3072, 768), (70, 520, 128), (1736, 2048, 512), (6944, 2048, 512), (3520, 3072, 768)])
def test_gemm_two_plane_weight(lib, C, M, N, K):
    """vitae_gemm_glds_w2 + vitae_cast_bf16_hilo: y = x16 (W_hi + W_lo)^T carries the fp32 weight to ~2^-17 (the one-plane launch: 2^-9) —
    few rows on the two-plane 64 x 64 workgroup, many rows on a big tile over 2 K with the activations wrapping; GELU epilogue with the
    saved derivative, residual form, split-K."""
    x = _bf(gen(M, K, seed=1)).float()
    w = gen(3, N, K, seed=2, scale=K ** -0.5)                       # three equally spaced tensors: the strided cast
    bias, res = gen(N, seed=3), gen(M, N, seed=4)
    wd = dev(w)
    x16 = _bf(x).cuda()
    hi = wd.to(torch.bfloat16)
    hilo = torch.full((3, N, 2 * K), float('nan'), dtype=torch.bfloat16, device='cuda')
    lib.vitae_cast_bf16_hilo(wd.data_ptr(), hilo.data_ptr(), N, K, N * K, 3, st())
    assert torch.equal(hilo[:, :, :K], hi) and torch.equal(hilo[:, :, K:], (wd - hi.float()).to(torch.bfloat16))
    t = 1
    ref = x.double() @ w[t].double().t()
    nan = lambda: torch.full((M, N), float('nan'), device='cuda')
    y1 = nan()
    lib.vitae_gemm_glds(1, 1, x16.data_ptr(), K, hi[t].data_ptr(), K, y1.data_ptr(), N, None, 0, M, N, K, None, None, 0, 0, None, 0, 0, 1, None, None, st())
    ws = torch.zeros(max(1, lib.vitae_gemm_glds_ws_floats(M, N, 8)), device='cuda')
    sp = lib.vitae_gemm_glds_w2_pick_split_k(M, N, K)
    y2 = nan()
    lib.vitae_gemm_glds_w2(x16.data_ptr(), K, hilo[t].data_ptr(), y2.data_ptr(), N, None, 0, M, N, K, None, None, 0, 0, None, 0, 0, sp,
                           ws.data_ptr(), None, st())
    e1, e2 = rel_err(y1, ref), rel_err(y2, ref)
    assert e2 < 3e-5 and e2 < e1 / 20, (e1, e2)                      # observed ~2e-3 against ~1e-5
    # GELU + saved derivative (bf16), bf16-only result — the decoder fc1 launch of the bf16 step
    DV = C['VITAE_EPI_GELU'] | C['VITAE_EPI_AUX_BF16'] | C['VITAE_EPI_AUX_DERIV']
    y16, der16 = torch.zeros(M, N, dtype=torch.bfloat16, device='cuda'), torch.zeros(M, N, dtype=torch.bfloat16, device='cuda')
    lib.vitae_gemm_glds_w2(x16.data_ptr(), K, hilo[t].data_ptr(), None, 0, y16.data_ptr(), N, M, N, K, dev(bias).data_ptr(), None, 0,
                           DV, der16.data_ptr(), N, 0, 1, None, None, st())
    pre = (ref + bias.double()).float().requires_grad_(True)
    F.gelu(pre).sum().backward()
    assert rel_err(y16.float(), F.gelu(pre.detach())) < 1e-2 and rel_err(der16.float(), pre.grad) < 1e-2
    # bias + residual on the two-plane workgroup with an in-launch split-K (any split other than the plan's goes there)
    if K >= 256:
        y3 = nan()
        lib.vitae_gemm_glds_w2(x16.data_ptr(), K, hilo[t].data_ptr(), y3.data_ptr(), N, None, 0, M, N, K, dev(bias).data_ptr(),
                               dev(res).data_ptr(), N, 0, None, 0, 0, 2, ws.data_ptr(), None, st())
        assert rel_err(y3, ref + bias.double() + res.double()) < 3e-5
        assert int(ws[:C['VITAE_GLDS_TICKETS']].abs().sum()) == 0


# ---------------------------------------------------------------------------------------------------------------------
# big-tile GEMM family (csrc/gemm_bt.hip) behind vitae_gemm_glds / vitae_linear_bwd_pair_glds
@pytest.fixture
def bt_mode(lib):
    yield lib.vitae_gemm_glds_set_bt_tile
    lib.vitae_gemm_glds_set_bt_tile(-1)


def _bt_operands(form, M, N, K, seed=0):
    akc, bkc = {'fwd': (1, 1), 'dgrad': (1, 0), 'wgrad': (0, 0)}[form]
    A = gen(*((M, K) if akc else (K, M)), seed=seed + 1).cuda().to(torch.bfloat16)
    B = gen(*((N, K) if bkc else (K, N)), seed=seed + 2, scale=K ** -0.5).cuda().to(torch.bfloat16)
    Af = A.float().cpu() if akc else A.float().cpu().t()
    Bf = B.float().cpu() if bkc else B.float().cpu().t()
    return akc, bkc, A, B, Af @ Bf.t()


@pytest.mark.parametrize('tile', [0, 3, 4, 5])
@pytest.mark.parametrize('form', ['fwd', 'dgrad', 'wgrad'])
@pytest.mark.parametrize('M,N,K', [(868, 16384, 512), (440, 776, 192), (1000, 520, 128), (300, 264, 640), (130, 128, 1024)])
def test_gemm_bt_forms_and_epilogues(lib, C, bt_mode, tile, form, M, N, K):
    """Every operand form of the big tiles on ragged shapes (rows / columns that do not fill the last tile, tiles with a whole
    half outside the matrix), with each epilogue kind of the row-major epilogue: bias + residual + bf16 copy + column sums,
    accumulate into C, GELU with the saved pre-activation (fp32 and bf16), GELU', ReLU mask, ReLU, bf16-only output."""
    if form == 'wgrad':
        M = M // 8 * 8            # row-contiguous operands move in 16-byte chunks of rows
    akc, bkc, A, B, prod = _bt_operands(form, M, N, K)
    lda, ldb = (K if akc else M), (K if bkc else N)
    bt_mode(tile)
    assert lib.vitae_gemm_glds_bt_choice(akc, bkc, M, N, K) == tile      # a forced tile serves every shape the kernel can run
    b, res, old, aux = gen(N, seed=3), gen(M, N, seed=4), gen(M, N, seed=5), gen(M, N, seed=6)
    bd, rd, auxd = dev(b), dev(res), dev(aux)
    aux16 = aux.cuda().to(torch.bfloat16)
    nan = lambda: torch.full((M, N), float('nan'), device='cuda')

    def run(C_, C16, bias, resid, epi, auxp, acc, colsum=None):
        lib.vitae_gemm_glds(akc, bkc, A.data_ptr(), lda, B.data_ptr(), ldb, None if C_ is None else C_.data_ptr(), N,
                            None if C16 is None else C16.data_ptr(), N, M, N, K, None if bias is None else bias.data_ptr(),
                            None if resid is None else resid.data_ptr(), N, epi, None if auxp is None else auxp.data_ptr(), N, acc, 1, None,
                            None if colsum is None else colsum.data_ptr(), st())
    # kind 1: bias + residual, bf16 copy, column sums
    y, y16, cs = nan(), torch.zeros(M, N, dtype=torch.bfloat16, device='cuda'), torch.zeros(N, device='cuda')
    run(y, y16, bd, rd, 0, None, 0, cs)
    assert rel_err(y, prod + b + res) < 2e-3
    assert torch.equal(y16, y.to(torch.bfloat16)) and rel_err(cs, y.sum(0)) < 1e-4
    # kind 0 and 2: plain, then accumulate on top
    y = nan(); run(y, None, None, None, 0, None, 0)
    assert rel_err(y, prod) < 2e-3
    y2 = dev(old); run(y2, None, None, None, 0, None, 1)
    assert rel_err(y2, prod + old) < 2e-3
    # kind 7 (generic): residual AND accumulate
    y2 = dev(old); run(y2, None, bd, rd, 0, None, 1)
    assert rel_err(y2, prod + b + res + old) < 2e-3
    # kind 3: GELU, pre-activation saved in fp32 / bf16, bf16-only result
    pre, y16 = nan(), torch.zeros(M, N, dtype=torch.bfloat16, device='cuda')
    run(None, y16, bd, None, C['VITAE_EPI_GELU'], pre, 0)
    assert rel_err(pre, prod + b) < 2e-3 and rel_err(y16.float(), F.gelu(prod + b)) < 1e-2
    pre16 = torch.zeros(M, N, dtype=torch.bfloat16, device='cuda')
    run(None, y16, bd, None, C['VITAE_EPI_GELU'] | C['VITAE_EPI_AUX_BF16'], pre16, 0)
    assert rel_err(pre16.float(), prod + b) < 1e-2 and rel_err(y16.float(), F.gelu(prod + b)) < 1e-2
    # kind 4: GELU'(aux) (fp32 and bf16 aux), kind 5: ReLU mask, kind 6: ReLU
    a_ = aux.clone().requires_grad_(True)
    F.gelu(a_).backward(prod)
    y = nan(); run(y, None, None, None, C['VITAE_EPI_DGELU'], auxd, 0)
    assert rel_err(y, a_.grad) < 2e-3
    a16 = aux16.float().cpu().requires_grad_(True)
    F.gelu(a16).backward(prod)
    y = nan(); run(y, None, None, None, C['VITAE_EPI_DGELU'] | C['VITAE_EPI_AUX_BF16'], aux16, 0)
    assert rel_err(y, a16.grad) < 2e-3
    y = nan(); run(y, None, None, None, C['VITAE_EPI_RELU_MASK'], auxd, 0)
    assert rel_err(y, torch.where(aux > 0, prod, torch.zeros(()))) < 2e-3
    y = nan(); run(y, None, bd, None, C['VITAE_EPI_RELU'], None, 0)
    assert rel_err(y, F.relu(prod + b)) < 2e-3
    # VITAE_EPI_AUX_DERIV: GELU saves GELU'(pre-activation) (fp32 / bf16), GELU' multiplies by the saved derivative
    DV = C['VITAE_EPI_AUX_DERIV']
    pb = (prod + b).clone().requires_grad_(True)
    F.gelu(pb).sum().backward()
    der, y16 = nan(), torch.zeros(M, N, dtype=torch.bfloat16, device='cuda')
    run(None, y16, bd, None, C['VITAE_EPI_GELU'] | DV, der, 0)
    assert rel_err(der, pb.grad) < 2e-3 and rel_err(y16.float(), F.gelu(prod + b)) < 1e-2
    der16 = torch.zeros(M, N, dtype=torch.bfloat16, device='cuda')
    run(None, y16, bd, None, C['VITAE_EPI_GELU'] | C['VITAE_EPI_AUX_BF16'] | DV, der16, 0)
    assert rel_err(der16.float(), pb.grad) < 1e-2 and rel_err(y16.float(), F.gelu(prod + b)) < 1e-2
    y = nan(); run(y, None, None, None, C['VITAE_EPI_DGELU'] | DV, auxd, 0)
    assert rel_err(y, prod * aux) < 2e-3
    y = nan(); run(y, None, None, None, C['VITAE_EPI_DGELU'] | C['VITAE_EPI_AUX_BF16'] | DV, aux16, 0)
    assert rel_err(y, prod * aux16.float().cpu()) < 2e-3


@pytest.mark.parametrize('tile', [3, 4, 5])
@pytest.mark.parametrize('form', ['fwd', 'dgrad', 'wgrad'])
@pytest.mark.parametrize('M,N,K,split', [(880, 768, 3072, 6), (440, 520, 1024, 2), (3456, 768, 4096, 3), (300, 264, 640, 2)])
def test_gemm_bt_split_k(lib, C, bt_mode, tile, form, M, N, K, split):
    """In-launch split-K of the 128x128 tiles (3: every wave loads and multiplies, 4: wave-specialised): partials through write-through stores, last arriver sums in split order —
    equal to the unsplit launch up to fp32 summation order, bitwise reproducible, tickets handed back, epilogue applied once."""
    if form == 'wgrad':
        M = M // 8 * 8
    akc, bkc, A, B, prod = _bt_operands(form, M, N, K, seed=7)
    lda, ldb = (K if akc else M), (K if bkc else N)
    bt_mode(tile)
    res, bd = dev(gen(M, N, seed=4)), dev(gen(N, seed=3))
    ws = torch.zeros(lib.vitae_gemm_glds_ws_floats(M, N, split), device='cuda')
    outs = []
    sq = torch.zeros(1, dtype=torch.float64, device='cuda')
    for rep in range(2):
        y, cs = torch.full((M, N), float('nan'), device='cuda'), torch.zeros(N, device='cuda')
        if form == 'wgrad':
            lib.vitae_gemm_glds_set_wgrad_sqnorm(sq.data_ptr())
        try:
            lib.vitae_gemm_glds(akc, bkc, A.data_ptr(), lda, B.data_ptr(), ldb, y.data_ptr(), N, None, 0, M, N, K, bd.data_ptr(), res.data_ptr(), N,
                                0, None, 0, 0, split, ws.data_ptr(), cs.data_ptr(), st())
        finally:
            lib.vitae_gemm_glds_set_wgrad_sqnorm(None)
        assert rel_err(y, prod + bd.cpu() + res.cpu()) < 2e-3 and rel_err(cs, y.sum(0)) < 1e-4
        assert int(ws[:C['VITAE_GLDS_TICKETS']].abs().sum()) == 0
        outs.append(y)
    assert torch.equal(outs[0], outs[1])
    if form == 'wgrad':
        assert abs(float(sq) - 2 * float(outs[0].double().pow(2).sum())) < 1e-4 * float(sq)      # one share per launch, every element once


def test_wgrad_sqnorm_spread_slots(lib, C):
    """vitae_gemm_glds_set_wgrad_sqnorm_spread (round 6): the weight-gradient workgroups of a paired launch add their squares to the
    VITAE_ACC_SQ_SLOTS spread slots of the accumulator block (same-address double atomics retire one per ~10 ns); vitae_grad_norm_finalize
    sums the slots and acc[GRADSQ]; a second launch keeps adding; bad slot counts are refused."""
    M, N, K = 440, 768, 3072
    Mp = (M + 63) // 64 * 64
    x16 = torch.zeros(Mp, K, dtype=torch.bfloat16, device='cuda'); x16[:M] = gen(M, K, seed=1).cuda().to(torch.bfloat16)
    dy16 = torch.zeros(Mp, N, dtype=torch.bfloat16, device='cuda'); dy16[:M] = gen(M, N, seed=5).cuda().to(torch.bfloat16)
    w16 = gen(N, K, seed=2, scale=K ** -0.5).cuda().to(torch.bfloat16)
    dx, dw = torch.empty(M, K, device='cuda'), torch.empty(N, K, device='cuda')
    acc = torch.zeros(C['VITAE_ACC_COUNT'], dtype=torch.float64, device='cuda')
    gn = torch.zeros(1, device='cuda')
    ws = torch.zeros(1 << 22, device='cuda')
    base, slots, stride = C['VITAE_ACC_SQ_BASE'], C['VITAE_ACC_SQ_SLOTS'], C['VITAE_ACC_SQ_STRIDE']
    assert C['VITAE_ACC_COUNT'] >= base + slots * stride
    with pytest.raises(Exception):
        lib.vitae_gemm_glds_set_wgrad_sqnorm_spread(acc.data_ptr(), 48, 16)
    split = lib.vitae_linear_bwd_pair_pick_split_k(M, Mp, N, K)
    lib.vitae_gemm_glds_set_wgrad_sqnorm_spread(acc.data_ptr() + 8 * base, slots, stride)
    try:
        for rep in (1, 2):
            lib.vitae_linear_bwd_pair_glds(dy16.data_ptr(), w16.data_ptr(), x16.data_ptr(), dx.data_ptr(), None, dw.data_ptr(), None, M, Mp, N, K,
                                           0, None, None, None, 0, 0, split, ws.data_ptr(), ws.numel(), st())
            lib.vitae_grad_norm_finalize(acc.data_ptr(), gn.data_ptr(), st())
            want = float(dw.double().pow(2).sum()) * rep
            got = acc[base:base + slots * stride].view(slots, stride)
            assert float(got[:, 1:].abs().sum()) == 0.0 and int((got[:, 0] != 0).sum()) == slots      # every slot used, nothing beside them
            assert abs(float(got[:, 0].sum()) - want) < 1e-6 * want
            assert abs(float(gn) - want ** 0.5) < 1e-5 * want ** 0.5
    finally:
        lib.vitae_gemm_glds_set_wgrad_sqnorm(None)
    acc[C['VITAE_ACC_GRADSQ']] = 9.0          # the single slot still counts
    lib.vitae_grad_norm_finalize(acc.data_ptr(), gn.data_ptr(), st())
    assert abs(float(gn) - (want + 9.0) ** 0.5) < 1e-5 * want ** 0.5


@pytest.mark.parametrize('M,N,K,split', [(2304, 768, 3520, 1), (768, 3072, 3520, 2), (440, 520, 1024, 2), (296, 264, 640, 1), (16384, 512, 896, 1),
                                         (136, 776, 192, 1)])
def test_gemm_ws_128x256_weight_gradient_tile(lib, C, bt_mode, M, N, K, split):
    """Tile id 6 (csrc/gemm_bt.hip: gemm_wsw_body — wave-specialised 128 x 256, weight-gradient form only): ragged shapes, accumulate,
    bf16 copy, in-launch split-K (bitwise reproducible, tickets handed back), the squared-norm share; other forms are not served."""
    akc, bkc, A, B, prod = _bt_operands('wgrad', M, N, K, seed=9)
    bt_mode(6)
    assert lib.vitae_gemm_glds_bt_choice(0, 0, M, N, K) == 6 and lib.vitae_gemm_glds_bt_choice(1, 1, M, N, K) == -1
    ws = torch.zeros(max(lib.vitae_gemm_glds_ws_floats(M, N, split), 4096), device='cuda')
    old = gen(M, N, seed=5)
    sq = torch.zeros(1, dtype=torch.float64, device='cuda')
    outs = []
    for rep in range(2):
        y, y16 = torch.full((M, N), float('nan'), device='cuda'), torch.zeros(M, N, dtype=torch.bfloat16, device='cuda')
        lib.vitae_gemm_glds_set_wgrad_sqnorm(sq.data_ptr())
        try:
            lib.vitae_gemm_glds(0, 0, A.data_ptr(), M, B.data_ptr(), N, y.data_ptr(), N, y16.data_ptr(), N, M, N, K, None, None, 0, 0, None, 0, 0, split,
                                ws.data_ptr(), None, st())
        finally:
            lib.vitae_gemm_glds_set_wgrad_sqnorm(None)
        assert rel_err(y, prod) < 2e-3 and torch.equal(y16, y.to(torch.bfloat16))
        assert int(ws[:C['VITAE_GLDS_TICKETS']].abs().sum()) == 0
        outs.append(y)
    assert torch.equal(outs[0], outs[1])
    assert abs(float(sq) - 2 * float(outs[0].double().pow(2).sum())) < 1e-4 * float(sq)
    y2 = dev(old)
    lib.vitae_gemm_glds(0, 0, A.data_ptr(), M, B.data_ptr(), N, y2.data_ptr(), N, None, 0, M, N, K, None, None, 0, 0, None, 0, 1, split, ws.data_ptr(), None, st())
    assert rel_err(y2, prod + old) < 2e-3


@pytest.mark.parametrize('tile', [0, 3, 4, 5])
@pytest.mark.parametrize('M,N,K', [(868, 16384, 512), (3464, 768, 768), (880, 3072, 768), (440, 2304, 768)])
def test_linear_bwd_pair_on_big_tiles(lib, C, bt_mode, tile, M, N, K):
    """vitae_linear_bwd_pair_glds when the planner serves a half with a big tile: the halves leave as two launches — same
    results as the paired launch (dx with GELU', its bf16 copy and column sums; dW, its bf16 copy; the bias gradient)."""
    Mp = (M + 63) // 64 * 64
    x, w, dy, h = gen(M, K, seed=1), gen(N, K, seed=2, scale=K ** -0.5), gen(M, N, seed=5), gen(M, K, seed=6)
    x16 = torch.zeros(Mp, K, dtype=torch.bfloat16, device='cuda'); x16[:M] = x.cuda().to(torch.bfloat16)
    dy16 = torch.zeros(Mp, N, dtype=torch.bfloat16, device='cuda'); dy16[:M] = dy.cuda().to(torch.bfloat16)
    w16, hd_ = w.cuda().to(torch.bfloat16), dev(h)
    ws = torch.zeros(1 << 24, device='cuda')
    outs = {}
    for mode in (-2, tile):
        bt_mode(mode)
        dx, dx16 = torch.full((M, K), float('nan'), device='cuda'), torch.zeros(M, K, dtype=torch.bfloat16, device='cuda')
        dw, dw16 = torch.full((N, K), float('nan'), device='cuda'), torch.zeros(N, K, dtype=torch.bfloat16, device='cuda')
        cs, dycs = torch.zeros(K, device='cuda'), torch.zeros(N, device='cuda')
        split = lib.vitae_linear_bwd_pair_pick_split_k(M, Mp, N, K)
        lib.vitae_linear_bwd_pair_glds(dy16.data_ptr(), w16.data_ptr(), x16.data_ptr(), dx.data_ptr(), dx16.data_ptr(), dw.data_ptr(), dw16.data_ptr(),
                                       M, Mp, N, K, C['VITAE_EPI_DGELU'], hd_.data_ptr(), cs.data_ptr(), dycs.data_ptr(), 0, 0, split, ws.data_ptr(), ws.numel(), st())
        assert torch.equal(dx16, dx.to(torch.bfloat16)) and torch.equal(dw16, dw.to(torch.bfloat16))
        assert int(ws[:C['VITAE_GLDS_TICKETS']].abs().sum()) == 0
        outs[mode] = (dx, dw, cs, dycs)
    dyr, wr, xr = dy16[:M].float().cpu(), w16.float().cpu(), x16[:M].float().cpu()
    hh = h.clone().requires_grad_(True)
    F.gelu(hh).backward(dyr @ wr)
    for mode, (dx, dw, cs, dycs) in outs.items():
        assert rel_err(dx, hh.grad) < 2e-3 and rel_err(dw, dyr.t() @ xr) < 2e-3, mode
        assert rel_err(cs, dx.sum(0)) < 1e-4 and rel_err(dycs, dyr.sum(0)) < 1e-5, mode
    for a, b in zip(outs[-2], outs[tile]):
        assert rel_err(a, b) < 1e-5           # the two routes differ in fp32 summation order only


@pytest.mark.parametrize('M,dims', [(3520, [(2304, 768), (768, 768), (3072, 768), (768, 3072)]), (1000, [(1536, 512), (512, 512)]),
                                    (6944, [(512, 2048)]), (260, [(264, 136), (128, 520), (520, 128)])])
@pytest.mark.parametrize('kind', [-1, 3, 4, 6])
def test_wgrad_group_bt(lib, bt_mode, M, dims, kind):
    """vitae_wgrad_group_bt: the weight gradients (and bias gradients) of up to four Linears of a block in one launch of 128x128
    tiles — the planner's kind, the ping-pong workgroups (forced tile 3), the wave-specialised ones (4) and their 128 x 256 form (6) — against fp32 products of
    the same bf16 operands; accumulation and the bf16 copy."""
    import numpy as np
    bt_mode(kind)
    Mp = (M + 63) // 64 * 64
    n = len(dims)
    dys = [torch.zeros(Mp, N, dtype=torch.bfloat16, device='cuda') for N, K in dims]
    xs = [torch.zeros(Mp, K, dtype=torch.bfloat16, device='cuda') for N, K in dims]
    for i, (N, K) in enumerate(dims):
        dys[i][:M] = dev(_bf(gen(M, N, seed=10 + i)))
        xs[i][:M] = dev(_bf(gen(M, K, seed=20 + i)))
    dws = [torch.full((N, K), float('nan'), device='cuda') for N, K in dims]
    d16 = [torch.empty(N, K, dtype=torch.bfloat16, device='cuda') for N, K in dims]
    dbs = [torch.zeros(N, device='cuda') for N, K in dims]
    ws = torch.zeros(1 << 24, device='cuda')
    arr = lambda ts: np.array([t.data_ptr() for t in ts], dtype=np.uint64)
    a_dy, a_x, a_dw, a_16, a_db = arr(dys), arr(xs), arr(dws), arr(d16), arr(dbs)
    Ns, Ks = np.array([d[0] for d in dims], dtype=np.int32), np.array([d[1] for d in dims], dtype=np.int32)
    refs = [dys[i][:M].float().t() @ xs[i][:M].float() for i in range(n)]
    for accumulate in (0, 1):
        lib.vitae_wgrad_group_bt(n, a_dy.ctypes.data, a_x.ctypes.data, a_dw.ctypes.data, a_16.ctypes.data, a_db.ctypes.data if not accumulate else None,
                                 Ns.ctypes.data, Ks.ctypes.data, M, Mp, accumulate, ws.data_ptr(), ws.numel(), st())
        for i in range(n):
            want = refs[i] * (2 if accumulate else 1)
            assert rel_err(dws[i], want) < 2e-5, (i, accumulate, rel_err(dws[i], want))
            assert torch.equal(d16[i], dws[i].to(torch.bfloat16))
            assert rel_err(dbs[i], dys[i][:M].float().sum(0)) < 1e-5
    assert float(ws[:4096].abs().max()) == 0.0          # the tickets are back to zero


def test_gemm_bt_planner_is_consistent(lib, bt_mode):
    """vitae_gemm_glds_pick_split_k returns the split of the plan the launcher will follow; forcing a tile changes the plan;
    -2 switches the family off."""
    bt_mode(-1)
    assert lib.vitae_gemm_glds_bt_choice(1, 1, 868, 16384, 512) == 0 and lib.vitae_gemm_glds_pick_split_k(868, 16384, 512) == 1
    assert lib.vitae_gemm_glds_bt_choice(1, 1, 440, 768, 768) == 5                  # a batch-4 encoder shape: the wave-specialised 64 x 64 tile
    assert lib.vitae_gemm_glds_bt_choice(1, 1, 3456, 768, 16384) == 3 and lib.vitae_gemm_glds_pick_split_k(3456, 768, 16384) > 1
    bt_mode(-2)
    assert lib.vitae_gemm_glds_bt_choice(1, 1, 868, 16384, 512) == -1
    bt_mode(3)
    assert lib.vitae_gemm_glds_bt_choice(1, 1, 868, 16384, 512) == 3
    with pytest.raises(Exception):
        lib.vitae_gemm_glds_set_bt_tile(1)


@pytest.mark.parametrize('B', [4, 8, 32])
def test_planner_pick_is_within_ten_percent_of_the_best_tile(lib, bt_mode, B):
    """the cost model of vitae_gemm_glds (csrc/gemm_glds.hip: bt_plan) against every tile family forced in turn, on the
    27 (shape, operand form) problems of the step at this batch — a cost-model regression fails a test instead of a profile.  Each
    candidate is timed as a graph of 20 back-to-back launches (best of 3); the pick may be 15 % (20 % on the 16384-deep reductions) + 1 us behind the best:
    profiles/round5_bt_forms_table.txt has 80 of 81 rows within 1.09, but two candidates 5 % apart swap places from box to box (a
    first bound of 10 % + 0.8 us failed one row in one of four full-suite runs), and a bound that flakes is worth less than a loose one."""
    Me, Md = B * 2 * 55, B * 217
    shapes = [('enc qkv', Me, 2304, 768), ('enc proj', Me, 768, 768), ('enc fc1', Me, 3072, 768), ('enc fc2', Me, 768, 3072),
              ('dec qkv', Md, 1536, 512), ('dec fc1', Md, 2048, 512), ('dec fc2', Md, 512, 2048), ('dec pred', Md, 16384, 512),
              ('patch embed', B * 2 * 54, 768, 16384)]
    ws = torch.zeros(1 << 24, device='cuda')

    def timed(akc, bkc, A, Bm, Cc, M, N, K, tile):
        bt_mode(tile)
        split = lib.vitae_gemm_glds_pick_split_k_form(akc, bkc, M, N, K)
        go = lambda: lib.vitae_gemm_glds(akc, bkc, A.data_ptr(), K if akc else M, Bm.data_ptr(), K if bkc else N, Cc.data_ptr(), N, None, 0, M, N, K,
                                         None, None, 0, 0, None, 0, 0, split, ws.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
        go(); torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(20):
                go()
        g.replay(); torch.cuda.synchronize()
        best = 1e9
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) / 20 * 1e3)
        return best

    bad = []
    for name, M0, N0, K0 in shapes:
        for form, (akc, bkc) in (('fwd', (1, 1)), ('dgrad', (1, 0)), ('wgrad', (0, 0))):
            M, N, K = (M0, N0, K0) if form == 'fwd' else (M0, K0, N0) if form == 'dgrad' else (N0, K0, (M0 + 63) // 64 * 64)
            A = torch.randn((M, K) if akc else (K, M), device='cuda').bfloat16()
            Bm = torch.randn((N, K) if bkc else (K, N), device='cuda').bfloat16()
            Cc = torch.empty(M, N, device='cuda')
            t = {tile: timed(akc, bkc, A, Bm, Cc, M, N, K, tile) for tile in ((6,) if form == 'wgrad' else ()) + (5, 4, 3, 0, -2, -1)}
            best = min(v for k, v in t.items() if k != -1)
            if t[-1] > (1.20 if K >= 8192 else 1.15) * best + 1.0:      # (16384-deep reductions stream their operand from HBM: both candidates' models are 2x low there)
                bad.append((name, form, round(t[-1], 1), round(best, 1), {k: round(v, 1) for k, v in t.items()}))
    bt_mode(-1)
    assert not bad, bad
