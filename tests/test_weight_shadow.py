"""bf16 weight shadows (ABI 57): ``vitae_ema_multi_shadow`` / ``vitae_lars_multi_shadow`` / ``vitae_adamw_multi_shadow`` and the slot
store of ``vit_ae_plus_plus_amd/shadow.py`` that the encoders and the three multi-tensor updaters share.

Every comparison in this file is bitwise; there is no tolerance anywhere.

Kernels (through the C ABI)
  * every fp32 output of a ``*_shadow`` call is compared with what the existing sibling entry point (unchanged, pinned by
    tests/test_moco_v3.py and tests/test_multi_adamw.py) writes from the same inputs at the same fp32 alignment — whole buffers,
    padding included;
  * every listed shadow is compared with ``vitae_cast_bf16`` (its rounding is pinned by tests/test_gemm_kernels.py) of the updated fp32
    tensor; 8 bf16 of a guard pattern before and after every shadow, and the whole would-be shadow of an entry listed as 0, stay;
  * lengths 1, 3, 4, 5, chunk - 1, chunk, chunk + 1, 2 chunk + 1 as one-tensor tables, and a five-tensor table whose entries 1 and 3
    list no shadow; four alignments: all aligned, fp32 one float off (element path), shadow 2 bytes off (element path against the
    sibling's 16-byte path), shadow 8 bytes off an aligned base (16-byte path with 8-byte shadow stores);
  * inputs carry NaN, +-inf, -0.0, fp32 denormals and values on bf16 ties.  Where they sit the gradient (and the optimiser state) is 0,
    so that an unscaled LARS tensor and an undecayed AdamW tensor hand them through to the shadow conversion unchanged; the EMA carries
    them in ``pb`` (m = 0 passes ``pb`` through).  No operation sees two NaNs, so no result depends on which payload an instruction keeps.

Models (micro encoder of the act16 tests: volume 8, patch 4, 1 channel, embed 64, depth 2, 2 heads, bf16 / bf16)
  ``vitae_cast_bf16`` calls are counted by wrapping the binding inside the test.  1 + 4 depth = 9 weights per encoder go through
  ``_bf16``: a MoCo step with ``VITAE_WEIGHT_SHADOW=0`` casts 2 x 9 = 18 times (the parent's count at every step: there each updater's
  ``increment_version`` invalidates every copy), a fine-tuning step 9 times; with the switch on, every step after the first casts nothing.
"""
import copy
import gc
from functools import partial

import numpy as np
import pytest
import torch

GUARD = 8                      # bf16 elements of guard pattern on both sides of a shadow
PATTERN = 0x5A5A               # what shadows and their guards hold before a call (as 16-bit words)
SENT32 = 12345.5               # padding of the fp32 buffers
gpu = pytest.mark.gpu


def _consts():
    from vit_ae_plus_plus_amd._abi import CONSTS
    return CONSTS


def _chunk():
    return int(_consts()['VITAE_MULTI_CHUNK'])


# =========================================================================== CPU
def test_header_binding_and_library_agree_on_abi_57():
    from vit_ae_plus_plus_amd._abi import CONSTS, PROTOS, lib
    assert CONSTS['VITAE_ABI_VERSION'] == 57
    dll = lib.load()
    assert dll.vitae_abi_version() == 57
    tail = ['ptr', 'ptr', 'ptr']           # shadow_host, shadow_dev, stream
    for name in ('vitae_ema_multi', 'vitae_lars_multi', 'vitae_adamw_multi'):
        ret, kinds = PROTOS[name]
        ret_s, kinds_s = PROTOS[name + '_shadow']
        assert ret_s == ret == 'int' and kinds_s == kinds[:-1] + tail, name          # the sibling's arguments, two arrays before stream
        assert getattr(dll, name + '_shadow') is not None


def test_shadow_column_lists_current_slots_only_and_leaves_the_entries_alone(monkeypatch):
    from vit_ae_plus_plus_amd import shadow
    from vit_ae_plus_plus_amd.optim import multi_table
    monkeypatch.delenv('VITAE_WEIGHT_SHADOW', raising=False)
    ps = [torch.nn.Parameter(torch.ones(n)) for n in (4, 4, 7, 3, 5)]          # ps[0] and ps[1] are equal by value
    store = shadow.ShadowStore()
    assert shadow.shadow_column(ps) == (None, [])                              # no slot anywhere: no column
    s0, s2, s4 = store.slot(ps[0]), store.slot(ps[2]), store.slot(ps[4])
    assert shadow.slot_for(ps[1]) is None and shadow.slot_for(ps[0]) is s0 and store.slot(ps[0]) is s0
    assert not s0.current()                                                    # made, never written
    for s in (s0, s2, s4):
        s.mark()
    with torch.no_grad():
        ps[2].add_(1.0)                                                        # version bump: stale
    col, listed = shadow.shadow_column(ps)
    assert col.dtype == np.int64 and col.tolist() == [s0.address(), 0, 0, 0, s4.address()] and listed == [s0, s4]
    ew = _consts()['VITAE_MULTI_ENTRY_WORDS']
    table = multi_table(*[[100 * k + i for i in range(5)] for k in range(1, 5)], [p.numel() for p in ps], [0, 1, 0, 1, 0])
    hyper = [1e-3, 5e-4, 0.05, 0.0, 0.25]                                      # an odd count: padded to whole words
    plain, with_col = shadow.pack_words(table, hyper), shadow.pack_words(table, hyper, col)
    assert ew == 6 and plain.dtype == with_col.dtype == np.int64
    assert np.array_equal(plain[:5 * ew].reshape(5, ew), table) and np.array_equal(with_col[:plain.size], plain)
    assert np.array_equal(plain[5 * ew:].view(np.float32)[:5], np.asarray(hyper, dtype=np.float32)) and plain.size == 5 * ew + 3
    assert with_col[plain.size:].tolist() == col.tolist()
    with pytest.raises(ValueError):
        shadow.pack_words(table, hyper, col[:4])
    # a moved parameter (another data_ptr) is stale; the switch lists nothing, read at call time
    ps[0].data = torch.ones(4)
    assert not s0.current() and shadow.shadow_column(ps)[0].tolist() == [0, 0, 0, 0, s4.address()]
    monkeypatch.setenv('VITAE_WEIGHT_SHADOW', '0')
    assert shadow.shadow_column(ps) == (None, [])
    monkeypatch.setenv('VITAE_WEIGHT_SHADOW', '1')
    assert shadow.shadow_column(ps)[1] == [s4]
    # identity, not value; copies get no slot; nothing keeps a parameter alive; drop() detaches
    q = copy.deepcopy(ps[4])
    assert shadow.slot_for(q) is None
    setattr(q, shadow._ATTR, s4)                                               # even a copy that carried the attribute along is not the owner
    assert shadow.slot_for(q) is None and store.slot(q) is not s4
    owner = s2.owner
    del ps[2]
    gc.collect()
    assert owner() is None and s2 not in store.slots()
    store.drop()
    assert shadow.slot_for(ps[0]) is None and store.slots() == []


# =========================================================================== GPU plumbing
def dev():
    return torch.device('cuda')


def stream():
    return torch.cuda.current_stream().cuda_stream


def raw(name):
    """the entry point without the status check (to read refusal codes)"""
    from vit_ae_plus_plus_amd._abi import lib
    return getattr(lib.load(), name)


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def same(a, b):
    return a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


HARD = [0x7FC00000, 0x7F800000, 0xFF800000]                                   # NaN, +inf, -inf
SOFT = [0x80000000, 0x00000001, 0x007FFFFF, 0x80000400,                       # -0.0, denormals
        0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,                       # ties: to even downwards, to even upwards, both signs
        0x7F7F8000, 0x00008000, 0x00018000, 0x3F807FFF, 0x3F808001]           # a tie that rounds to inf, denormal ties, either side of a tie


def values(n, rng, hard, scale=0.05):
    """n floats: random, the first min(n, .) of them special values (rotated by n, so that short tensors see different ones)"""
    a = (rng.standard_normal(n) * scale).astype(np.float32)
    sp = (HARD if hard else []) + SOFT
    k = min(n, len(sp))
    a.view(np.uint32)[:k] = [sp[(j + n) % len(sp)] for j in range(k)]
    return a, k


class F32:
    """n floats on the device, ``off`` floats away from 16-byte alignment, padding on both sides of it"""

    def __init__(self, data, off):
        data = np.ascontiguousarray(data, dtype=np.float32).reshape(-1)
        self.n, self.off = data.size, off
        host = np.full(4 + off + data.size + 4, SENT32, dtype=np.float32)
        host[4 + off:4 + off + data.size] = data
        self.buf = torch.from_numpy(host).to(dev())
        assert self.buf.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * (4 + self.off)

    def set(self, data):
        self.buf[4 + self.off:4 + self.off + self.n] = torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)).to(dev())

    def aligned_copy(self):
        return self.buf[4 + self.off:4 + self.off + self.n].clone()


class Shadow:
    """n bf16 on the device between GUARD-element guards, ``off`` bf16 elements (2 bytes each) away from 16-byte alignment; everything
    starts as PATTERN"""

    def __init__(self, n, off):
        self.n, self.off = n, off
        self.buf = torch.full((GUARD + off + n + GUARD,), PATTERN, dtype=torch.int16, device=dev())
        assert self.buf.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + 2 * (GUARD + self.off)

    def data(self):
        return self.buf[GUARD + self.off:GUARD + self.off + self.n]

    def guards_intact(self):
        lo = GUARD + self.off
        return bool((self.buf[:lo] == PATTERN).all()) and bool((self.buf[lo + self.n:] == PATTERN).all())

    def untouched(self):
        return bool((self.buf == PATTERN).all())


def cast_reference(f32):
    """vitae_cast_bf16 of the tensor's current values, from an aligned copy into an aligned destination, as 16-bit words"""
    src = f32.aligned_copy()
    dst = torch.full((f32.n,), PATTERN, dtype=torch.int16, device=dev())
    assert raw('vitae_cast_bf16')(src.data_ptr(), dst.data_ptr(), f32.n, stream()) == 0
    return dst


class Upload:
    """host and device copies of a table, its chunk list, hyper-parameters and (optionally) a shadow column"""

    def __init__(self, table, lengths, hyper=(), column=None):
        from vit_ae_plus_plus_amd.optim import multi_chunk_list
        self.table = np.ascontiguousarray(table, dtype=np.int64)
        self.chunks = np.ascontiguousarray(multi_chunk_list(lengths, _chunk()))
        self.table_d = torch.from_numpy(self.table).to(dev())
        self.chunks_d = torch.from_numpy(self.chunks).to(dev())
        self.hyper_d = torch.tensor(list(hyper) or [0.0], dtype=torch.float32, device=dev())
        self.column = None if column is None else np.ascontiguousarray(column, dtype=np.int64)
        self.column_d = None if column is None else torch.from_numpy(self.column).to(dev())

    def args(self):
        return (self.table.ctypes.data, self.table_d.data_ptr(), len(self.table), self.chunks.ctypes.data, self.chunks_d.data_ptr(),
                len(self.chunks), _chunk())

    def shadow_args(self):
        return (None, None) if self.column is None else (self.column.ctypes.data, self.column_d.data_ptr())


def tables():
    c = _chunk()
    return [[n] for n in (1, 3, 4, 5, c - 1, c, c + 1, 2 * c + 1)] + [[c + 1, 4, 2 * c + 1, c - 1, 5]]


def listed_entries(lengths):
    return [0, 2, 4] if len(lengths) == 5 else list(range(len(lengths)))          # entries 1 and 3 of the five list no shadow


ALIGN = {'aligned': (0, 0), 'fp32_one_float_off': (1, 0), 'shadow_2_bytes_off': (0, 1), 'shadow_8_bytes_off': (0, 4)}


def make_shadows(lengths, s_off):
    sh = [Shadow(n, s_off) for n in lengths]
    lst = listed_entries(lengths)
    col = np.array([sh[t].ptr if t in lst else 0 for t in range(len(lengths))], dtype=np.int64)
    if s_off == 0:
        assert all(sh[t].ptr % 16 == 0 for t in lst)
    elif s_off == 1:
        assert all(sh[t].ptr % 4 == 2 for t in lst)
    else:
        assert all(sh[t].ptr % 16 == 8 for t in lst)
    return sh, col, lst


def check_shadows(sh, lst, updated, label):
    """listed shadows == vitae_cast_bf16(updated tensor), guards intact; the would-be shadows of the other entries untouched"""
    torch.cuda.synchronize()
    for t, s in enumerate(sh):
        if t in lst:
            assert same(s.data(), cast_reference(updated[t])), (label, t, s.n)
            assert s.guards_intact(), (label, t, s.n)
        else:
            assert s.untouched(), (label, t, s.n)


def assert_same_buffers(a_lists, b_lists, label):
    for k, (al, bl) in enumerate(zip(a_lists, b_lists)):
        for t, (a, b) in enumerate(zip(al, bl)):
            assert same(a.buf, b.buf), (label, 'output list', k, 'tensor', t)


# =========================================================================== EMA
def ema_inputs(lengths, seed):
    rng = np.random.default_rng(seed)
    pms, pbs = [], []
    for n in lengths:
        pm = values(n, rng, hard=False)[0][::-1].copy()          # its special values at the end, away from those of pb (longer tensors)
        pms.append(pm)
        pbs.append(values(n, rng, hard=True)[0])                 # NaN, infinities and the ties in pb: m = 0 passes them through
    return pms, pbs


def ema_run(lengths, pms, pbs, m, f_off, column, entry):
    gm, gb = [F32(a, f_off) for a in pms], [F32(a, f_off) for a in pbs]
    table = np.zeros((len(lengths), 6), dtype=np.int64)
    table[:, 0], table[:, 1], table[:, 4] = [x.ptr for x in gm], [x.ptr for x in gb], lengths
    up = Upload(table, lengths, column=column)
    if entry == 'sibling':
        rc = raw('vitae_ema_multi')(*up.args(), float(m), stream())
    else:
        rc = raw('vitae_ema_multi_shadow')(*up.args(), float(m), *up.shadow_args(), stream())
    assert rc == 0
    torch.cuda.synchronize()
    return gm, gb


@gpu
@pytest.mark.parametrize('m', [0.0, 0.5, 0.99, 1.0])
@pytest.mark.parametrize('align', list(ALIGN))
def test_ema_shadow(align, m):
    f_off, s_off = ALIGN[align]
    for i, lengths in enumerate(tables()):
        pms, pbs = ema_inputs(lengths, seed=i)
        sh, col, lst = make_shadows(lengths, s_off)
        want = ema_run(lengths, pms, pbs, m, f_off, None, 'sibling')
        got = ema_run(lengths, pms, pbs, m, f_off, col, 'shadow')
        assert_same_buffers(want, got, ('ema', align, m, lengths))
        check_shadows(sh, lst, got[0], ('ema', align, m))
        if m == 0.0:      # pm * 0 + pb: pb itself wherever it is not a zero (whose sign the sum decides), so the ties of pb reach the conversion
            for t in lst:
                keep = torch.from_numpy(pbs[t] != 0).to(dev())
                assert same(sh[t].data()[keep], cast_reference(F32(pbs[t], 0))[keep]), (align, lengths, t)
        if m == 1.0:      # pm + pb * 0: NaN wherever pb is not finite (pm itself elsewhere: judged by the sibling above)
            for t in range(len(lengths)):
                wild = torch.from_numpy(~np.isfinite(pbs[t])).to(dev())
                assert bool(torch.isnan(got[0][t].aligned_copy()[wild]).all()), (align, lengths, t)


# =========================================================================== LARS
LARS_HYPER = [0.3, 0.05, 1e-2, 0.0, 0.9, 0.8, 0.001, 0.002]          # lr, weight_decay, momentum, trust_coefficient of two groups


def lars_inputs(lengths, seed, steps=3):
    """per tensor: p, scaled; per step: gradients.  Unscaled tensors carry NaN / inf; every special value meets a zero gradient, so an
    unscaled tensor keeps it (p - lr (momentum 0 + 0)) and hands it to the shadow conversion.  Entry 0 of the five is the |p| = 0 tensor."""
    rng = np.random.default_rng(100 + seed)
    ps, scaled, ks = [], [], []
    for t, n in enumerate(lengths):
        sc = (t in (0, 2, 3)) if len(lengths) > 1 else bool(seed % 2)
        p, k = values(n, rng, hard=not sc)
        if len(lengths) > 1 and t == 0:
            p, k = np.zeros(n, dtype=np.float32), 0
        ps.append(p); scaled.append(sc); ks.append(k)
    grads = []
    for s in range(steps):
        gs = []
        for n, k in zip(lengths, ks):
            g = (rng.standard_normal(n) * 0.01).astype(np.float32)
            g[:k] = 0
            gs.append(g)
        grads.append(gs)
    return ps, scaled, grads


def lars_run(lengths, ps, scaled, grads, f_off, column, entry, after_step=None):
    gp = [F32(p, f_off) for p in ps]
    gmu = [F32(np.zeros_like(p), f_off) for p in ps]
    gg = [F32(np.zeros_like(p), f_off) for p in ps]
    table = np.zeros((len(lengths), 6), dtype=np.int64)
    table[:, 0], table[:, 1], table[:, 2] = [x.ptr for x in gp], [x.ptr for x in gg], [x.ptr for x in gmu]
    table[:, 3], table[:, 4], table[:, 5] = [int(s) for s in scaled], lengths, [t % 2 for t in range(len(lengths))]
    up = Upload(table, lengths, LARS_HYPER, column)
    ws = torch.full((2 * len(up.chunks) + 2,), float('nan'), dtype=torch.float64, device=dev())
    for step, gs in enumerate(grads):
        for x, g in zip(gg, gs):
            x.set(g)
        if entry == 'sibling':
            rc = raw('vitae_lars_multi')(*up.args(), up.hyper_d.data_ptr(), 2, ws.data_ptr(), stream())
        else:
            rc = raw('vitae_lars_multi_shadow')(*up.args(), up.hyper_d.data_ptr(), 2, ws.data_ptr(), *up.shadow_args(), stream())
        assert rc == 0
        torch.cuda.synchronize()
        if after_step:
            after_step(step, gp)
    assert bool(torch.isnan(ws[-2:]).all())
    return gp, gmu


@gpu
@pytest.mark.parametrize('align', list(ALIGN))
def test_lars_shadow_over_three_steps(align):
    f_off, s_off = ALIGN[align]
    for i, lengths in enumerate(tables()):
        ps, scaled, grads = lars_inputs(lengths, seed=i)
        sh, col, lst = make_shadows(lengths, s_off)
        want = lars_run(lengths, ps, scaled, grads, f_off, None, 'sibling')
        got = lars_run(lengths, ps, scaled, grads, f_off, col, 'shadow',
                       after_step=lambda step, gp: check_shadows(sh, lst, gp, ('lars', align, lengths, step)))
        assert_same_buffers(want, got, ('lars', align, lengths))
        again = lars_run(lengths, ps, scaled, grads, f_off, col, 'shadow')
        assert_same_buffers(got, again, ('lars repeat', align, lengths))
        for t in lst:           # an unscaled tensor kept its special values, so the shadow saw NaN, infinities and ties
            if not scaled[t]:
                k = min(lengths[t], len(HARD) + len(SOFT))
                assert np.array_equal(got[0][t].aligned_copy().cpu().numpy()[:k].view(np.uint32), ps[t][:k].view(np.uint32))


# =========================================================================== AdamW
ADAMW_HYPER = [1e-3, 5e-4, 0.05, 0.0]          # lr of two groups, weight_decay of two groups
BETAS, EPS = (0.9, 0.95), 1e-8


def adamw_inputs(lengths, seed, steps=3):
    rng = np.random.default_rng(200 + seed)
    ps, ms, vs, ks = [], [], [], []
    for n in lengths:
        p, k = values(n, rng, hard=True)
        m, v = (rng.standard_normal(n) * 0.01).astype(np.float32), (rng.standard_normal(n) ** 2 * 1e-4).astype(np.float32)
        m[:k] = 0; v[:k] = 0          # with a zero gradient: the update of a special value is p * (1 - lr wd), p itself where wd = 0
        ps.append(p); ms.append(m); vs.append(v); ks.append(k)
    grads = []
    for s in range(steps):
        gs = []
        for n, k in zip(lengths, ks):
            g = (rng.standard_normal(n) * 0.01).astype(np.float32)
            g[:k] = 0
            gs.append(g)
        grads.append(gs)
    return ps, ms, vs, grads


class AdamwList:
    def __init__(self, lengths, ps, ms, vs, f_off, column, group0=0):
        self.p, self.m, self.v = ([F32(a, f_off) for a in k] for k in (ps, ms, vs))
        self.g = [F32(np.zeros_like(a), f_off) for a in ps]
        table = np.zeros((len(lengths), 6), dtype=np.int64)
        for c, k in enumerate((self.p, self.g, self.m, self.v)):
            table[:, c] = [x.ptr for x in k]
        table[:, 4], table[:, 5] = lengths, [(t + group0) % 2 for t in range(len(lengths))]
        self.up = Upload(table, lengths, ADAMW_HYPER, column)
        C = _consts()
        self.state = torch.zeros(C['VITAE_MULTI_STATE_COUNT'], dtype=torch.float32, device=dev())
        self.acc = torch.zeros(C['VITAE_ACC_COUNT'], dtype=torch.float64, device=dev())
        self.norm = torch.full((3,), 99.0, dtype=torch.float32, device=dev())

    def tail(self, max_norm):
        hd = self.up.hyper_d.data_ptr()
        return (hd, hd + 8, 2, BETAS[0], BETAS[1], EPS, float(max_norm), self.state.data_ptr(), self.acc.data_ptr(), self.norm.data_ptr() + 4)

    def step(self, gs, max_norm, entry):
        for x, g in zip(self.g, gs):
            x.set(g)
        assert raw('vitae_grad_sqnorm_multi')(*self.up.args(), self.acc.data_ptr(), stream()) == 0
        if entry == 'sibling':
            rc = raw('vitae_adamw_multi')(*self.up.args(), *self.tail(max_norm), stream())
        else:
            rc = raw('vitae_adamw_multi_shadow')(*self.up.args(), *self.tail(max_norm), *self.up.shadow_args(), stream())
        assert rc == 0
        torch.cuda.synchronize()

    def outputs(self):
        return [self.p, self.m, self.v]

    def scalars(self):
        return [self.state, self.acc, self.norm]


@gpu
@pytest.mark.parametrize('max_norm', [0.0, 0.05])
@pytest.mark.parametrize('align', list(ALIGN))
def test_adamw_shadow_over_three_steps(align, max_norm):
    f_off, s_off = ALIGN[align]
    for i, lengths in enumerate(tables()):
        ps, ms, vs, grads = adamw_inputs(lengths, seed=i)
        sh, col, lst = make_shadows(lengths, s_off)
        want = AdamwList(lengths, ps, ms, vs, f_off, None, group0=i)
        got = AdamwList(lengths, ps, ms, vs, f_off, col, group0=i)
        for step, gs in enumerate(grads):
            want.step(gs, max_norm, 'sibling')
            got.step(gs, max_norm, 'shadow')
            check_shadows(sh, lst, got.p, ('adamw', align, max_norm, lengths, step))
        assert_same_buffers(want.outputs(), got.outputs(), ('adamw', align, max_norm, lengths))
        assert all(same(a, b) for a, b in zip(want.scalars(), got.scalars())), (align, max_norm, lengths)
        C = _consts()
        assert float(got.state[C['VITAE_MULTI_STATE_STEP']]) == 3.0 and float(got.state[C['VITAE_MULTI_STATE_SKIPPED']]) == 0.0
        assert float(got.norm[0]) == 99.0 and float(got.norm[2]) == 99.0
        if max_norm and sum(lengths) > 1000:
            assert float(got.norm[1]) > max_norm          # the clipping factor was in force
        for t in lst:           # an undecayed tensor kept its special values
            if (t + i) % 2 == 1:
                k = min(lengths[t], len(HARD) + len(SOFT))
                assert np.array_equal(got.p[t].aligned_copy().cpu().numpy()[:k].view(np.uint32), ps[t][:k].view(np.uint32))


@gpu
@pytest.mark.parametrize('align', ['aligned', 'shadow_2_bytes_off'])
def test_adamw_shadow_non_finite_gradient_writes_nothing(align):
    f_off, s_off = ALIGN[align]
    lengths = tables()[-1]
    ps, ms, vs, grads = adamw_inputs(lengths, seed=7, steps=2)
    sh, col, lst = make_shadows(lengths, s_off)
    d = AdamwList(lengths, ps, ms, vs, f_off, col)
    d.step(grads[0], 0.0, 'shadow')
    check_shadows(sh, lst, d.p, 'before the skipped step')
    for s in sh:                # a pattern of their own: a rewrite with the same values would show
        s.buf.fill_(0x1234)
    before = [x.buf.clone() for k in d.outputs() for x in k]
    bad = [g.copy() for g in grads[1]]
    bad[2][lengths[2] // 2] = np.inf
    d.step(bad, 0.0, 'shadow')
    C = _consts()
    assert all(same(a, x.buf) for a, x in zip(before, [x for k in d.outputs() for x in k]))
    assert all(bool((s.buf == 0x1234).all()) for s in sh)
    assert float(d.state[C['VITAE_MULTI_STATE_STEP']]) == 1.0 and float(d.state[C['VITAE_MULTI_STATE_SKIPPED']]) == 1.0
    assert float(d.norm[1]) == float('inf') and float(d.acc.abs().sum()) == 0.0


# =========================================================================== refusals, and the call without a column
@gpu
def test_refusals_write_nothing_and_no_column_is_the_sibling():
    lengths = [_chunk() + 1, 5]
    sh, col, lst = make_shadows(lengths, 0)
    odd = col.copy(); odd[1] += 1
    up_odd = Upload(np.zeros((2, 6), dtype=np.int64), lengths, column=odd)
    # --- EMA
    pms, pbs = ema_inputs(lengths, seed=3)
    gm, gb = [F32(a, 0) for a in pms], [F32(a, 0) for a in pbs]
    table = np.zeros((2, 6), dtype=np.int64)
    table[:, 0], table[:, 1], table[:, 4] = [x.ptr for x in gm], [x.ptr for x in gb], lengths
    up = Upload(table, lengths, column=col)
    fn = raw('vitae_ema_multi_shadow')
    snap = [x.buf.clone() for x in gm]
    sa = up.shadow_args()
    assert fn(*up.args(), 0.5, sa[0], None, stream()) == -1 and fn(*up.args(), 0.5, None, sa[1], stream()) == -1
    assert fn(*up.args(), 0.5, *up_odd.shadow_args(), stream()) == -1
    assert fn(*up.args()[:6], 6, 0.5, *sa, stream()) == -1 and fn(*up.args(), 1.5, *sa, stream()) == -1          # the sibling's refusals
    torch.cuda.synchronize()
    assert all(same(a, x.buf) for a, x in zip(snap, gm)) and all(s.untouched() for s in sh)
    want = ema_run(lengths, pms, pbs, 0.5, 0, None, 'sibling')
    got = ema_run(lengths, pms, pbs, 0.5, 0, None, 'shadow')           # both arrays NULL
    assert_same_buffers(want, got, 'ema without a column')
    # --- LARS
    ps, scaled, grads = lars_inputs(lengths, seed=3, steps=1)
    gp, gmu, gg = [F32(p, 0) for p in ps], [F32(np.zeros_like(p), 0) for p in ps], [F32(g, 0) for g in grads[0]]
    table = np.zeros((2, 6), dtype=np.int64)
    table[:, 0], table[:, 1], table[:, 2] = [x.ptr for x in gp], [x.ptr for x in gg], [x.ptr for x in gmu]
    table[:, 3], table[:, 4] = [1, 0], lengths
    up = Upload(table, lengths, LARS_HYPER, col)
    ws = torch.full((2 * len(up.chunks),), float('nan'), dtype=torch.float64, device=dev())
    fn = raw('vitae_lars_multi_shadow')
    snap = [x.buf.clone() for x in gp + gmu]
    sa, hd = up.shadow_args(), up.hyper_d.data_ptr()
    assert fn(*up.args(), hd, 2, ws.data_ptr(), sa[0], None, stream()) == -1
    assert fn(*up.args(), hd, 2, ws.data_ptr(), None, sa[1], stream()) == -1
    assert fn(*up.args(), hd, 2, ws.data_ptr(), *up_odd.shadow_args(), stream()) == -1
    assert fn(*up.args(), hd, 0, ws.data_ptr(), *sa, stream()) == -1 and fn(*up.args(), hd, 2, None, *sa, stream()) == -1
    torch.cuda.synchronize()
    assert all(same(a, x.buf) for a, x in zip(snap, gp + gmu)) and all(s.untouched() for s in sh) and bool(torch.isnan(ws).all())
    want = lars_run(lengths, ps, scaled, grads, 0, None, 'sibling')
    got = lars_run(lengths, ps, scaled, grads, 0, None, 'shadow')
    assert_same_buffers(want, got, 'lars without a column')
    # --- AdamW
    ps, ms, vs, grads = adamw_inputs(lengths, seed=3, steps=1)
    d = AdamwList(lengths, ps, ms, vs, 0, col)
    for x, g in zip(d.g, grads[0]):
        x.set(g)
    fn = raw('vitae_adamw_multi_shadow')
    snap = [x.buf.clone() for k in d.outputs() for x in k] + [t.clone() for t in d.scalars()]
    sa = d.up.shadow_args()
    assert fn(*d.up.args(), *d.tail(0.0), sa[0], None, stream()) == -1 and fn(*d.up.args(), *d.tail(0.0), None, sa[1], stream()) == -1
    assert fn(*d.up.args(), *d.tail(0.0), *up_odd.shadow_args(), stream()) == -1
    no_state = list(d.tail(0.0)); no_state[7] = None
    assert fn(*d.up.args(), *no_state, *sa, stream()) == -1 and fn(*d.up.args()[:6], 1022, *d.tail(0.0), *sa, stream()) == -1
    torch.cuda.synchronize()
    assert all(same(a, b) for a, b in zip(snap, [x.buf for k in d.outputs() for x in k] + d.scalars())) and all(s.untouched() for s in sh)
    want, got = AdamwList(lengths, ps, ms, vs, 0, None), AdamwList(lengths, ps, ms, vs, 0, None)
    want.step(grads[0], 0.05, 'sibling')
    got.step(grads[0], 0.05, 'shadow')
    assert_same_buffers(want.outputs(), got.outputs(), 'adamw without a column')
    assert all(same(a, b) for a, b in zip(want.scalars(), got.scalars()))


# =========================================================================== models
ENC = dict(volume_size=8, patch_size=4, in_chans=1, embed_dim=64, depth=2, num_heads=2, precision='bf16', activations='bf16')
WEIGHTS = 1 + 4 * ENC['depth']          # what goes through HipEncoder._bf16: the patch embedding and four Linear weights per block


class CastCounter:
    """wraps the binding of vitae_cast_bf16 (``lib`` is the object encoder.py calls through) and counts the calls"""

    def __init__(self, monkeypatch):
        from vit_ae_plus_plus_amd._abi import lib
        inner = lib.vitae_cast_bf16
        self.n = 0

        def counted(*a):
            self.n += 1
            return inner(*a)

        monkeypatch.setattr(lib, 'vitae_cast_bf16', counted)

    def take(self):
        n, self.n = self.n, 0
        return n


def vit(num_classes=3, seed=0):
    from vit_ae_plus_plus_amd.model.vit import VisionTransformer3D
    torch.manual_seed(seed)
    m = VisionTransformer3D(num_classes=num_classes, **ENC)
    torch.nn.init.normal_(m.head.weight, std=0.1)          # (the constructor zeroes the head: no gradient would reach the encoder)
    return m.cuda().train()


def loss_of(model, x):
    return (model(x) - 1.0).square().mean()


def volumes(B, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 1, 8, 8, 8, generator=g).cuda()


def assert_slots_hold_their_parameters(module, label):
    """every slot of the model's store is current and holds, bit for bit, vitae_cast_bf16 of its parameter"""
    from vit_ae_plus_plus_amd import shadow
    slots = shadow.store_of(module).slots()
    assert len(slots) == WEIGHTS, (label, len(slots))
    torch.cuda.synchronize()
    for s in slots:
        p = s.owner()
        assert s.current() and shadow.slot_for(p) is s, label
        want = torch.empty(p.numel(), dtype=torch.bfloat16, device=p.device)
        assert raw('vitae_cast_bf16')(p.data_ptr(), want.data_ptr(), p.numel(), stream()) == 0
        assert same(s.data.view(torch.int16), want.view(torch.int16)), label


def fresh_features(model, x):
    """features of a newly built model that loaded the same state dict (its own slots, cast from the fp32 weights)"""
    from vit_ae_plus_plus_amd.model.vit import VisionTransformer3D
    m = VisionTransformer3D(num_classes=model.num_classes, **ENC)
    m.load_state_dict({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
    return m.cuda().eval().forward_features(x)


def eval_features(model, x):
    was = model.training
    f = model.eval().forward_features(x)
    model.train(was)
    return f


@gpu
@pytest.mark.parametrize('switch', ['1', '0'])
def test_moco_lars_steps_cast_nothing_after_the_first(monkeypatch, switch):
    from vit_ae_plus_plus_amd.model.vit import VisionTransformer3D
    from vit_ae_plus_plus_amd.other_baselines.mocov3.moco.builder import MoCo_ViT
    from vit_ae_plus_plus_amd.other_baselines.mocov3.moco.optimizer import LARS
    monkeypatch.setenv('VITAE_WEIGHT_SHADOW', switch)
    torch.manual_seed(0)
    model = MoCo_ViT(partial(VisionTransformer3D, **ENC), 32, 64, 1.0).cuda().train()
    opt = LARS(model.parameters(), 0.3, weight_decay=1e-6, momentum=0.9)
    x1, x2 = volumes(2, 1), volumes(2, 2)
    casts = CastCounter(monkeypatch)
    per_step = []
    for step in range(4):
        opt.zero_grad()
        model(x1, x2, 0.99).backward()
        opt.step()
        per_step.append(casts.take())
        if switch == '1':
            for enc in (model.base_encoder, model.momentum_encoder):
                assert_slots_hold_their_parameters(enc, ('moco', step))
    # off: the parent's count — every weight of both encoders is cast again after each LARS step and each momentum update
    assert per_step == ([2 * WEIGHTS, 0, 0, 0] if switch == '1' else [2 * WEIGHTS] * 4), per_step


@gpu
@pytest.mark.parametrize('switch', ['1', '0'])
def test_finetune_adamw_steps_cast_nothing_after_the_first(monkeypatch, switch):
    from vit_ae_plus_plus_amd import shadow
    from vit_ae_plus_plus_amd.optim import MultiTensorAdamW
    monkeypatch.setenv('VITAE_WEIGHT_SHADOW', switch)
    model = vit()
    opt = MultiTensorAdamW(model.parameters(), lr=1e-3, weight_decay=0.05)
    x = volumes(2)
    casts = CastCounter(monkeypatch)
    per_step = []
    for step in range(4):
        opt.zero_grad()
        loss_of(model, x).backward()
        opt.norm_clip_step(1.0)
        per_step.append(casts.take())
        if switch == '1':
            assert_slots_hold_their_parameters(model, ('finetune', step))
    assert per_step == ([WEIGHTS, 0, 0, 0] if switch == '1' else [WEIGHTS] * 4), per_step
    assert opt.applied_steps() == 4 and opt.skipped_steps() == 0
    # evaluate() after the epoch: the inference encoder reads the trainer's slots — one store per model
    f = eval_features(model, x)
    assert casts.take() == (0 if switch == '1' else WEIGHTS)
    assert model._trainer is not None and model._encoder is not None and len(shadow.store_of(model).slots()) == WEIGHTS
    assert same(f, fresh_features(model, x))
    # set_precision drops the store with the encoders
    slot = shadow.slot_for(model.patch_embed.proj.weight)
    assert slot is not None
    model.set_precision('bf16')
    assert model._shadow is None and shadow.slot_for(model.patch_embed.proj.weight) is None


@gpu
def test_every_other_way_to_write_a_weight_costs_its_cast(monkeypatch):
    from vit_ae_plus_plus_amd.optim import MultiTensorAdamW
    monkeypatch.setenv('VITAE_WEIGHT_SHADOW', '1')
    model = vit()
    opt = MultiTensorAdamW(model.parameters(), lr=1e-3)
    x = volumes(2)
    casts = CastCounter(monkeypatch)

    def train_step(optimizer):
        optimizer.zero_grad()
        loss_of(model, x).backward()
        optimizer.step()

    def judge(expected, label):
        casts.take()
        f = eval_features(model, x)
        assert casts.take() == expected, label
        assert same(f, fresh_features(model, x)), label
        assert_slots_hold_their_parameters(model, label)

    train_step(opt)
    train_step(opt)
    judge(0, 'after two fused steps')
    # load_state_dict
    sd = {k: (v.detach().clone() * 1.25 if v.is_floating_point() else v.clone()) for k, v in model.state_dict().items()}
    model.load_state_dict(sd)
    judge(WEIGHTS, 'load_state_dict')
    # a no-grad in-place edit of one weight
    with torch.no_grad():
        model.blocks[1].mlp.fc1.weight.mul_(0.5)
    judge(1, 'in-place edit')
    # an optimiser of torch's
    tadam = torch.optim.AdamW(model.parameters(), lr=1e-3)
    train_step(tadam)
    judge(WEIGHTS, 'torch.optim.AdamW')
    # load_state_dict, then a fused step with no forward between: the updater lists no stale slot, so the next forward casts them all
    opt.zero_grad()
    loss_of(model, x).backward()
    model.load_state_dict(sd)
    opt.step()
    judge(WEIGHTS, 'load_state_dict + fused step')
    train_step(opt)
    judge(0, 'and a fused step after a forward keeps them current again')


@gpu
def test_skipped_step_keeps_weights_slots_and_features(monkeypatch):
    from vit_ae_plus_plus_amd.optim import MultiTensorAdamW
    monkeypatch.setenv('VITAE_WEIGHT_SHADOW', '1')
    model = vit()
    opt = MultiTensorAdamW(model.parameters(), lr=1e-3)
    x = volumes(2)
    casts = CastCounter(monkeypatch)
    opt.zero_grad()
    loss_of(model, x).backward()
    opt.step()
    opt.zero_grad()
    loss_of(model, x).backward()
    model.blocks[0].attn.qkv.weight.grad[3, 5] = float('inf')
    before = eval_features(model, x)
    casts.take()
    norm = opt.norm_clip_step(1.0)
    after = eval_features(model, x)
    assert casts.take() == 0
    assert not bool(torch.isfinite(norm)) and opt.skipped_steps() == 1 and opt.applied_steps() == 1
    assert same(before, after)
    assert_slots_hold_their_parameters(model, 'after a skipped step')


@gpu
def test_frozen_backbone_head_only_step_casts_nothing(monkeypatch):
    from vit_ae_plus_plus_amd.optim import MultiTensorAdamW
    monkeypatch.setenv('VITAE_WEIGHT_SHADOW', '1')
    model = vit()
    for n, p in model.named_parameters():
        if not n.startswith('head.'):
            p.requires_grad_(False)
    opt = MultiTensorAdamW([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    x = volumes(2)
    casts = CastCounter(monkeypatch)
    head = model.head.weight.detach().clone()
    for step in range(3):
        opt.zero_grad()
        loss_of(model, x).backward()
        opt.step()
        assert casts.take() == (WEIGHTS if step == 0 else 0), step
    assert not same(head, model.head.weight.detach())
    assert_slots_hold_their_parameters(model, 'frozen backbone')
