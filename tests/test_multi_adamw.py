"""Multi-tensor AdamW for fine-tuning (ABI 54): ``vitae_grad_sqnorm_multi`` / ``vitae_adamw_multi`` and ``optim.MultiTensorAdamW``.

Metric and bound of the update are those of tests/test_optimizer_kernels.py (restated here): e = |p_got - p_64| / |p_64 - p0|
(2-norms) against AdamW in float64, bound 3 x e32 with e32 the same metric of ``torch.optim.AdamW`` in fp32 on the same inputs, per
tensor; m and v likewise relative to their own norms.  The float64 AdamW is ``torch.optim.AdamW`` on float64 tensors (that file shows
it equal to the closed formula to 1e-12); with clipping both references run ``clip_grad_norm_`` first, in their own dtype.

Tensors of fewer than ``POOL_BELOW`` elements are judged together, as ONE vector (the concatenation of them all), under the same
rule: e32 of a tensor of 1 .. 7 elements is the rounding of 1 .. 7 numbers, it is exactly zero for a good share of them and the
ratio of two such figures says nothing, so "per tensor" is only a bound from a few hundred elements on (the file above measures at
n >= 1001).  No element is left out and the rule is the same; an element stepped with the wrong group, or not at all, is 1e3 .. 1e6
times past it.

Norm: |norm - norm_64| / norm_64 <= max(3 x the same figure of ``get_grad_norm_`` in fp32, 6e-8 = one fp32 ulp for when torch
happens to be exact).

Repeats: the kernels add per-workgroup squares into 64 spread slots with double atomics, whose order is not fixed, so the last bit
of the double sum — and with it, rarely, the fp32 norm and the clip factor — is not reproducible.  The repeat test therefore asserts
the parameters and moments bit for bit WITHOUT clipping (the norm only gates the step there) and the norm to one fp32 ulp.

Model tests use the existing micro fixtures and the bounds of the tests they restate (tests/test_vit_finetune.py,
tests/test_vit_finetune_act16.py); nothing is imported from a test file."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from oracle import vit_ref as V
from oracle.gen_golden import MICRO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'vit_finetune.npz')
FEAT = os.path.join(ROOT, 'tests', 'golden', 'vit_features.npz')
GOLD16 = os.path.join(ROOT, 'tests', 'golden', 'vit_finetune_act16.npz')

EPS = 1e-8
BETAS = [(0.9, 0.999), (0.9, 0.95)]
GROUP_LR = (3e-4, 1e-3, 4.2e-5)          # three groups; a tensor's group is its index % 3, so neighbours in the list differ
GROUP_WD = (0.05, 0.0, 0.1)
GUARD = 64                               # elements in front of and behind every buffer that no launch may touch
SENT = {'p': 7.25, 'g': -1.75, 'm': -3.5, 'v': 5.5}
FACTOR = 3.0
POOL_BELOW = 64
ULP = 6e-8


def _consts():
    from vit_ae_plus_plus_amd._abi import CONSTS
    return CONSTS


def _chunk():
    return _consts()['VITAE_MULTI_CHUNK']


def list_lengths(chunk=None):
    c = chunk or _chunk()
    return [1, 3, 4, 5, c - 1, c, c + 1, 2 * c + 5] + [7] * 300


# =========================================================================== CPU
def test_header_abi_and_library_agree():
    import ctypes
    from vit_ae_plus_plus_amd import _abi
    protos, consts = _abi.parse_header()
    assert consts['VITAE_ABI_VERSION'] >= 54
    assert protos['vitae_grad_sqnorm_multi'] == ('int', ['ptr', 'ptr', 'long', 'ptr', 'ptr', 'long', 'long', 'ptr', 'ptr'])
    assert protos['vitae_adamw_multi'] == ('int', ['ptr', 'ptr', 'long', 'ptr', 'ptr', 'long', 'long', 'ptr', 'ptr', 'int', 'double', 'double',
                                                   'double', 'double', 'ptr', 'ptr', 'ptr', 'ptr'])
    for name in ('vitae_grad_sqnorm_multi', 'vitae_adamw_multi'):
        assert _abi.PROTOS[name] == protos[name]
    assert consts['VITAE_MULTI_MAX_GROUPS'] >= 64 and consts['VITAE_MULTI_CHUNK'] > 0 and consts['VITAE_MULTI_CHUNK'] % 4 == 0
    assert consts['VITAE_MULTI_ENTRY_WORDS'] == 6 and consts['VITAE_MULTI_STATE_COUNT'] >= 2
    assert _abi.CONSTS['VITAE_MULTI_CHUNK'] == consts['VITAE_MULTI_CHUNK']
    dll = ctypes.CDLL(_abi.LIB_PATH)
    assert dll.vitae_abi_version() == consts['VITAE_ABI_VERSION']
    for name in ('vitae_grad_sqnorm_multi', 'vitae_adamw_multi'):
        getattr(dll, name)


@pytest.mark.parametrize('chunk', [None, 8, 4096])
def test_chunk_list_covers_every_element_once(chunk):
    """Against the brute-force statement: mark every element every pair covers."""
    from vit_ae_plus_plus_amd.optim import multi_chunk_list, multi_table
    c = chunk or _chunk()
    lengths = list_lengths(c) + [0, 2 * c]
    groups = np.arange(len(lengths)) % 3
    pairs = multi_chunk_list(lengths, chunk)
    assert pairs.dtype == np.int32 and pairs.ndim == 2 and pairs.shape[1] == 2
    cover = [np.zeros(n, dtype=np.int64) for n in lengths]
    for t, k in pairs:
        assert 0 <= t < len(lengths) and k >= 0
        lo, hi = k * c, min(lengths[t], (k + 1) * c)
        assert lo < lengths[t]                                # no chunk starts behind its tensor ...
        assert hi - lo <= c and hi <= lengths[t]              # ... or crosses into the next one
        cover[t][lo:hi] += 1
    for t, cv in enumerate(cover):
        assert (cv == 1).all(), (t, lengths[t])
    assert len(pairs) == sum(-(-n // c) for n in lengths)
    table = multi_table(*([list(range(100, 100 + len(lengths)))] * 4), lengths, groups)
    assert table.shape == (len(lengths), 6) and table.dtype == np.int64
    assert (table[:, 4] == lengths).all() and (table[:, 5] == groups).all()
    assert (table[pairs[:, 0], 5] == groups[pairs[:, 0]]).all()     # the group a chunk is stepped with is its tensor's
    assert (np.diff(table[:, 5]) != 0).all()


def _cpu_params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g) * 0.02) for s in ((5, 3), (7,), (2, 2, 2))]


def _warm(opt, ps, steps=3, seed=1):
    g = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g) * 0.01
        opt.step()


def _same_state_dict(a, b):
    assert a.keys() == b.keys() and a['param_groups'] == b['param_groups'] and a['state'].keys() == b['state'].keys()
    for k in a['state']:
        assert a['state'][k].keys() == b['state'][k].keys()
        for n in a['state'][k]:
            x, y = a['state'][k][n], b['state'][k][n]
            assert x.dtype == y.dtype and x.shape == y.shape and x.device == y.device and torch.equal(x, y), (k, n)


def test_checkpoint_interchange_on_cpu():
    from vit_ae_plus_plus_amd._abi import VitaeError
    from vit_ae_plus_plus_amd.optim import MultiTensorAdamW
    ps = _cpu_params()
    groups = lambda: [{'params': ps[:2], 'lr_scale': 0.5, 'weight_decay': 0.0}, {'params': ps[2:], 'lr_scale': 1.0}]
    t = torch.optim.AdamW(groups(), lr=1e-3, betas=(0.9, 0.95), weight_decay=0.05)
    _warm(t, ps)
    sd = t.state_dict()
    m = MultiTensorAdamW(groups(), lr=3.0, betas=(0.5, 0.5), weight_decay=0.7)
    assert isinstance(m, torch.optim.AdamW) and m.defaults.keys() == t.defaults.keys()
    m.load_state_dict(sd)
    assert m.param_groups[0]['lr_scale'] == 0.5 and m.param_groups[1]['betas'] == (0.9, 0.95) and m.applied_steps() == 3
    _same_state_dict(m.state_dict(), sd)
    back = torch.optim.AdamW(groups(), lr=9.0)
    back.load_state_dict(m.state_dict())
    _same_state_dict(back.state_dict(), sd)
    # state whose per-parameter steps differ is refused
    bad = t.state_dict()
    bad['state'][1] = dict(bad['state'][1], step=torch.tensor(7.0))          # (the packed state shares the optimiser's own dicts)
    with pytest.raises(VitaeError):
        MultiTensorAdamW(groups(), lr=1e-3).load_state_dict(bad)
    # from_torch: the same groups and state, in one line
    f = MultiTensorAdamW.from_torch(t)
    assert isinstance(f, MultiTensorAdamW) and f.applied_steps() == 3
    _same_state_dict(f.state_dict(), sd)
    assert all(f.state[p]['exp_avg'] is t.state[p]['exp_avg'] for p in ps)
    # ... and what it cannot serve: None, nothing changed
    a = torch.optim.AdamW(groups(), lr=1e-3, amsgrad=True)
    b = torch.optim.AdamW([{'params': ps[:2], 'betas': (0.9, 0.95)}, {'params': ps[2:], 'betas': (0.9, 0.999)}], lr=1e-3)
    e = torch.optim.AdamW([{'params': ps[:2], 'eps': 1e-6}, {'params': ps[2:]}], lr=1e-3)
    for o in (a, b, e, torch.optim.AdamW(groups(), lr=1e-3, maximize=True)):
        before = o.state_dict()
        assert MultiTensorAdamW.from_torch(o) is None
        _same_state_dict(o.state_dict(), before)
    assert MultiTensorAdamW.from_torch(torch.optim.SGD(ps, lr=0.1)) is None
    with pytest.raises(VitaeError):
        MultiTensorAdamW(ps, amsgrad=True)
    # no CPU fallback: a step on CPU parameters raises and changes nothing
    snap = [p.detach().clone() for p in ps]
    for p in ps:
        p.grad = torch.ones_like(p)
    with pytest.raises(VitaeError):
        f.step()
    with pytest.raises(VitaeError):
        f.norm_clip_step(1.0)
    assert all(torch.equal(p.detach(), s) for p, s in zip(ps, snap))
    # zero_grad and add_param_group are torch's
    f.zero_grad()
    assert all(p.grad is None for p in ps)
    extra = torch.nn.Parameter(torch.zeros(3))
    f.add_param_group({'params': [extra], 'lr_scale': 0.1})
    assert f.param_groups[-1]['lr_scale'] == 0.1 and f.param_groups[-1]['betas'] == (0.9, 0.95)


def test_scaler_takes_the_new_branch_only_for_owned_gradients():
    """No GPU: a stand-in optimiser records which path NativeScalerWithGradNormCount takes."""
    from vit_ae_plus_plus_amd.utils.misc import NativeScalerWithGradNormCount, get_grad_norm_
    ps = _cpu_params()
    other = torch.nn.Parameter(torch.ones(4))

    class Spy(torch.optim.SGD):
        calls = []

        def norm_clip_step(self, max_norm=None):
            self.calls.append(('norm_clip_step', max_norm))
            return torch.tensor(42.0)

        def step(self, closure=None):
            self.calls.append(('step',))

    opt = Spy(ps, lr=0.0)
    scaler = NativeScalerWithGradNormCount()
    loss = lambda extra=0.0: sum((p * p).sum() for p in ps) + extra
    assert float(scaler(loss(), opt, clip_grad=0.5, parameters=ps)) == 42.0
    assert float(scaler(loss(), opt)) == 42.0
    assert scaler(loss(), opt, update_grad=False) is None
    assert Spy.calls == [('norm_clip_step', 0.5), ('norm_clip_step', None)]
    # a gradient the optimiser does not own: the generic path, whose norm includes it
    for p in ps:
        p.grad = None
    norm = scaler(loss((other * other).sum()), opt, parameters=ps + [other])
    assert Spy.calls[-1] == ('step',) and len(Spy.calls) == 3
    assert float(norm) == float(get_grad_norm_(ps + [other])) > float(get_grad_norm_(ps))


# =========================================================================== references (CPU, shared by the GPU tests)
def make_list(lengths, seed, warm):
    """fp32 CPU inputs of one tensor list: weights at the scale of real ones, warm or zero moments."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in lengths:
        p0 = torch.randn(n, generator=g) * 0.02
        m0 = torch.randn(n, generator=g) * 0.005 if warm else torch.zeros(n)
        v0 = torch.rand(n, generator=g) * 1e-4 + 1e-7 if warm else torch.zeros(n)
        out.append((p0, m0, v0))
    return out


def make_grads(lengths, steps, seed, scale=0.01):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(n, generator=g) * scale * (1.0 if k % 2 else -1.0) for n in lengths] for k in range(steps)]


def lr_schedule(k):
    """What lr_sched.adjust_learning_rate does to every group between steps: lr = schedule x lr_scale."""
    return 0.5 * (1.0 + np.cos(np.pi * k / 25.0)) if k else 1.0


def torch_reference(tensors, grads, betas, t0, dtype, max_norm=None, lr_of=lr_schedule, shift=0):
    """``[clip_grad_norm_ +] torch.optim.AdamW`` in ``dtype`` on the CPU -> ([(p, m, v)], [norm of every step])."""
    ps = [p0.to(dtype).clone().requires_grad_(True) for p0, _, _ in tensors]
    opt = torch.optim.AdamW([{'params': [q for i, q in enumerate(ps) if (i + shift) % 3 == gi], 'weight_decay': GROUP_WD[gi], 'lr': GROUP_LR[gi]}
                             for gi in range(3)], betas=betas, eps=EPS)
    for q, (_, m0, v0) in zip(ps, tensors):
        opt.state[q] = {'step': torch.tensor(float(t0)), 'exp_avg': m0.to(dtype).clone(), 'exp_avg_sq': v0.to(dtype).clone()}
    norms = []
    for k, gs in enumerate(grads):
        for gi, group in enumerate(opt.param_groups):
            group['lr'] = GROUP_LR[gi] * lr_of(k)
        for q, g in zip(ps, gs):
            q.grad = g.to(dtype).clone()
        if max_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(ps, max_norm)))
        else:
            norms.append(float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(q.grad) for q in ps]))))
        opt.step()
    return [(q.detach(), opt.state[q]['exp_avg'], opt.state[q]['exp_avg_sq']) for q in ps], norms


def _err(got, ref, base=None):
    ref = ref.double()
    den = (ref - base.double()).norm() if base is not None else ref.norm()
    return float((got.double() - ref).norm() / den.clamp_min(1e-300))


def judged_units(lengths):
    """Index lists: every tensor of >= POOL_BELOW elements alone, all smaller ones together (module docstring)."""
    big = [[i] for i, n in enumerate(lengths) if n >= POOL_BELOW]
    small = [i for i, n in enumerate(lengths) if n < POOL_BELOW]
    return big + ([small] if small else [])


def check_against_references(got, tensors, ref64, ref32, label):
    """got / ref64 / ref32: [(p, m, v)] on the CPU.  The 3 x e32 rule on p (share of the update), m and v (own norms)."""
    lengths = [t[0].numel() for t in tensors]
    worst = {}
    cat = lambda xs, idx, j: torch.cat([xs[i][j].reshape(-1).cpu() for i in idx])
    for idx in judged_units(lengths):
        for j, name in enumerate('pmv'):
            base = cat(tensors, idx, 0) if j == 0 else None
            r64 = cat(ref64, idx, j)
            e, e32 = _err(cat(got, idx, j), r64, base), _err(cat(ref32, idx, j), r64, base)
            key = f'{name} of tensors {idx[0]}..{idx[-1]} ({sum(lengths[i] for i in idx)} elements)'
            assert e <= FACTOR * e32, f'{label}: {key}: e={e:.3e} e32={e32:.3e}'
            worst[name] = max(worst.get(name, (0.0, '')), (e / e32 if e32 else 0.0, key))
    print(f'RATIO {label}: ' + '; '.join(f'{n} {r:.2f} ({k})' for n, (r, k) in worst.items()))


def test_references_agree_with_each_other():
    """The fp32 side of every comparison is itself a sane AdamW: within 1e-4 of the update of the float64 one (the smallest lr moves a weight by 2e-3 of itself, 1e4 fp32 ulps) (so that 3 x e32 is a
    bound worth having), with and without clipping, and pooling leaves no tensor out."""
    lengths = list_lengths()                                 # the lengths of the GPU tests, around the library's chunk length
    tensors, grads = make_list(lengths, 3, True), make_grads(lengths, 3, 4)
    assert sorted(i for u in judged_units(lengths) for i in u) == list(range(len(lengths)))
    for max_norm in (None, 0.5):
        r64, n64 = torch_reference(tensors, grads, (0.9, 0.999), 999, torch.float64, max_norm)
        r32, n32 = torch_reference(tensors, grads, (0.9, 0.999), 999, torch.float32, max_norm)
        assert max(abs(a - b) / a for a, b in zip(n64, n32)) < 1e-6
        for idx in judged_units(lengths):
            cat = lambda xs, j: torch.cat([xs[i][j] for i in idx])
            e32 = _err(cat(r32, 0), cat(r64, 0), cat(tensors, 0))
            assert 0 < e32 < 1e-4, (idx[:3], e32)
    # the mutants of LABNOTES.md that a reference can play: each is far outside 3 x e32
    r64, _ = torch_reference(tensors, grads[:1], (0.9, 0.999), 999, torch.float64)
    r32, _ = torch_reference(tensors, grads[:1], (0.9, 0.999), 999, torch.float32)
    wrong_group, _ = torch_reference(tensors, grads[:1], (0.9, 0.999), 999, torch.float32, shift=1)     # every tensor with its neighbour's group
    with pytest.raises(AssertionError):
        check_against_references(wrong_group, tensors, r64, r32, 'mutant')
    short = [tuple(x.clone() for x in t) for t in r32]
    short[7][0][-1] = tensors[7][0][-1]                      # the last element of the last chunk not stepped
    with pytest.raises(AssertionError):
        check_against_references(short, tensors, r64, r32, 'mutant')


# =========================================================================== launches (GPU)
gpu = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    from vit_ae_plus_plus_amd._abi import lib as L
    L.load()
    return L


def st():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """One tensor of n elements on the device with GUARD sentinels on both sides; ``off`` elements (4 bytes each) off 16-byte alignment."""

    def __init__(self, x, sentinel, off=0):
        n = x.numel()
        buf = torch.full((GUARD + off + n + GUARD,), sentinel, dtype=torch.float32)
        buf[GUARD + off:GUARD + off + n] = x
        self.buf, self.lo, self.n, self.sentinel = buf.cuda(), GUARD + off, n, sentinel
        assert self.buf.data_ptr() % 16 == 0

    @property
    def t(self):
        return self.buf[self.lo:self.lo + self.n]

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.lo

    def set(self, x):
        self.t.copy_(x)

    def guards_intact(self):
        return bool((self.buf[:self.lo] == self.sentinel).all()) and bool((self.buf[self.lo + self.n:] == self.sentinel).all())


class DeviceList:
    """A tensor list on the device, its table and chunk list (host and device copies), state and accumulator."""

    def __init__(self, tensors, misalign=None, t0=0, chunk=None):
        from vit_ae_plus_plus_amd.optim import multi_chunk_list, multi_table
        C = _consts()
        self.C, self.chunk = C, chunk or C['VITAE_MULTI_CHUNK']
        off = lambda kind, i: 1 if (misalign == kind and i % 2 == 1) else 0
        self.p = [Guarded(t[0], SENT['p'], off('p', i)) for i, t in enumerate(tensors)]
        self.m = [Guarded(t[1], SENT['m'], off('m', i)) for i, t in enumerate(tensors)]
        self.v = [Guarded(t[2], SENT['v'], off('v', i)) for i, t in enumerate(tensors)]
        self.g = [Guarded(torch.zeros_like(t[0]), SENT['g'], off('g', i)) for i, t in enumerate(tensors)]
        if misalign:
            kind = getattr(self, misalign)
            assert kind[1].ptr % 16 == 4 and kind[0].ptr % 16 == 0 and any(x.ptr % 16 for x in kind if x.n > 2 * self.chunk)
        self.lengths = [t[0].numel() for t in tensors]
        self.groups = [i % 3 for i in range(len(tensors))]
        self.table = multi_table(*[[x.ptr for x in k] for k in (self.p, self.g, self.m, self.v)], self.lengths, self.groups)
        self.chunks = np.ascontiguousarray(multi_chunk_list(self.lengths, self.chunk))
        self.state = torch.tensor([float(t0), 0.0], dtype=torch.float32).cuda()
        self.acc = torch.zeros(C['VITAE_ACC_COUNT'], dtype=torch.float64).cuda()
        self.norm = torch.full((1 + 2 * GUARD,), 99.0, dtype=torch.float32).cuda()
        self.upload()

    def upload(self, lr_mul=1.0):
        self.table_d = torch.from_numpy(self.table).cuda()
        self.chunks_d = torch.from_numpy(self.chunks).cuda()
        self.hyper_d = torch.tensor([l * lr_mul for l in GROUP_LR] + list(GROUP_WD), dtype=torch.float32).cuda()

    def args(self, table=None, chunks=None, n_tensors=None, n_chunks=None):
        table = self.table if table is None else table
        chunks = self.chunks if chunks is None else chunks
        self._keep = (table, chunks)
        return (table.ctypes.data, self.table_d.data_ptr(), len(self.lengths) if n_tensors is None else n_tensors,
                chunks.ctypes.data, self.chunks_d.data_ptr(), len(self.chunks) if n_chunks is None else n_chunks, self.chunk)

    def step(self, lib, grads, betas, lr_mul=1.0, max_norm=0.0):
        for x, g in zip(self.g, grads):
            x.set(g)
        self.hyper_d = torch.tensor([l * lr_mul for l in GROUP_LR] + list(GROUP_WD), dtype=torch.float32).cuda()
        lib.vitae_grad_sqnorm_multi(*self.args(), self.acc.data_ptr(), st())
        self.adamw(lib, betas, max_norm)
        torch.cuda.synchronize()
        return float(self.norm[GUARD])

    def adamw(self, lib, betas, max_norm=0.0, **kw):
        return lib.vitae_adamw_multi(*self.args(**kw), self.hyper_d.data_ptr(), self.hyper_d.data_ptr() + 12, 3, betas[0], betas[1], EPS,
                                     float(max_norm), self.state.data_ptr(), self.acc.data_ptr(), self.norm.data_ptr() + 4 * GUARD, st())

    def result(self):
        return [(p.t.cpu(), m.t.cpu(), v.t.cpu()) for p, m, v in zip(self.p, self.m, self.v)]

    def snapshot(self):
        return [x.buf.clone() for k in (self.p, self.g, self.m, self.v) for x in k] + [self.state.clone(), self.acc.clone(), self.norm.clone()]

    def unchanged_since(self, snap):
        now = self.snapshot()
        return all(torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int64),
                               b.view(torch.int32 if b.dtype == torch.float32 else torch.int64)) for a, b in zip(now, snap))

    def assert_guards(self):
        for k in (self.p, self.g, self.m, self.v):
            for i, x in enumerate(k):
                assert x.guards_intact(), i
        assert bool((self.norm[:GUARD] == 99.0).all()) and bool((self.norm[GUARD + 1:] == 99.0).all())

    def assert_accumulator_zero(self):
        assert float(self.acc.abs().sum()) == 0.0 and bool((self.acc.view(torch.int64) == 0).all())


_REFS = {}


def shared_reference(betas, t0, steps, max_norm=None):
    """Computed once per (case), shared by the tests that need it, never modified."""
    key = (betas, t0, steps, max_norm)
    if key not in _REFS:
        lengths = list_lengths()
        tensors, grads = make_list(lengths, 11 + t0, t0 > 0), make_grads(lengths, steps, 12 + t0)
        r64 = torch_reference(tensors, grads, betas, t0, torch.float64, max_norm)
        r32 = torch_reference(tensors, grads, betas, t0, torch.float32, max_norm)
        _REFS[key] = (tensors, grads, r64, r32)
    return _REFS[key]


@pytest.fixture(scope='module', autouse=True)
def _drop_references():
    yield
    _REFS.clear()


def check_norm(got, n64, n32, label):
    e, e32 = abs(got - n64) / n64, abs(n32 - n64) / n64
    print(f'NORM {label}: got {got!r} float64 {n64!r} fp32 torch {n32!r}: e={e:.2e} e32={e32:.2e}')
    assert e <= max(FACTOR * e32, ULP), (got, n64, n32)


CASES = [(None, 1, 0), (None, 1, 1), (None, 1, 999), (None, 20, 0), (None, 20, 999),
         ('p', 1, 999), ('g', 1, 999), ('m', 1, 999), ('v', 1, 999), ('g', 20, 0)]


@gpu
@pytest.mark.parametrize('betas', BETAS)
@pytest.mark.parametrize('misalign,steps,t0', CASES)
def test_update_of_a_mixed_list(lib, betas, misalign, steps, t0):
    tensors, grads, (r64, n64), (r32, n32) = shared_reference(betas, t0, steps)
    check_against_references(r32, tensors, r64, r32, 'reference side')          # the comparator stays inside the bound by itself
    d = DeviceList(tensors, misalign, t0)
    for k, gs in enumerate(grads):
        norm = d.step(lib, gs, betas, lr_schedule(k))
        check_norm(norm, n64[k], n32[k], f'step {k}')
        d.assert_accumulator_zero()
        assert all(torch.equal(x.t.cpu(), g) for x, g in zip(d.g, gs))          # gradients are read, never written
    d.assert_guards()
    assert d.state.tolist() == [float(t0 + steps), 0.0]
    check_against_references(d.result(), tensors, r64, r32, f'betas={betas} misalign={misalign} steps={steps} t0={t0}')


@gpu
def test_norm_with_one_large_element(lib):
    lengths = list_lengths()
    tensors = make_list(lengths, 5, False)
    g = make_grads(lengths, 1, 6, scale=1e-3)[0]
    g[6][77] = 1e4
    n64 = float(torch.cat(g).double().norm())
    n32 = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(x) for x in g])))
    d = DeviceList(tensors)
    check_norm(d.step(lib, g, BETAS[0]), n64, n32, 'one element of 1e4 among 1e-3')
    # ... and without it, where every element counts
    g[6][77] = 1e-3
    n64 = float(torch.cat(g).double().norm())
    n32 = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(x) for x in g])))
    check_norm(d.step(lib, g, BETAS[0]), n64, n32, 'values of 1e-3')
    d.assert_guards()


@gpu
@pytest.mark.parametrize('where', ['below', 'equal', 'above'])
def test_clipping(lib, where):
    betas, t0 = BETAS[0], 999
    tensors, grads, _, _ = shared_reference(betas, t0, 1)
    n64 = float(torch.cat(grads[0]).double().norm())
    max_norm = {'below': 0.25 * n64, 'equal': float(np.float32(n64)), 'above': 4.0 * n64}[where]
    r64, w64 = torch_reference(tensors, grads, betas, t0, torch.float64, max_norm)
    r32, w32 = torch_reference(tensors, grads, betas, t0, torch.float32, max_norm)
    check_against_references(r32, tensors, r64, r32, 'reference side')
    d = DeviceList(tensors, None, t0)
    norm = d.step(lib, grads[0], betas, max_norm=max_norm)
    check_norm(norm, w64[0], w32[0], f'clip {where}')                           # the norm BEFORE clipping, as clip_grad_norm_ returns it
    assert all(torch.equal(x.t.cpu(), g) for x, g in zip(d.g, grads[0]))        # .grad stays bit-equal: the factor is applied as it is read
    d.assert_guards()
    check_against_references(d.result(), tensors, r64, r32, f'clip {where} max_norm={max_norm:.4g} norm={n64:.4g}')
    if where == 'below':
        # what the comparison is worth: the unclipped update is far outside the bound
        unclipped, _ = torch_reference(tensors, grads, betas, t0, torch.float32, None)
        with pytest.raises(AssertionError):
            check_against_references(unclipped, tensors, r64, r32, 'mutant: no clip factor')
        # ... and so is the clip factor missing from the second moment only
        no_v = [(p, m, u[2]) for (p, m, _), u in zip(r32, unclipped)]
        with pytest.raises(AssertionError):
            check_against_references(no_v, tensors, r64, r32, 'mutant: clip factor missing from v')


@gpu
@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
def test_non_finite_gradient_skips_the_step(lib, bad):
    betas, t0 = BETAS[0], 999
    tensors, grads, (r64, n64), (r32, n32) = shared_reference(betas, t0, 1)
    d = DeviceList(tensors, None, t0)
    poisoned = [g.clone() for g in grads[0]]
    poisoned[len(poisoned) // 2][3] = bad                   # one gradient of one tensor in the middle of the list
    for x, g in zip(d.g, poisoned):
        x.set(g)
    snap = [x.buf.clone() for k in (d.p, d.m, d.v) for x in k]
    norm = d.step(lib, poisoned, betas, max_norm=1.0)
    assert not np.isfinite(norm)
    now = [x.buf for k in (d.p, d.m, d.v) for x in k]
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(now, snap))     # not a bit
    assert d.state.tolist() == [float(t0), 1.0]             # the step counter stays, the skipped counter goes up by one
    d.assert_accumulator_zero()
    # the following clean step is the step the references make
    norm = d.step(lib, grads[0], betas)
    check_norm(norm, n64[0], n32[0], 'clean step after a skipped one')
    assert d.state.tolist() == [float(t0 + 1), 1.0]
    d.assert_accumulator_zero()
    d.assert_guards()
    check_against_references(d.result(), tensors, r64, r32, f'after a skipped step ({bad})')


@gpu
def test_repeats_are_bit_equal(lib):
    """Parameters and moments bit for bit (no clipping: module docstring); the norm to one fp32 ulp."""
    betas, t0 = BETAS[1], 1
    tensors, grads, _, _ = shared_reference(betas, t0, 1)
    out = []
    for _ in range(2):
        d = DeviceList(tensors, 'g', t0)
        norm = d.step(lib, grads[0], betas)
        out.append((norm, [x.buf.clone() for k in (d.p, d.m, d.v) for x in k]))
    assert abs(out[0][0] - out[1][0]) <= ULP * out[0][0]
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out[0][1], out[1][1]))


@gpu
def test_refusals_write_nothing_and_an_empty_list_succeeds(lib):
    from vit_ae_plus_plus_amd._abi import VitaeError
    betas = BETAS[0]
    lengths = [5, 4096, 7]
    tensors = make_list(lengths, 1, True)
    d = DeviceList(tensors, None, 3, chunk=1024)
    for x, g in zip(d.g, make_grads(lengths, 1, 2)[0]):
        x.set(g)
    torch.cuda.synchronize()
    snap = d.snapshot()

    def edited(col, value, row=1):
        t = d.table.copy()
        t[row, col] = value
        return t

    refused = []
    for col in range(4):                                     # a NULL address in an entry
        refused.append(lambda col=col: d.adamw(lib, betas, table=edited(col, 0)))
    refused.append(lambda: lib.vitae_grad_sqnorm_multi(*d.args(table=edited(1, 0)), d.acc.data_ptr(), st()))
    refused.append(lambda: d.adamw(lib, betas, table=edited(4, -1)))                       # negative counts
    refused.append(lambda: d.adamw(lib, betas, n_tensors=-1))
    refused.append(lambda: d.adamw(lib, betas, n_chunks=-1))
    refused.append(lambda: lib.vitae_grad_sqnorm_multi(*d.args(n_chunks=-2), d.acc.data_ptr(), st()))
    refused.append(lambda: d.adamw(lib, betas, table=edited(5, 3)))                        # a group outside the group arrays
    refused.append(lambda: d.adamw(lib, betas, table=edited(5, -1)))
    bad_chunks = d.chunks.copy()
    bad_chunks[-1] = (1, 4)                                                                 # a chunk behind its tensor (4096 = 4 x 1024)
    refused.append(lambda: d.adamw(lib, betas, chunks=bad_chunks))
    refused.append(lambda: lib.vitae_grad_sqnorm_multi(*d.args(chunks=bad_chunks), d.acc.data_ptr(), st()))
    bad_chunks2 = d.chunks.copy()
    bad_chunks2[0, 0] = 3                                                                   # a tensor that is not in the table
    refused.append(lambda: d.adamw(lib, betas, chunks=bad_chunks2))
    a = d.args()
    hp, nrm = d.hyper_d.data_ptr(), d.norm.data_ptr() + 4 * GUARD
    tail = lambda state=d.state.data_ptr(), acc=d.acc.data_ptr(), norm=nrm: (betas[0], betas[1], EPS, 0.0, state, acc, norm, st())
    M = d.C['VITAE_MULTI_MAX_GROUPS']
    refused.append(lambda: lib.vitae_adamw_multi(*a, hp, hp + 12, M + 1, *tail()))         # more groups than the bound
    refused.append(lambda: lib.vitae_adamw_multi(*a, hp, hp + 12, 0, *tail()))
    refused.append(lambda: lib.vitae_adamw_multi(*a, None, hp + 12, 3, *tail()))           # NULL where one is required
    refused.append(lambda: lib.vitae_adamw_multi(*a, hp, None, 3, *tail()))
    refused.append(lambda: lib.vitae_adamw_multi(*a, hp, hp + 12, 3, *tail(state=None)))
    refused.append(lambda: lib.vitae_adamw_multi(*a, hp, hp + 12, 3, *tail(acc=None)))
    refused.append(lambda: lib.vitae_adamw_multi(*a, hp, hp + 12, 3, *tail(norm=None)))
    refused.append(lambda: lib.vitae_adamw_multi(None, *a[1:], hp, hp + 12, 3, *tail()))
    refused.append(lambda: lib.vitae_adamw_multi(a[0], None, *a[2:], hp, hp + 12, 3, *tail()))
    refused.append(lambda: lib.vitae_adamw_multi(*a[:3], None, *a[4:], hp, hp + 12, 3, *tail()))
    refused.append(lambda: lib.vitae_adamw_multi(*a[:4], None, *a[5:], hp, hp + 12, 3, *tail()))
    refused.append(lambda: lib.vitae_adamw_multi(*a[:6], 0, hp, hp + 12, 3, *tail()))      # chunk <= 0, chunk % 4
    refused.append(lambda: lib.vitae_adamw_multi(*a[:6], 1022, hp, hp + 12, 3, *tail()))
    refused.append(lambda: lib.vitae_grad_sqnorm_multi(*a, None, st()))
    refused.append(lambda: lib.vitae_grad_sqnorm_multi(a[0], None, *a[2:], d.acc.data_ptr(), st()))
    for i, call in enumerate(refused):
        with pytest.raises(VitaeError):
            call()
            pytest.fail(f'refusal {i} was accepted')
    torch.cuda.synchronize()
    assert d.unchanged_since(snap)
    # an empty list: success, nothing launched, nothing written (not even the norm or a counter)
    assert lib.vitae_grad_sqnorm_multi(None, None, 0, None, None, 0, d.chunk, d.acc.data_ptr(), st()) == 0
    assert lib.vitae_adamw_multi(None, None, 0, None, None, 0, d.chunk, hp, hp + 12, 3, *tail()) == 0
    assert d.adamw(lib, betas, n_chunks=0) == 0
    torch.cuda.synchronize()
    assert d.unchanged_since(snap)


# =========================================================================== the class on the device
def _device_params(lengths, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(n, generator=g) * 0.02).cuda()) for n in lengths]


def _groups(ps):
    return [{'params': ps[gi::3], 'weight_decay': GROUP_WD[gi], 'lr': GROUP_LR[gi]} for gi in range(3)]


SWITCH_LENGTHS = [1, 5, 1000, 4099, 20000, 7, 7, 33000]


def _switch_reference(dtype):
    tensors = make_list(SWITCH_LENGTHS, 21, False)
    grads = make_grads(SWITCH_LENGTHS, 4, 22)
    ps = [t[0].to(dtype).clone().requires_grad_(True) for t in tensors]
    opt = torch.optim.AdamW(_groups(ps), betas=(0.9, 0.999), eps=EPS)
    for gs in grads:
        for q, g in zip(ps, gs):
            q.grad = g.to(dtype).clone()
        opt.step()
    # in list order ps[gi::3] is group gi: the index % 3 rule of the kernel tests
    return tensors, grads, [(q.detach(), opt.state[q]['exp_avg'], opt.state[q]['exp_avg_sq']) for q in ps]


@gpu
@pytest.mark.parametrize('direction', ['torch_then_multi', 'multi_then_torch', 'multi_alone'])
def test_mid_run_switch(direction):
    """Two steps with one optimiser, two with the other (from_torch one way, state_dict the other), on fixed gradient sequences:
    the four steps of the float64 AdamW, under the 3 x rule against four steps of torch's fp32 AdamW alone."""
    from vit_ae_plus_plus_amd.optim import MultiTensorAdamW
    tensors, grads, r64 = _switch_reference(torch.float64)
    _, _, r32 = _switch_reference(torch.float32)
    check_against_references(r32, tensors, r64, r32, 'reference side')
    ps = [torch.nn.Parameter(t[0].clone().cuda()) for t in tensors]

    def run(opt, seq):
        for gs in seq:
            for q, g in zip(ps, gs):
                q.grad = g.clone().cuda()
            opt.step()
            opt.zero_grad(set_to_none=True)

    if direction == 'torch_then_multi':
        first = torch.optim.AdamW(_groups(ps), betas=(0.9, 0.999), eps=EPS)
        run(first, grads[:2])
        second = MultiTensorAdamW.from_torch(first)
        assert second is not None and second.applied_steps() == 2
        run(second, grads[2:])
    elif direction == 'multi_then_torch':
        first = MultiTensorAdamW(_groups(ps), betas=(0.9, 0.999), eps=EPS)
        run(first, grads[:2])
        second = torch.optim.AdamW(_groups(ps), betas=(0.9, 0.999), eps=EPS)
        second.load_state_dict(first.state_dict())
        assert all(float(s['step']) == 2.0 for s in second.state.values())
        run(second, grads[2:])
    else:
        second = MultiTensorAdamW(_groups(ps), betas=(0.9, 0.999), eps=EPS)
        run(second, grads)
        assert second.applied_steps() == 4 and second.skipped_steps() == 0
    sd = second.state_dict()
    assert all(float(s['step']) == 4.0 for s in sd['state'].values())
    got = [(q.detach().cpu(), second.state[q]['exp_avg'].cpu(), second.state[q]['exp_avg_sq'].cpu()) for q in ps]
    check_against_references(got, tensors, r64, r32, direction)


@gpu
def test_class_norm_clipping_versions_and_missing_gradients():
    from vit_ae_plus_plus_amd.optim import MultiTensorAdamW
    from vit_ae_plus_plus_amd.utils.misc import get_grad_norm_
    ps = _device_params(SWITCH_LENGTHS, 3)
    opt = MultiTensorAdamW(_groups(ps), betas=(0.9, 0.95), eps=EPS)
    grads = make_grads(SWITCH_LENGTHS, 3, 9)
    absent = {2, 5}
    for k, gs in enumerate(grads):
        for i, (q, g) in enumerate(zip(ps, gs)):
            q.grad = None if i in absent else g.clone().cuda()      # new gradient tensors every iteration
        held = [None if q.grad is None else q.grad.clone() for q in ps]
        before = [q.detach().clone() for q in ps]
        versions = [q._version for q in ps]
        want = get_grad_norm_(ps)
        norm = opt.norm_clip_step(0.5 * float(want)) if k else opt.norm_clip_step(None)
        assert norm.ndim == 0 and norm.is_cuda and norm.dtype == torch.float32
        assert abs(float(norm) - float(want)) <= 1e-6 * float(want)
        for i, q in enumerate(ps):
            if i in absent:       # left out of the step, as torch does: no update, no state, no version bump
                assert torch.equal(q.detach(), before[i]) and not opt.state.get(q) and q._version == versions[i]
            else:
                assert not torch.equal(q.detach(), before[i]) and q._version > versions[i]
                assert torch.equal(q.grad, held[i])                  # clipping does not rewrite .grad
    assert opt.applied_steps() == 3 and opt.skipped_steps() == 0
    # a non-finite gradient: nothing moves, the count stays, the skipped count goes up, the norm says why
    ps[0].grad = torch.full_like(ps[0], float('inf'))
    before = [q.detach().clone() for q in ps]
    assert not np.isfinite(float(opt.norm_clip_step(1.0)))
    assert all(torch.equal(q.detach(), b) for q, b in zip(ps, before))
    assert opt.applied_steps() == 3 and opt.skipped_steps() == 1
    assert all(float(s['step']) == 3.0 for s in opt.state_dict()['state'].values())
    # non-contiguous or non-fp32 parameters are refused at step()
    from vit_ae_plus_plus_amd._abi import VitaeError
    half = torch.nn.Parameter(torch.zeros(8, device='cuda', dtype=torch.bfloat16))
    half.grad = torch.ones_like(half)
    with pytest.raises(VitaeError):
        MultiTensorAdamW([half]).step()
    nc = torch.nn.Parameter(torch.zeros(8, 4, device='cuda').t())
    nc.grad = torch.ones(4, 8, device='cuda')
    with pytest.raises(VitaeError):
        MultiTensorAdamW([nc]).step()


# =========================================================================== the model (existing micro fixtures, existing bounds)
ENC = {k: MICRO[k] for k in ('volume_size', 'patch_size', 'in_chans', 'embed_dim', 'depth', 'num_heads')}
TAGS = {False: 'cls', True: 'gp'}


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD, allow_pickle=False)


@pytest.fixture(scope='module')
def x_micro():
    return torch.from_numpy(np.load(FEAT, allow_pickle=False)['micro/x'])


def _module(cfg, precision='fp32', **kw):
    from vit_ae_plus_plus_amd.model.vit import VisionTransformer3D
    return VisionTransformer3D(volume_size=cfg.volume_size[0], patch_size=cfg.patch_size, in_chans=cfg.in_chans,
                               num_classes=cfg.num_classes, embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads,
                               global_pool=cfg.global_pool, precision=precision, **kw)


def _micro(gp, precision='fp32', **kw):
    cfg = V.VitConfig(num_classes=3, global_pool=gp, **ENC)
    m = _module(cfg, precision, **kw).cuda().train()
    m.load_state_dict(V.init_vit_state_dict(cfg, seed=5))
    return m


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _losses(m, opt, x, y, crit, steps=4):
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = crit(m(x), y)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


@gpu
@pytest.mark.parametrize('gp', [False, True])
@pytest.mark.parametrize('precision', ['fp32', 'fp32x3'])
def test_finetune_adamw_trajectory_micro(gold, x_micro, gp, precision):
    """_check_trajectory of tests/test_vit_finetune.py with MultiTensorAdamW: four steps against the reference's losses at 1e-4."""
    from vit_ae_plus_plus_amd.optim import MultiTensorAdamW
    m = _micro(gp, precision)
    crit = torch.nn.CrossEntropyLoss(weight=torch.from_numpy(gold['class_weights']).cuda())
    opt = MultiTensorAdamW(m.parameters(), lr=1e-3, weight_decay=0.05)
    losses = _losses(m, opt, x_micro.cuda(), torch.from_numpy(gold['labels']).cuda(), crit)
    ref = gold[f'{TAGS[gp]}/adamw_losses']
    print(f'{precision} {TAGS[gp]} MultiTensorAdamW losses {losses} (reference {list(ref)})')
    for a, b in zip(losses, ref):
        assert abs(a - b) <= 1e-4 * abs(b), (losses, list(ref))
    assert opt.applied_steps() == 4


ENC16 = dict(volume_size=(16, 16, 16), patch_size=4, in_chans=1, embed_dim=64, depth=2)
STORED16 = [('h32', False, 2), ('h64', True, 1)]


@gpu
@pytest.mark.parametrize('name,gp,heads', STORED16, ids=['h32-cls', 'h64-gp'])
def test_route_adamw_trajectory_bf16_activations(name, gp, heads):
    """The rule of tests/test_vit_finetune_act16.py::test_route_adamw_trajectory on the two pairs its fixture stores: step i of the
    bf16-activation route stepped by MultiTensorAdamW deviates from the fp32 loss by at most 2 x max(the reference under autocast,
    the existing bf16 route stepped by torch.optim.AdamW in the same run).  This is the test that sees a missing version bump: the
    route's bf16 weight copies are keyed by ``p._version``, and stale copies repeat the first loss four times."""
    from vit_ae_plus_plus_amd.optim import MultiTensorAdamW
    g16 = np.load(GOLD16, allow_pickle=False)
    cfg = V.VitConfig(num_classes=3, global_pool=gp, num_heads=heads, **ENC16)
    x, y = torch.from_numpy(g16['x']).cuda(), torch.from_numpy(g16['labels']).cuda()
    crit = torch.nn.CrossEntropyLoss(weight=torch.from_numpy(g16['class_weights']).cuda())
    ref, ref_dev = g16[f'{name}/{TAGS[gp]}/adamw_losses'], g16[f'{name}/{TAGS[gp]}/bf16_ref_adamw_dev']
    dev = {}
    for act, make in (('bf16', MultiTensorAdamW), (None, torch.optim.AdamW)):
        m = _module(cfg, 'bf16', activations=act).cuda().train()
        m.load_state_dict(V.init_vit_state_dict(cfg, seed=5))
        losses = _losses(m, make(m.parameters(), lr=1e-3, weight_decay=0.05), x, y, crit)
        dev[act] = np.abs(np.array(losses) - ref)
        print(f'{name}/{TAGS[gp]} activations={act} {make.__name__}: {losses} (fp32 {list(ref)}); deviation {list(dev[act])}')
    assert np.isfinite(dev['bf16']).all()
    bound = 2.0 * np.maximum(np.asarray(ref_dev), dev[None])
    print(f'reference under autocast deviates by {list(ref_dev)}; new / bound per step: {list(np.round(dev["bf16"] / bound, 2))}')
    assert (dev['bf16'] <= bound).all(), (list(dev['bf16']), list(bound))


@gpu
def test_finetune_epoch_soft_targets_accumulation(gold, x_micro):
    """The scenario of the test of that name in tests/test_vit_finetune.py through NativeScalerWithGradNormCount's new branch, with
    its bounds (loss 1e-4, parameter deltas 1e-4 relative L2, the key third of ``attn.qkv.bias`` held to |step| <= lr x lr_scale:
    its gradient is rounding noise, see there).  The returned norm against get_grad_norm_ on the same gradients: 1e-6, the suite's
    bound for two fp32 summation orders of the same numbers."""
    from vit_ae_plus_plus_amd.optim import MultiTensorAdamW
    from vit_ae_plus_plus_amd.post_training_utils.fine_tune_epoch import train_one_epoch
    from vit_ae_plus_plus_amd.utils.custom_loss import SoftCrossEntropyWithWeightsLoss
    from vit_ae_plus_plus_amd.utils.lr_decay import get_layer_id_for_vit, param_groups_lrd
    from vit_ae_plus_plus_amd.utils.misc import NativeScalerWithGradNormCount, get_grad_norm_
    accum_iter, lr, min_lr, warmup_epochs, epochs, epoch = (float(v) for v in gold['epoch/args'])
    args = Namespace(accum_iter=int(accum_iter), lr=lr, min_lr=min_lr, warmup_epochs=warmup_epochs, epochs=epochs)
    t0, t1 = (torch.from_numpy(t) for t in gold['epoch/targets'])
    batches = [(x_micro, None, t0), (x_micro.flip(0).contiguous(), None, t1)]
    m = _micro(True)
    before = {n: p.detach().cpu().clone() for n, p in m.named_parameters()}
    wd, ld = (float(v) for v in gold['lrd/args'])
    opt = MultiTensorAdamW(param_groups_lrd(m, wd, no_weight_decay_list=m.no_weight_decay(), layer_decay=ld), lr=lr)
    assert len(opt.param_groups) > 3 and all('lr_scale' in g for g in opt.param_groups)
    norms, inner = [], opt.norm_clip_step

    def recording(max_norm=None):
        want = float(get_grad_norm_(list(m.parameters())))
        got = inner(max_norm)
        norms.append((float(got), want))
        return got

    opt.norm_clip_step = recording
    crit = SoftCrossEntropyWithWeightsLoss(torch.from_numpy(gold['class_weights'])).cuda()
    stats = train_one_epoch(m, crit, batches, opt, torch.device('cuda'), int(epoch), NativeScalerWithGradNormCount(),
                            max_norm=None, args=args)
    print('epoch stats', stats, 'reference', float(gold['epoch/loss']), float(gold['epoch/lr']), 'norms', norms)
    assert len(norms) == 1 and opt.applied_steps() == 1                  # two batches, one step: the branch was taken, once
    assert abs(norms[0][0] - norms[0][1]) <= 1e-6 * norms[0][1]
    assert abs(stats['loss'] - float(gold['epoch/loss'])) <= 1e-4 * float(gold['epoch/loss'])
    assert abs(stats['lr'] - float(gold['epoch/lr'])) <= 1e-12 + 1e-9 * float(gold['epoch/lr'])
    worst = (0.0, None)
    D, n_layers = m.embed_dim, len(m.blocks) + 1
    for n, p in m.named_parameters():
        got, ref = (p.detach().cpu() - before[n]).numpy(), gold[f'epoch/delta/{n}']
        if n.endswith('attn.qkv.bias'):
            step = lr * ld ** (n_layers - get_layer_id_for_vit(n, n_layers))
            assert np.abs(got[D:2 * D]).max() <= step * (1 + 1e-6), n
            got, ref = np.delete(got, np.s_[D:2 * D]), np.delete(ref, np.s_[D:2 * D])
        e = _rel(got, ref)
        print(f'epoch delta {n}: relative L2 error {e:.3e}')
        worst = max(worst, (e, n))
    assert worst[0] <= 1e-4, worst
    assert all(p.grad is None or float(p.grad.abs().sum()) == 0 for p in m.parameters())


@gpu
@pytest.mark.parametrize('gp', [False, True])
def test_frozen_parameters_stay_bit_equal_and_get_no_state(gold, x_micro, gp):
    from vit_ae_plus_plus_amd.optim import MultiTensorAdamW
    x, y = x_micro.cuda(), torch.from_numpy(gold['labels']).cuda()
    crit = torch.nn.CrossEntropyLoss(weight=torch.from_numpy(gold['class_weights']).cuda())
    frozen_sets = {'head only (--fix_backbone)': lambda n: not n.startswith('head.'),
                   'embedding and block 0': lambda n: n.startswith(('patch_embed.', 'blocks.0.')) or n in ('pos_embed', 'cls_token')}
    for label, frozen in frozen_sets.items():
        m = _micro(gp)
        for n, p in m.named_parameters():
            p.requires_grad = not frozen(n)
        before = {n: p.detach().clone() for n, p in m.named_parameters()}
        opt = MultiTensorAdamW(m.parameters(), lr=1e-3, weight_decay=0.05)
        losses = _losses(m, opt, x, y, crit, steps=2)
        assert losses[1] < losses[0], (label, losses)
        live = [n for n, _ in m.named_parameters() if not frozen(n)]
        if label.startswith('head'):
            assert sorted(live) == ['head.bias', 'head.weight']          # two tensors
        for n, p in m.named_parameters():
            if frozen(n):
                assert torch.equal(p.detach().view(torch.int32), before[n].view(torch.int32)) and not opt.state.get(p), (label, n)
            else:
                assert not torch.equal(p.detach(), before[n]) and set(opt.state[p]) == {'step', 'exp_avg', 'exp_avg_sq'}, (label, n)
        assert opt.applied_steps() == 2
