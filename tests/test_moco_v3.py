"""MoCo v3 (ABI 55): the four launch groups of csrc/moco.hip / csrc/norm.hip through the C ABI, and the CPU side of
``other_baselines.mocov3.moco`` (surface, state dicts, tables, refusals).  The model tests are in tests/test_moco_v3_model.py.

References are float64 statements written out here (``ema32``, ``loss_ref``, ``lars_ref``, ``bn_ref``); ``test_restatement_reproduces_the_
float64_fixture`` holds the loss and LARS ones against the reference's own float64 run (tests/golden/moco_v3.npz), so this file's
yardstick is the reference, not itself.

Bound, the project's rule (tests/test_norm_kernels.py, tests/test_loss_kernels.py): e <= max(3 e32, 4 2^-24), e32 the same figure of
the plain fp32 torch statement on the same inputs (CPU).  Figures:
  loss scalar   |l - l64| / |l64| (absolute where l64 = 0: N = 1 owes an exact zero)
  dq            per row, max_c |dq - dq64| / max_c |dq64|
  LARS          per tensor, |p - p64| / |p64 - p0| and |mu - mu64| / |mu64| (2-norms) after 3 steps, the rule of tests/test_multi_adamw.py:
                tensors of fewer than POOL_BELOW elements are judged together as one vector (the rounding of 1 .. 7 numbers is exactly
                zero for a good share of them, and the ratio of two such figures says nothing)
  BatchNorm     per element |y - y64| / (|xhat w| + |b|), dx against its first-order scale rstd |w| (|dy| + mean|dy| + |xhat| mean|dy xhat|);
                the maximum of every row and of every column obeys the rule with e32 of that row / column.  Statistics and dw / db
                per column, relative.
EMA is not a tolerance: it is bit-equal to the fp32 statement.

Every output lives between GUARD sentinel elements no launch may touch; outputs start as NaN; inputs sit between NaN."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'moco_v3.npz')
GUARD, SENT = 64, 7.25
FACTOR, FLOOR = 3.0, 4.0 * 2.0 ** -24
POOL_BELOW = 64
NORM_EPS = 1e-12
F32, F64 = torch.float32, torch.float64


def _consts():
    from vit_ae_plus_plus_amd._abi import CONSTS
    return CONSTS


def _chunk():
    return _consts()['VITAE_MULTI_CHUNK']


def rule(e, e32):
    return e <= max(FACTOR * e32, FLOOR)


# =========================================================================== float64 statements
def ema32(pm, pb, m):
    """the momentum update's statement in fp32 (numpy: two rounded products, one rounded sum)"""
    return pm * np.float32(m) + pb * np.float32(1. - m)


def loss_ref(q1, k2, q2, k1, T, dtype=np.float64):
    """-> (loss, dq1, dq2): both InfoNCE terms and the query gradients, the clamped norm a constant"""
    def term(q, k):
        q, k = q.astype(dtype), k.astype(dtype)
        nq = np.maximum(np.sqrt((q * q).sum(1, keepdims=True)), dtype(NORM_EPS))
        nk = np.maximum(np.sqrt((k * k).sum(1, keepdims=True)), dtype(NORM_EPS))
        qn, kn = q / nq, k / nk
        logits = qn @ kn.T / dtype(T)
        N = q.shape[0]
        z = logits - logits.max(1, keepdims=True)
        ez = np.exp(z)
        lse = np.log(ez.sum(1, keepdims=True))
        loss = -(z - lse)[np.arange(N), np.arange(N)].mean() * dtype(2 * T)
        dlogits = (ez / ez.sum(1, keepdims=True) - np.eye(N, dtype=dtype)) * dtype(2 * T) / N
        dqn = dlogits @ kn / dtype(T)
        clamped = np.sqrt((q * q).sum(1, keepdims=True)) <= NORM_EPS
        dq = np.where(clamped, dqn / nq, (dqn - qn * (qn * dqn).sum(1, keepdims=True)) / nq)
        return loss, dq
    l1, d1 = term(q1, k2)
    l2, d2 = term(q2, k1)
    return l1 + l2, d1, d2


def loss_torch32(q1, k2, q2, k1, T):
    """the reference's statement on fp32 torch tensors (CPU), gradients by autograd"""
    def term(q, k):
        qn, kn = F.normalize(q, dim=1), F.normalize(k, dim=1)
        logits = torch.einsum('nc,mc->nm', [qn, kn]) / T
        return F.cross_entropy(logits, torch.arange(q.shape[0])) * (2 * T)
    a, b = torch.from_numpy(q1).requires_grad_(), torch.from_numpy(q2).requires_grad_()
    loss = term(a, torch.from_numpy(k2)) + term(b, torch.from_numpy(k1))
    loss.backward()
    return float(loss.detach()), a.grad.numpy(), b.grad.numpy()


def lars_ref(p, g, mu, scaled, lr, wd, mom, trust, dtype=np.float64):
    """one LARS step of one tensor -> (p, mu)"""
    p, g, mu = p.astype(dtype), g.astype(dtype), mu.astype(dtype)
    dp = g
    if scaled:
        dp = g + dtype(wd) * p
        pn, un = np.sqrt((p * p).sum()), np.sqrt((dp * dp).sum())
        q = dtype(trust) * pn / un if (pn > 0 and un > 0) else dtype(1)
        dp = dp * q
    mu = mu * dtype(mom) + dp
    return p - dtype(lr) * mu, mu


def lars_torch32(p, g, mu, scaled, lr, wd, mom, trust):
    """the same step as torch statements on fp32 CPU tensors"""
    p, g, mu = torch.from_numpy(p.copy()), torch.from_numpy(g), torch.from_numpy(mu.copy())
    dp = g
    if scaled:
        dp = g.add(p, alpha=wd)
        pn, un = torch.norm(p), torch.norm(dp)
        q = trust * pn / un if (pn > 0 and un > 0) else torch.ones_like(pn)
        dp = dp.mul(q)
    mu.mul_(mom).add_(dp)
    p.add_(mu, alpha=-lr)
    return p.numpy(), mu.numpy()


def bn_ref(x, w, b, rm, rv, eps, momentum, dy=None, dtype=F64):
    """training-mode BatchNorm1d -> dict(y, mean, rstd, rm, rv, [dx, dw, db]) in `dtype` (torch; autograd for the backward)"""
    x = x.detach().clone().to(dtype).requires_grad_(dy is not None)
    wt = None if w is None else w.detach().clone().to(dtype).requires_grad_(dy is not None)
    bt = None if b is None else b.detach().clone().to(dtype).requires_grad_(dy is not None)
    rm, rv = rm.to(dtype).clone(), rv.to(dtype).clone()
    y = F.batch_norm(x, rm, rv, wt, bt, True, momentum, eps)
    xd = x.detach()
    mean, var = xd.mean(0), xd.var(0, unbiased=False)
    out = {'y': y.detach(), 'mean': mean, 'rstd': (var + eps).rsqrt(), 'rm': rm, 'rv': rv}
    if dy is not None:
        y.backward(dy.to(dtype))
        out.update(dx=x.grad, dw=None if wt is None else wt.grad, db=None if bt is None else bt.grad)
    return out


# =========================================================================== CPU
NEW_PROTOS = {
    'vitae_ema_multi': ('int', ['ptr', 'ptr', 'long', 'ptr', 'ptr', 'long', 'long', 'double', 'ptr']),
    'vitae_lars_multi': ('int', ['ptr', 'ptr', 'long', 'ptr', 'ptr', 'long', 'long', 'ptr', 'int', 'ptr', 'ptr']),
    'vitae_moco_loss_ws_floats': ('long', ['int', 'int']),
    'vitae_moco_loss': ('int', ['ptr', 'ptr', 'ptr', 'ptr', 'int', 'int', 'double', 'ptr', 'ptr', 'ptr', 'ptr', 'ptr']),
    'vitae_bn1d_fwd': ('int', ['ptr'] * 10 + ['int', 'int', 'float', 'float', 'ptr']),
    'vitae_bn1d_eval': ('int', ['ptr'] * 6 + ['int', 'int', 'float', 'ptr']),
    'vitae_bn1d_bwd': ('int', ['ptr'] * 9 + ['int', 'int', 'ptr']),
    'vitae_layernorm_bwd_part_any': ('int', ['ptr'] * 8 + ['int', 'int', 'int', 'ptr']),
    'vitae_colsum_ordered_ws_floats': ('long', ['int', 'int']),
    'vitae_colsum_ordered': ('int', ['ptr', 'long', 'ptr', 'ptr', 'int', 'int', 'ptr']),
}


def test_header_abi_and_library_agree():
    from vit_ae_plus_plus_amd import _abi
    protos, consts = _abi.parse_header()
    assert consts['VITAE_ABI_VERSION'] >= 55
    dll = ctypes.CDLL(_abi.LIB_PATH)
    assert dll.vitae_abi_version() == consts['VITAE_ABI_VERSION']
    for name, proto in NEW_PROTOS.items():
        assert protos[name] == proto and _abi.PROTOS[name] == proto, name
        getattr(dll, name)
    assert consts['VITAE_MOCO_MAX_N'] >= 1024 and consts['VITAE_MOCO_MAX_C'] >= 4096 and consts['VITAE_LARS_FLAG_SCALED'] == 1
    dll.vitae_moco_loss_ws_floats.restype = ctypes.c_long
    assert dll.vitae_moco_loss_ws_floats(8, 32) > 0 and dll.vitae_moco_loss_ws_floats(0, 32) == 0


def test_dropin_exposes_the_baseline():
    import sys
    from vit_ae_plus_plus_amd import dropin
    saved = {k: sys.modules.get(k) for k in dropin._ALIASES}
    try:
        dropin.install(force=True)
        import other_baselines.mocov3.moco.builder as b
        import other_baselines.mocov3.moco.optimizer as o
        import vit_ae_plus_plus_amd.other_baselines.mocov3.moco.builder as b2
        assert b is b2 and callable(b.MoCo_ViT) and callable(b.MoCo) and issubclass(o.LARS, torch.optim.Optimizer)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def micro_model(T=1.0, **kw):
    from functools import partial
    from vit_ae_plus_plus_amd.model.vit import VisionTransformer3D
    from vit_ae_plus_plus_amd.other_baselines.mocov3.moco.builder import MoCo_ViT
    enc = partial(VisionTransformer3D, volume_size=8, patch_size=4, in_chans=1, embed_dim=64, depth=2, num_heads=2, **kw)
    return MoCo_ViT(enc, 32, 64, T)


def test_state_dict_keys_and_shapes_are_the_references():
    z = np.load(GOLD)
    sd = micro_model().state_dict()
    assert list(sd.keys()) == [str(n) for n in z['names']]
    assert [','.join(str(s) for s in v.shape) for v in sd.values()] == [str(s) for s in z['shapes']]
    for k in ('base_encoder.head.0.weight', 'base_encoder.head.7.running_mean', 'momentum_encoder.head.6.weight', 'predictor.4.running_var'):
        assert k in sd
    assert 'base_encoder.head.7.weight' not in sd and 'predictor.4.weight' not in sd          # affine=False
    m = micro_model()
    assert not any(p.requires_grad for p in m.momentum_encoder.parameters())
    assert all(torch.equal(a, b) for a, b in zip(m.base_encoder.parameters(), m.momentum_encoder.parameters()))
    # what main_extract_ssl_features.py does with a checkpoint: strip 'base_encoder.' and load into a plain encoder
    from vit_ae_plus_plus_amd.model.vit import VisionTransformer3D
    plain = VisionTransformer3D(volume_size=8, patch_size=4, in_chans=1, embed_dim=64, depth=2, num_heads=2, num_classes=0)
    stripped = {k[len('base_encoder.'):]: v for k, v in sd.items() if k.startswith('base_encoder.') and not k.startswith('base_encoder.head')}
    missing, unexpected = plain.load_state_dict(stripped, strict=False)
    assert not missing and not unexpected


def test_moco_resnet_raises():
    from vit_ae_plus_plus_amd.other_baselines.mocov3.moco.builder import MoCo_ResNet
    with pytest.raises(NotImplementedError):
        MoCo_ResNet(lambda num_classes: None)


def test_lars_state_dict_round_trip_and_reference_format():
    from vit_ae_plus_plus_amd.other_baselines.mocov3.moco.optimizer import LARS
    g = torch.Generator().manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((5, 3), (7,), (2, 2, 2))]
    opt = LARS(ps, 0.3, weight_decay=1e-2, momentum=0.8)
    assert opt.defaults == dict(lr=0.3, weight_decay=1e-2, momentum=0.8, trust_coefficient=0.001)
    # a state dict in the reference's format: what torch.optim.Optimizer.state_dict() packs for state {'mu'}
    ref_sd = {'state': {i: {'mu': torch.randn(p.shape, generator=g)} for i, p in enumerate(ps)},
              'param_groups': [{'lr': 0.1, 'weight_decay': 0.5, 'momentum': 0.7, 'trust_coefficient': 0.002, 'params': [0, 1, 2]}]}
    opt.load_state_dict(ref_sd)
    assert opt.param_groups[0]['lr'] == 0.1 and opt.param_groups[0]['trust_coefficient'] == 0.002
    for i, p in enumerate(ps):
        assert set(opt.state[p]) == {'mu'} and torch.equal(opt.state[p]['mu'], ref_sd['state'][i]['mu'])
    back = opt.state_dict()
    assert back['param_groups'][0]['params'] == [0, 1, 2] and set(back['state']) == {0, 1, 2}
    opt2 = LARS(ps, 9.0)
    opt2.load_state_dict(back)
    assert all(torch.equal(opt2.state[p]['mu'], opt.state[p]['mu']) for p in ps) and opt2.param_groups[0]['momentum'] == 0.7


def test_cpu_tensors_raise():
    from vit_ae_plus_plus_amd._abi import VitaeError
    from vit_ae_plus_plus_amd.other_baselines.mocov3.moco.optimizer import LARS
    m = micro_model()
    x = torch.zeros(2, 1, 8, 8, 8)
    with pytest.raises(VitaeError):
        m(x, x, 0.99)
    with pytest.raises(VitaeError):
        m.contrastive_loss(torch.zeros(2, 4), torch.zeros(2, 4))
    with pytest.raises(VitaeError):
        m._update_momentum_encoder(0.5)
    opt = LARS(m.parameters(), 0.3)
    opt.step()                                   # no gradient anywhere: nothing to do, nothing raised
    snap = [p.detach().clone() for p in m.parameters()]
    for p in m.parameters():
        if p.requires_grad:
            p.grad = torch.ones_like(p)
    with pytest.raises(VitaeError):
        opt.step()
    assert all(torch.equal(a, b) for a, b in zip(snap, m.parameters()))


def list_lengths():
    c = _chunk()
    return [1, 3, 4, 5, c - 1, c, c + 1, 2 * c + 1]


def test_tables_cover_every_element_once():
    """The EMA and LARS tables over the chunk list: every element of every tensor is in exactly one (tensor, chunk) pair, and the
    pairs are in tensor order with a tensor's chunks ascending — what vitae_lars_multi's second launch relies on."""
    from vit_ae_plus_plus_amd.optim import multi_chunk_list
    from vit_ae_plus_plus_amd.other_baselines.mocov3.moco.optimizer import ema_table, lars_table
    c = _chunk()
    lengths = list_lengths() + [7] * 40
    pairs = multi_chunk_list(lengths, c)
    cover = [np.zeros(n, dtype=np.int64) for n in lengths]
    for t, k in pairs:
        cover[t][k * c:min(lengths[t], (k + 1) * c)] += 1
    assert all((cv == 1).all() for cv in cover)
    order = [(int(t), int(k)) for t, k in pairs]
    assert order == sorted(order) and all(k == 0 or order[i - 1] == (t, k - 1) for i, (t, k) in enumerate(order))
    ids = list(range(100, 100 + len(lengths)))
    scaled = [i % 2 == 0 for i in range(len(lengths))]
    table = lars_table(ids, ids, ids, scaled, lengths, np.arange(len(lengths)) % 3)
    assert table.shape == (len(lengths), 6) and table.dtype == np.int64
    assert (table[:, 3] == np.array(scaled, dtype=np.int64)).all() and (table[:, 4] == lengths).all() and (table[:, 5] == np.arange(len(lengths)) % 3).all()
    # the momentum update's table: (pm, pb, 0, 0, n, 0) per pair, and every element of every pair in exactly one chunk of it
    pm_ids, pb_ids = [1000 + 16 * i for i in range(len(lengths))], [9000 + 16 * i for i in range(len(lengths))]
    et = ema_table(pm_ids, pb_ids, lengths)
    assert et.shape == (len(lengths), 6) and et.dtype == np.int64
    assert (et[:, 0] == pm_ids).all() and (et[:, 1] == pb_ids).all() and (et[:, 4] == lengths).all() and not et[:, [2, 3, 5]].any()
    seen = [np.zeros(n, dtype=np.int64) for n in lengths]
    for t, k in pairs:
        seen[t][k * c:min(int(et[t, 4]), (k + 1) * c)] += 1
    assert all((sv == 1).all() for sv in seen)


def test_restatement_reproduces_the_float64_fixture():
    z = np.load(GOLD)
    lr, wd, mom = (float(v) for v in z['lars'])
    for T in z['temps']:
        tag = f'T{float(T)}/f64/'
        loss, dq1, dq2 = loss_ref(z[tag + 'q1'], z[tag + 'k2'], z[tag + 'q2'], z[tag + 'k1'], float(T))
        assert abs(loss - float(z[tag + 'loss'])) <= 1e-12 * abs(float(z[tag + 'loss']))
        for got, want in ((dq1, z[tag + 'dq1']), (dq2, z[tag + 'dq2'])):
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        for n in z['f64/lars_names']:
            pre = f'{tag}lars/{n}/'
            p, mu = lars_ref(z[pre + 'p'], z[pre + 'g'], np.zeros_like(z[pre + 'p']), z[pre + 'p'].ndim > 1, lr, wd, mom, 0.001)
            assert np.abs(p - z[pre + 'p_after']).max() <= 1e-12 * np.abs(z[pre + 'p_after']).max(), n
            assert np.abs(mu - z[pre + 'mu_after']).max() <= 1e-12 * np.abs(z[pre + 'mu_after']).max(), n


# =========================================================================== GPU plumbing
def dev():
    return torch.device('cuda')


class Guarded:
    """a [n] fp32 device array between GUARD sentinels (`guard`), `off` floats away from 16-byte alignment"""

    def __init__(self, data, guard=SENT, off=0, dtype=np.float32):
        data = np.ascontiguousarray(data, dtype=dtype).reshape(-1)
        self.n, self.off, self.guard = data.size, off, guard
        host = np.full(2 * GUARD + off + data.size, guard, dtype=dtype)
        host[GUARD + off:GUARD + off + data.size] = data
        self.buf = torch.from_numpy(host).to(dev())
        assert self.buf.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.buf.element_size() * (GUARD + self.off)

    def get(self):
        return self.buf.cpu().numpy()[GUARD + self.off:GUARD + self.off + self.n].copy()

    def guards_intact(self):
        h = self.buf.cpu().numpy()
        edge = np.concatenate([h[:GUARD + self.off], h[GUARD + self.off + self.n:]])
        return bool(np.isnan(edge).all()) if np.isnan(self.guard) else bool((edge == self.guard).all())


def inp(data, off=0):
    return Guarded(data, guard=np.nan, off=off)


def outp(n, off=0):
    return Guarded(np.full(n, np.nan, dtype=np.float32), off=off)


def stream():
    return torch.cuda.current_stream().cuda_stream


def send_table(table, lengths, hyper=()):
    """host and device copies of [table], [hyper] and the chunk list -> kwargs-like tuple for the launchers"""
    from vit_ae_plus_plus_amd.optim import multi_chunk_list
    chunks = np.ascontiguousarray(multi_chunk_list(lengths, _chunk()))
    keep = {'table': np.ascontiguousarray(table), 'chunks': chunks,
            'table_d': torch.from_numpy(np.ascontiguousarray(table)).to(dev()) if len(table) else torch.zeros(1, dtype=torch.int64, device=dev()),
            'chunks_d': torch.from_numpy(chunks).to(dev()) if len(chunks) else torch.zeros(2, dtype=torch.int32, device=dev()),
            'hyper_d': torch.tensor(list(hyper) or [0.0], dtype=torch.float32, device=dev())}
    args = (keep['table'].ctypes.data if len(table) else None, keep['table_d'].data_ptr(), len(table),
            chunks.ctypes.data if len(chunks) else None, keep['chunks_d'].data_ptr(), len(chunks), _chunk())
    return args, keep


def raw(name):
    """the entry point without the status check (to read refusal codes)"""
    from vit_ae_plus_plus_amd._abi import lib
    return getattr(lib.load(), name)


# =========================================================================== EMA
def _ema_case(lengths, m, off=0, seed=0):
    from vit_ae_plus_plus_amd._abi import lib
    rng = np.random.default_rng(seed)
    pms = [rng.standard_normal(n).astype(np.float32) for n in lengths]
    pbs = [rng.standard_normal(n).astype(np.float32) for n in lengths]
    gm = [Guarded(a, off=off) for a in pms]            # pm is input and output: sentinels around it
    gb = [inp(a, off=off) for a in pbs]
    table = np.zeros((len(lengths), 6), dtype=np.int64)
    table[:, 0], table[:, 1], table[:, 4] = [x.ptr for x in gm], [x.ptr for x in gb], lengths
    args, keep = send_table(table, lengths)
    lib.vitae_ema_multi(*args, float(m), stream())
    torch.cuda.synchronize()
    for t, (a, b) in enumerate(zip(pms, pbs)):
        got = gm[t].get()
        assert np.array_equal(got.view(np.uint32), ema32(a, b, m).view(np.uint32)), (t, lengths[t], m)
        # (the numpy statement is torch's: what the reference's `param_m.data * m + param_b.data * (1. - m)` computes on fp32 tensors)
        want = torch.from_numpy(a) * m + torch.from_numpy(b) * (1. - m)
        assert np.array_equal(got.view(np.uint32), want.numpy().view(np.uint32)), (t, lengths[t], m)
        assert gm[t].guards_intact() and gb[t].guards_intact() and np.array_equal(gb[t].get().view(np.uint32), b.view(np.uint32))
    return pms, pbs, gm


@pytest.mark.gpu
@pytest.mark.parametrize('m', [0.0, 0.5, 0.99, 0.996, 0.9999, 1.0])
def test_ema_bit_equal_to_the_statement(m):
    pms, pbs, gm = _ema_case(list_lengths(), m)
    if m == 1.0:
        assert all(np.array_equal(g.get().view(np.uint32), a.view(np.uint32)) for g, a in zip(gm, pms))
    if m == 0.0:
        assert all(np.array_equal(g.get(), b) for g, b in zip(gm, pbs))


@pytest.mark.gpu
def test_ema_one_tensor_forty_tensors_and_misaligned():
    _ema_case([2 * _chunk() + 1], 0.99)
    mixed = (list_lengths() * 5)[:40]
    _ema_case(mixed, 0.996, seed=1)
    _ema_case(list_lengths(), 0.99, off=1, seed=2)


@pytest.mark.gpu
def test_ema_empty_table_and_refusals():
    from vit_ae_plus_plus_amd._abi import lib
    args, keep = send_table(np.zeros((0, 6), dtype=np.int64), [])
    lib.vitae_ema_multi(*args, 0.5, stream())                       # no-op
    fn = raw('vitae_ema_multi')
    pm, pb = Guarded(np.ones(8)), inp(np.ones(8))
    table = np.array([[pm.ptr, pb.ptr, 0, 0, 8, 0]], dtype=np.int64)
    args, keep = send_table(table, [8])
    bad_table = table.copy(); bad_table[0, 1] = 0
    bad_chunks = np.array([[0, 1]], dtype=np.int32)
    assert fn(*args, 1.5, stream()) == -1 and fn(*args, float('nan'), stream()) == -1
    assert fn(bad_table.ctypes.data, *args[1:], 0.5, stream()) == -1
    assert fn(*args[:3], bad_chunks.ctypes.data, *args[4:], 0.5, stream()) == -1
    assert fn(*args[:6], 6, 0.5, stream()) == -1
    torch.cuda.synchronize()
    assert (pm.get() == 1).all() and pm.guards_intact()


# =========================================================================== loss
def _loss_launch(q1, k2, q2, k1, T, off=0):
    from vit_ae_plus_plus_amd._abi import lib
    N, C = q1.shape
    ins = [inp(a, off=off) for a in (q1, k2, q2, k1)]
    loss, dq1, dq2 = outp(1), outp(N * C, off=off), outp(N * C, off=off)
    ws = outp(int(lib.vitae_moco_loss_ws_floats(N, C)))
    lib.vitae_moco_loss(*(x.ptr for x in ins), N, C, float(T), loss.ptr, dq1.ptr, dq2.ptr, ws.ptr, stream())
    torch.cuda.synchronize()
    for x in ins + [loss, dq1, dq2, ws]:
        assert x.guards_intact()
    return loss.get()[0], dq1.get().reshape(N, C), dq2.get().reshape(N, C)


def _loss_check(q1, k2, q2, k1, T, tag, grads=True):
    got = _loss_launch(q1, k2, q2, k1, T)
    again = _loss_launch(q1, k2, q2, k1, T)
    assert all(np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32)) for a, b in zip(got, again)), 'repeats differ'
    l64, d1_64, d2_64 = loss_ref(q1, k2, q2, k1, T)
    l32, d1_32, d2_32 = loss_torch32(q1, k2, q2, k1, T)
    den = abs(l64) if l64 != 0 else 1.0
    e, e32 = abs(float(got[0]) - l64) / den, abs(l32 - l64) / den
    print(f'RATIO loss {tag}: e {e:.3g} e32 {e32:.3g}')
    assert np.isfinite(got[0]) and rule(e, e32), (tag, e, e32)
    for name, g, r64, r32 in () if not grads else (('dq1', got[1], d1_64, d1_32), ('dq2', got[2], d2_64, d2_32)):
        assert np.isfinite(g).all()
        scale = np.abs(r64).max(1)
        ok = scale > 0
        assert (g[~ok] == 0).all(), (tag, name, 'rows that owe an exact zero')
        er = np.abs(g - r64).max(1)[ok] / scale[ok]
        er32 = np.abs(r32 - r64).max(1)[ok] / scale[ok]
        if ok.any():
            print(f'RATIO {name} {tag}: e {er.max():.3g} e32 {er32.max():.3g}')
        bad = [(i, a, b) for i, (a, b) in enumerate(zip(er, er32)) if not rule(a, b)]
        assert not bad, (tag, name, bad[:4])
    return got


@pytest.mark.gpu
@pytest.mark.parametrize('T', [1.0, 0.2])
@pytest.mark.parametrize('N,C', [(1, 1), (2, 4), (3, 63), (8, 256), (33, 4), (65, 63), (33, 256), (2, 1)])
def test_loss_against_float64(N, C, T):
    rng = np.random.default_rng(N * 1000 + C)
    q1, k2, q2, k1 = (rng.standard_normal((N, C)).astype(np.float32) for _ in range(4))
    got = _loss_check(q1, k2, q2, k1, T, f'N{N} C{C} T{T}')
    if N == 1:
        assert got[0] == 0 and (got[1] == 0).all() and (got[2] == 0).all()


@pytest.mark.gpu
def test_loss_edge_cases():
    rng = np.random.default_rng(7)
    N, C = 8, 64
    q1, k2, q2, k1 = (rng.standard_normal((N, C)).astype(np.float32) for _ in range(4))
    # the clamp: a zero row and a row of norm 1e-20 among the queries and among the keys
    a, b = q1.copy(), k2.copy()
    a[2] = 0
    a[5] = 0; a[5, 3] = 1e-20
    b[1] = 0
    b[6] = 0; b[6, 0] = -1e-20
    _loss_check(a, b, q2, k1, 1.0, 'clamp')
    # q = k: the diagonal holds the maximum of every row (cos = 1), ties where rows repeat
    c = q1.copy(); c[4] = c[3]
    _loss_check(c, c.copy(), q2, q2.copy(), 0.2, 'q=k')
    # T = 0.005: logits reach +-200, exp overflows fp32 without the max subtraction
    got = _loss_check(q1, q1.copy(), q2, k1, 0.005, 'T0.005')
    assert np.isfinite(got[0])
    # all rows equal: uniform softmax, loss = 2 * (2 T ln N); the gradient is zero in exact arithmetic and round-off in any other
    row = rng.standard_normal((1, C)).astype(np.float32)
    e = np.repeat(row, N, 0)
    for T in (1.0, 0.2):
        got = _loss_check(e, e.copy(), e.copy(), e.copy(), T, f'equal T{T}', grads=False)
        want = 2 * 2 * T * np.log(N)
        assert rule(abs(float(got[0]) - want) / want, abs(loss_torch32(e, e, e, e, T)[0] - want) / want)
        assert np.isfinite(got[1]).all() and np.abs(got[1]).max() <= 1e-5 and np.abs(got[2]).max() <= 1e-5


@pytest.mark.gpu
def test_loss_refusals_write_nothing():
    c = _consts()
    fn = raw('vitae_moco_loss')
    x = inp(np.ones(16))
    loss, dq1, dq2, ws = outp(1), outp(16), outp(16), outp(1024)
    a = (x.ptr, x.ptr, x.ptr, x.ptr)
    o = (loss.ptr, dq1.ptr, dq2.ptr, ws.ptr, stream())
    assert fn(*a, c['VITAE_MOCO_MAX_N'] + 1, 4, 1.0, *o) == -2
    assert fn(*a, 4, c['VITAE_MOCO_MAX_C'] + 1, 1.0, *o) == -2
    assert fn(*a, 4, 4, 0.0, *o) == -1 and fn(*a, 4, 4, -1.0, *o) == -1 and fn(*a, 4, 4, float('nan'), *o) == -1
    assert fn(*a, 0, 4, 1.0, *o) == -1 and fn(None, *a[1:], 4, 4, 1.0, *o) == -1
    torch.cuda.synchronize()
    for t in (loss, dq1, dq2, ws):
        assert np.isnan(t.get()).all() and t.guards_intact()


@pytest.mark.gpu
def test_loss_autograd_node_scales_on_the_device():
    m = micro_model(T=0.2)
    g = torch.Generator().manual_seed(5)
    q, k = torch.randn(8, 32, generator=g), torch.randn(8, 32, generator=g)
    l64, d64, _ = loss_ref(q.numpy(), k.numpy(), q.numpy(), k.numpy(), 0.2)
    qd = q.to(dev()).requires_grad_()
    loss = m.contrastive_loss(qd, k.to(dev()))
    assert loss.dim() == 0 and loss.grad_fn is not None
    (loss * 3.0).backward()
    assert abs(float(loss) - l64 / 2) <= 1e-5 * l64
    assert np.abs(qd.grad.cpu().numpy() - 3.0 * d64).max() <= 1e-5 * np.abs(3.0 * d64).max()


# =========================================================================== LARS
GROUPS = [dict(lr=0.3, weight_decay=1e-2, momentum=0.9, trust_coefficient=0.001),
          dict(lr=0.05, weight_decay=0.0, momentum=0.5, trust_coefficient=0.01),
          dict(lr=1.2, weight_decay=0.1, momentum=0.0, trust_coefficient=0.002)]


def _lars_tensors(seed=0):
    """(name, p, scaled, group): chunk-boundary sizes as 2-D and 1-D tensors, single elements, the degenerate norms, 40 in all"""
    rng = np.random.default_rng(seed)
    c = _chunk()
    items = []
    for i, n in enumerate(list_lengths()):
        items.append((f'w{n}', rng.standard_normal(n).astype(np.float32) * 0.05, True, i % 3))
        items.append((f'v{n}', rng.standard_normal(n).astype(np.float32) * 0.05, False, (i + 1) % 3))
    items.append(('zero_p', np.zeros(300, dtype=np.float32), True, 0))
    items.append(('cancel', rng.standard_normal(300).astype(np.float32), True, 2))
    while len(items) < 40:
        n = 7 + len(items)
        items.append((f'small{len(items)}', rng.standard_normal(n).astype(np.float32), len(items) % 2 == 0, len(items) % 3))
    return items


def _lars_grads(items, step, seed=0):
    rng = np.random.default_rng(1000 + 17 * step + seed)
    gs = []
    for name, p, scaled, gi in items:
        g = rng.standard_normal(p.size).astype(np.float32) * 0.01
        gs.append(g)
    return gs


def _lars_run_gpu(items, steps=3, off=0, skip=()):
    from vit_ae_plus_plus_amd._abi import lib
    gp = [Guarded(p, off=off) for _, p, _, _ in items]
    gmu = [Guarded(np.zeros_like(p), off=off) for _, p, _, _ in items]
    live = [i for i, it in enumerate(items) if it[0] not in skip]
    lengths = [items[i][1].size for i in live]
    hyper = [float(g[k]) for k in ('lr', 'weight_decay', 'momentum', 'trust_coefficient') for g in GROUPS]
    all_grads = []
    for step in range(steps):
        grads = _lars_grads(items, step)
        for i, it in enumerate(items):
            if it[0] == 'cancel':           # g = -(wd p) in fp32, p as it is now: the update's norm is exactly 0
                grads[i] = -(np.float32(GROUPS[it[3]]['weight_decay']) * gp[i].get())
        all_grads.append(grads)
        gg = [inp(grads[i], off=off) for i in live]
        table = np.zeros((len(live), 6), dtype=np.int64)
        table[:, 0] = [gp[i].ptr for i in live]
        table[:, 1] = [x.ptr for x in gg]
        table[:, 2] = [gmu[i].ptr for i in live]
        table[:, 3] = [int(items[i][2]) for i in live]
        table[:, 4] = lengths
        table[:, 5] = [items[i][3] for i in live]
        args, keep = send_table(table, lengths, hyper)
        ws = Guarded(np.full(2 * args[5], np.nan), dtype=np.float64)
        lib.vitae_lars_multi(*args, keep['hyper_d'].data_ptr(), len(GROUPS), ws.ptr, stream())
        torch.cuda.synchronize()
        assert ws.guards_intact() and all(x.guards_intact() for x in gg)
    assert all(x.guards_intact() for x in gp + gmu)
    return [x.get() for x in gp], [x.get() for x in gmu], all_grads


@pytest.mark.gpu
@pytest.mark.parametrize('off', [0, 1])
def test_lars_against_float64_over_three_steps(off):
    items = _lars_tensors()
    p_got, mu_got, all_grads = _lars_run_gpu(items, off=off)
    p_again, mu_again, _ = _lars_run_gpu(items, off=off)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(p_got + mu_got, p_again + mu_again)), 'repeats differ'
    pool = {k: [] for k in ('p', 'p64', 'p32', 'p0', 'mu', 'mu64', 'mu32')}
    for i, (name, p0, scaled, gi) in enumerate(items):
        h = GROUPS[gi]
        hp = (h['lr'], h['weight_decay'], h['momentum'], h['trust_coefficient'])
        p64, mu64 = p0.astype(np.float64), np.zeros(p0.size)
        p32, mu32 = p0.copy(), np.zeros_like(p0)
        for step in range(3):
            g = all_grads[step][i]
            p64, mu64 = lars_ref(p64, g, mu64, scaled, *hp)
            p32, mu32 = lars_torch32(p32, g, mu32, scaled, *hp)
        if name == 'cancel':                # update norm 0 -> q = 1, dp = 0: nothing moves, exactly
            assert np.array_equal(p_got[i].view(np.uint32), p0.view(np.uint32)) and (mu_got[i] == 0).all()
            continue
        # ('zero_p': |p| = 0 -> q = 1, its first step is p = -lr g; judged like every other tensor)
        vals = dict(p=p_got[i], p64=p64, p32=p32, p0=p0.astype(np.float64), mu=mu_got[i], mu64=mu64, mu32=mu32)
        if p0.size < POOL_BELOW:
            for k, v in vals.items():
                pool[k].append(np.asarray(v, dtype=np.float64))
            continue
        _lars_judge(name, **vals)
    _lars_judge('pooled', **{k: np.concatenate(v) for k, v in pool.items()})


def _lars_judge(name, p, p64, p32, p0, mu, mu64, mu32):
    step = np.linalg.norm(p64 - p0)
    e, e32 = np.linalg.norm(p - p64) / step, np.linalg.norm(p32 - p64) / step
    em, em32 = np.linalg.norm(mu - mu64) / np.linalg.norm(mu64), np.linalg.norm(mu32 - mu64) / np.linalg.norm(mu64)
    print(f'RATIO lars {name}: p e {e:.3g} e32 {e32:.3g}  mu e {em:.3g} e32 {em32:.3g}')
    assert np.isfinite(p).all() and np.isfinite(mu).all()
    assert e <= FACTOR * e32 and em <= max(FACTOR * em32, FLOOR), (name, e, e32, em, em32)


@pytest.mark.gpu
def test_lars_unscaled_tensors_get_no_decay_and_no_scaling():
    """a 1-D tensor in a group with weight decay and a trust coefficient: p - lr (momentum 0 + g), bit for bit in fp32"""
    items = [('v', np.linspace(-1, 1, 4099).astype(np.float32), False, 0), ('w', np.ones(8, dtype=np.float32), True, 0)]
    p, mu, grads = _lars_run_gpu(items, steps=1)
    g = grads[0][0]
    assert np.array_equal(mu[0].view(np.uint32), g.view(np.uint32))
    assert np.array_equal(p[0].view(np.uint32), (items[0][1] - g * np.float32(0.3)).view(np.uint32))


@pytest.mark.gpu
def test_lars_refusals_write_nothing():
    fn = raw('vitae_lars_multi')
    p, g, mu = Guarded(np.ones(8)), inp(np.ones(8)), Guarded(np.zeros(8))
    table = np.array([[p.ptr, g.ptr, mu.ptr, 1, 8, 0]], dtype=np.int64)
    args, keep = send_table(table, [8], [0.3, 0.0, 0.9, 0.001])
    ws = Guarded(np.full(2, np.nan), dtype=np.float64)
    hd = keep['hyper_d'].data_ptr()
    t_group, t_null = table.copy(), table.copy()
    t_group[0, 5] = 1
    t_null[0, 2] = 0
    assert fn(t_group.ctypes.data, *args[1:], hd, 1, ws.ptr, stream()) == -1
    assert fn(t_null.ctypes.data, *args[1:], hd, 1, ws.ptr, stream()) == -1
    assert fn(*args, hd, 0, ws.ptr, stream()) == -1 and fn(*args, hd, 65, ws.ptr, stream()) == -1
    assert fn(*args, None, 1, ws.ptr, stream()) == -1 and fn(*args, hd, 1, None, stream()) == -1
    two = np.array([[p.ptr, g.ptr, mu.ptr, 1, 2 * _chunk(), 0]], dtype=np.int64)
    out_of_order = np.array([[0, 1], [0, 0]], dtype=np.int32)
    incomplete = np.array([[0, 0]], dtype=np.int32)
    assert fn(two.ctypes.data, args[1], 1, out_of_order.ctypes.data, args[4], 2, _chunk(), hd, 1, ws.ptr, stream()) == -1
    assert fn(two.ctypes.data, args[1], 1, incomplete.ctypes.data, args[4], 1, _chunk(), hd, 1, ws.ptr, stream()) == -1
    torch.cuda.synchronize()
    assert (p.get() == 1).all() and (mu.get() == 0).all() and np.isnan(ws.get()).all()
    assert p.guards_intact() and mu.guards_intact() and ws.guards_intact()


@pytest.mark.gpu
def test_lars_optimizer_skips_missing_grads_and_bumps_versions():
    from vit_ae_plus_plus_amd.other_baselines.mocov3.moco.optimizer import LARS
    g = torch.Generator().manual_seed(2)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g).to(dev())) for s in ((33, 5), (7,), (4, 4), (3,))]
    opt = LARS([{'params': ps[:2]}, {'params': ps[2:], 'lr': 0.05, 'weight_decay': 0.0}], 0.3, weight_decay=1e-2, momentum=0.9)
    before = [p.detach().cpu().numpy().copy() for p in ps]
    grads = [torch.randn(p.shape, generator=g) * 0.01 for p in ps]
    for i, p in enumerate(ps):
        if i != 2:
            p.grad = grads[i].to(dev())
    versions = [p._version for p in ps]
    opt.step()
    torch.cuda.synchronize()
    assert torch.equal(ps[2].detach().cpu(), torch.from_numpy(before[2])) and 'mu' not in opt.state[ps[2]] and ps[2]._version == versions[2]
    for i in (0, 1, 3):
        assert ps[i]._version > versions[i]
        h = opt.param_groups[0 if i < 2 else 1]
        want, mu = lars_ref(before[i].reshape(-1), grads[i].numpy().reshape(-1), np.zeros(before[i].size), ps[i].ndim > 1, h['lr'],
                            h['weight_decay'], h['momentum'], h['trust_coefficient'])
        assert np.abs(ps[i].detach().cpu().numpy().reshape(-1) - want).max() <= 1e-6 * np.abs(want).max()
        assert np.abs(opt.state[ps[i]]['mu'].cpu().numpy().reshape(-1) - mu).max() <= 1e-6 * np.abs(mu).max()


# =========================================================================== plain BatchNorm
BN_EPS, BN_MOM = 1e-5, 0.1


def _bn_inputs(R, D, affine, offset, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, D, generator=g) + (1000.0 if offset else 0.0)
    w = (1.0 + 0.3 * torch.randn(D, generator=g)) if affine else None
    b = (0.2 * torch.randn(D, generator=g)) if affine else None
    rm, rv = torch.randn(D, generator=g), torch.rand(D, generator=g) + 0.5
    dy = torch.randn(R, D, generator=g)
    return x, w, b, rm, rv, dy


def _rows_and_columns(tag, e, e32):
    """e, e32: [R, D] figures; the maximum of every row and of every column obeys the rule"""
    for axis, what in ((1, 'row'), (0, 'column')):
        a, b = e.max(axis), e32.max(axis)
        bad = [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if not rule(x, y)]
        assert not bad, (tag, what, bad[:4])
    print(f'RATIO bn {tag}: e {e.max():.3g} e32 {e32.max():.3g}')


def _col_rule(tag, got, r64, r32, scale=None):
    scale = r64.abs() if scale is None else scale
    e, e32 = (got.double() - r64).abs() / scale, (r32.double() - r64).abs() / scale
    bad = [(i, float(a), float(b)) for i, (a, b) in enumerate(zip(e, e32)) if not rule(float(a), float(b))]
    assert not bad, (tag, bad[:4])


@pytest.mark.gpu
@pytest.mark.parametrize('offset', [False, True])
@pytest.mark.parametrize('affine', [True, False])
@pytest.mark.parametrize('R,D', [(2, 4), (8, 64), (33, 68), (8, 68), (33, 4)])
def test_plain_batchnorm(R, D, affine, offset):
    from vit_ae_plus_plus_amd._abi import lib
    tag = f'R{R} D{D} affine{int(affine)} offset{int(offset)}'
    x, w, b, rm, rv, dy = _bn_inputs(R, D, affine, offset, R * 100 + D)
    r64 = bn_ref(x, w, b, rm, rv, BN_EPS, BN_MOM, dy)
    r32 = bn_ref(x, w, b, rm, rv, BN_EPS, BN_MOM, dy, dtype=F32)
    gx, gdy = inp(x.numpy()), inp(dy.numpy())
    gw, gb = (inp(w.numpy()), inp(b.numpy())) if affine else (None, None)
    y, mean, rstd, dx = outp(R * D), outp(D), outp(D), outp(R * D)
    grm, grv = Guarded(rm.numpy()), Guarded(rv.numpy())
    nbt = torch.full((3,), 5, dtype=torch.int64, device=dev())
    dw, db = (Guarded(np.zeros(D)), Guarded(np.zeros(D))) if affine else (None, None)
    P = lambda t: None if t is None else t.ptr
    lib.vitae_bn1d_fwd(gx.ptr, P(gw), P(gb), y.ptr, None, mean.ptr, rstd.ptr, grm.ptr, grv.ptr, nbt.data_ptr() + 8, R, D, BN_EPS, BN_MOM, stream())
    lib.vitae_bn1d_bwd(gdy.ptr, gx.ptr, P(gw), mean.ptr, rstd.ptr, dx.ptr, None, P(dw), P(db), R, D, stream())
    torch.cuda.synchronize()
    for t in [gx, gdy, y, mean, rstd, dx, grm, grv] + ([gw, gb, dw, db] if affine else []):
        assert t.guards_intact()
    assert nbt.tolist() == [5, 6, 5]
    T = lambda t, shape: torch.from_numpy(t.get()).reshape(shape)
    wa = (w if affine else torch.ones(D)).double()
    ba = (b if affine else torch.zeros(D)).double()
    xhat = (x.double() - r64['mean']) * r64['rstd']
    # y
    scale = (xhat * wa).abs() + ba.abs()
    got = T(y, (R, D))
    assert torch.isfinite(got).all()
    _rows_and_columns(tag + ' y', ((got.double() - r64['y']).abs() / scale).numpy(), ((r32['y'].double() - r64['y']).abs() / scale).numpy())
    # saved and running statistics
    _col_rule(tag + ' mean', T(mean, (D,)), r64['mean'], r32['mean'], scale=x.double().abs().mean(0))
    _col_rule(tag + ' rstd', T(rstd, (D,)), r64['rstd'], r32['rstd'])
    _col_rule(tag + ' running_mean', T(grm, (D,)), r64['rm'], r32['rm'], scale=0.9 * rm.double().abs() + 0.1 * x.double().abs().mean(0))
    _col_rule(tag + ' running_var', T(grv, (D,)), r64['rv'], r32['rv'])
    # dx, dw, db
    dyd = dy.double()
    sdx = r64['rstd'] * wa.abs() * (dyd.abs() + dyd.abs().mean(0) + xhat.abs() * (dyd * xhat).abs().mean(0))
    got = T(dx, (R, D))
    assert torch.isfinite(got).all()
    _rows_and_columns(tag + ' dx', ((got.double() - r64['dx']).abs() / sdx).numpy(), ((r32['dx'].double() - r64['dx']).abs() / sdx).numpy())
    if affine:
        _col_rule(tag + ' dw', T(dw, (D,)), r64['dw'], r32['dw'], scale=(dyd * xhat).abs().sum(0))
        _col_rule(tag + ' db', T(db, (D,)), r64['db'], r32['db'], scale=dyd.abs().sum(0))


@pytest.mark.gpu
@pytest.mark.parametrize('affine', [True, False])
@pytest.mark.parametrize('R,D', [(2, 4), (33, 68)])
def test_plain_batchnorm_eval(R, D, affine):
    from vit_ae_plus_plus_amd._abi import lib
    x, w, b, rm, rv, _ = _bn_inputs(R, D, affine, False, R + D)
    gx, grm, grv = inp(x.numpy()), inp(rm.numpy()), inp(rv.numpy())
    gw, gb = (inp(w.numpy()), inp(b.numpy())) if affine else (None, None)
    y = outp(R * D)
    P = lambda t: None if t is None else t.ptr
    lib.vitae_bn1d_eval(gx.ptr, P(gw), P(gb), grm.ptr, grv.ptr, y.ptr, R, D, BN_EPS, stream())
    torch.cuda.synchronize()
    assert y.guards_intact() and np.array_equal(grm.get(), rm.numpy()) and np.array_equal(grv.get(), rv.numpy())
    ref = lambda dt: F.batch_norm(x.to(dt), rm.to(dt), rv.to(dt), None if w is None else w.to(dt), None if b is None else b.to(dt), False, 0.0, BN_EPS)
    r64, r32 = ref(F64), ref(F32)
    wa = (w if affine else torch.ones(D)).double()
    ba = (b if affine else torch.zeros(D)).double()
    scale = ((x.double() - rm.double()) * (rv.double() + BN_EPS).rsqrt() * wa).abs() + ba.abs() + (rm.double() * (rv.double() + BN_EPS).rsqrt() * wa).abs()
    got = torch.from_numpy(y.get()).reshape(R, D)
    _rows_and_columns(f'eval R{R} D{D} affine{int(affine)}', ((got.double() - r64).abs() / scale).numpy(), ((r32.double() - r64).abs() / scale).numpy())


@pytest.mark.gpu
def test_plain_batchnorm_refusals_write_nothing():
    fwd, bwd, ev = raw('vitae_bn1d_fwd'), raw('vitae_bn1d_bwd'), raw('vitae_bn1d_eval')
    x, w = inp(np.ones(64)), inp(np.ones(8))
    y, mean, rstd = outp(64), outp(8), outp(8)
    s = stream()
    assert fwd(x.ptr, None, None, y.ptr, None, mean.ptr, rstd.ptr, None, None, None, 8, 6, BN_EPS, BN_MOM, s) == -2      # D % 4
    assert fwd(x.ptr + 4, None, None, y.ptr, None, mean.ptr, rstd.ptr, None, None, None, 8, 8, BN_EPS, BN_MOM, s) == -2  # alignment
    assert fwd(x.ptr, w.ptr, None, y.ptr, None, mean.ptr, rstd.ptr, None, None, None, 8, 8, BN_EPS, BN_MOM, s) == -1    # weight without bias
    assert fwd(None, None, None, y.ptr, None, mean.ptr, rstd.ptr, None, None, None, 8, 8, BN_EPS, BN_MOM, s) == -1
    assert bwd(x.ptr, x.ptr, None, mean.ptr, rstd.ptr, y.ptr, None, mean.ptr, rstd.ptr, 8, 8, s) == -1                  # dw without w
    assert bwd(x.ptr, x.ptr, None, mean.ptr, rstd.ptr, y.ptr, None, None, None, 8, 6, s) == -2
    assert ev(x.ptr, None, None, None, w.ptr, y.ptr, 8, 8, BN_EPS, s) == -1
    torch.cuda.synchronize()
    for t in (y, mean, rstd):
        assert np.isnan(t.get()).all() and t.guards_intact()


# =========================================================================== LayerNorm backward without atomics, any D
@pytest.mark.gpu
@pytest.mark.parametrize('acc', [0, 1])
@pytest.mark.parametrize('M,D', [(1, 4), (9, 64), (144, 64), (33, 68), (16, 760)])
def test_layernorm_record_backward(M, D, acc):
    """vitae_layernorm_bwd_part_any + vitae_ln_grad_reduce (what MoCo's base encoder trains with) against vitae_layernorm_bwd: the
    same kernel body, so dx is bit-equal; d gamma, d beta and colsum(dx) are the same partials added in a fixed order instead of by
    atomics: equal to 4 fp32 ulps of the sum of their absolute terms, and bit-equal between two calls."""
    from vit_ae_plus_plus_amd._abi import lib
    g = torch.Generator().manual_seed(M * 1000 + D + acc)
    x, dy, dx0 = torch.randn(M, D, generator=g), torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)
    w = 1.0 + 0.3 * torch.randn(D, generator=g)
    mean, rstd = x.mean(1), (x.var(1, unbiased=False) + 1e-6).rsqrt()
    G = -(-M // _consts()['VITAE_LN_PART_ANY_ROWS'])

    def records():
        ins = [inp(t.numpy()) for t in (dy, x, w, mean, rstd)]
        dx, part = Guarded(dx0.numpy()), outp(G * 3 * D)
        outs = [Guarded(np.zeros(D)) for _ in range(3)]
        lib.vitae_layernorm_bwd_part_any(*(t.ptr for t in ins), dx.ptr, part.ptr, None, M, D, acc, stream())
        one = lambda v, t=ctypes.c_void_p: (t * 1)(v)
        lib.vitae_ln_grad_reduce(1, one(part.ptr), one(outs[0].ptr), one(outs[1].ptr), one(outs[2].ptr), one(G, ctypes.c_int),
                                 one(D, ctypes.c_int), stream())
        torch.cuda.synchronize()
        assert all(t.guards_intact() for t in ins + [dx, part] + outs) and not np.isnan(part.get()).any()
        return [dx.get()] + [o.get() for o in outs]

    def atomics():
        ins = [inp(t.numpy()) for t in (dy, x, w, mean, rstd)]
        dx = Guarded(dx0.numpy())
        outs = [Guarded(np.zeros(D)) for _ in range(3)]
        lib.vitae_layernorm_bwd(*(t.ptr for t in ins), dx.ptr, outs[0].ptr, outs[1].ptr, None, outs[2].ptr, M, D, acc, stream())
        torch.cuda.synchronize()
        return [dx.get()] + [o.get() for o in outs]

    a, b, ref = records(), records(), atomics()
    assert all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a, b)), 'repeats differ'
    assert np.array_equal(a[0].view(np.uint32), ref[0].view(np.uint32))
    xhat = ((x - mean[:, None]) * rstd[:, None]).double()
    scales = [(dy.double() * xhat).abs().sum(0), dy.double().abs().sum(0), torch.from_numpy(a[0]).reshape(M, D).double().abs().sum(0)]
    for name, got, want, sc in zip(('d gamma', 'd beta', 'colsum dx'), a[1:], ref[1:], scales):
        assert (np.abs(got.astype(np.float64) - want) <= 4 * 2.0 ** -23 * sc.numpy()).all(), name
    # ... and against float64 on the statement
    assert np.abs(a[2] - dy.double().sum(0).numpy()).max() <= 1e-6 * float(scales[1].max())
    assert np.abs(a[1] - (dy.double() * xhat).sum(0).numpy()).max() <= 1e-5 * float(scales[0].max())


@pytest.mark.gpu
def test_layernorm_record_backward_refusals():
    fn = raw('vitae_layernorm_bwd_part_any')
    x = inp(np.ones(4096))
    dx, part = outp(4096), outp(4096)
    a = (x.ptr, x.ptr, x.ptr, x.ptr, x.ptr)
    assert fn(*a, dx.ptr, part.ptr, None, 2, 6, 0, stream()) == -2
    assert fn(*a, dx.ptr, part.ptr, None, 1, 772, 0, stream()) == -2
    assert fn(*a, dx.ptr, part.ptr + 4, None, 2, 8, 0, stream()) == -2
    assert fn(*a, dx.ptr, None, None, 2, 8, 0, stream()) == -1 and fn(*a, dx.ptr, part.ptr, None, 0, 8, 0, stream()) == -1
    torch.cuda.synchronize()
    assert np.isnan(dx.get()).all() and np.isnan(part.get()).all() and dx.guards_intact() and part.guards_intact()


@pytest.mark.gpu
@pytest.mark.parametrize('M,N,ld', [(1, 1, 1), (32, 64, 64), (33, 64, 70), (144, 257, 257), (100, 4, 4)])
def test_colsum_ordered(M, N, ld):
    """out[n] += sum_m dy[m, n] without atomics: against float64 at 4 fp32 ulps of sum |dy|, bit-equal repeats, `out` added to."""
    from vit_ae_plus_plus_amd._abi import lib
    rng = np.random.default_rng(M * 100 + N)
    dy = rng.standard_normal((M, ld)).astype(np.float32)
    start = rng.standard_normal(N).astype(np.float32)
    want = start.astype(np.float64) + dy[:, :N].astype(np.float64).sum(0)
    scale = np.abs(start) + np.abs(dy[:, :N]).astype(np.float64).sum(0)

    def once():
        g, out = inp(dy), Guarded(start)
        ws = outp(int(lib.vitae_colsum_ordered_ws_floats(M, N)))
        lib.vitae_colsum_ordered(g.ptr, ld, out.ptr, ws.ptr, M, N, stream())
        torch.cuda.synchronize()
        assert g.guards_intact() and out.guards_intact() and ws.guards_intact()
        return out.get()
    a, b = once(), once()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert (np.abs(a - want) <= 4 * 2.0 ** -23 * scale).all()
    fn = raw('vitae_colsum_ordered')
    out = Guarded(start)
    assert fn(None, ld, out.ptr, out.ptr, M, N, stream()) == -1 and fn(out.ptr, N - 1, out.ptr, out.ptr, M, N, stream()) == -1
    assert fn(out.ptr, ld, out.ptr, None, M, N, stream()) == -1
    torch.cuda.synchronize()
    assert np.array_equal(out.get(), start)
