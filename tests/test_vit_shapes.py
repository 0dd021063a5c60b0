"""``VisionTransformer3D`` through ``encoder.py`` against the float64 oracle, at the model shapes where the host sequencing changes
its mind: head size (scalar / fp32-MFMA / bf16-MFMA attention, act16 refused), ``vitae_sdpa_bwd_fused_fits`` (one-launch or streaming
attention backward), ``M = B (L + 1)`` against 64 (pad rows, ``Mpad`` weight gradients, caches keyed by ``B`` or by ``(M, N, K)``),
``act16_refusal`` switching inference between ``_block16`` and ``_block32``, ``H = D`` (fc2 and proj share every cache key), no
blocks, no qkv bias, anisotropic volumes, and five frozen-parameter patterns.  The kernels are held per element elsewhere; what
these tests look for is a bug of sequencing: a stale pad row, a buffer shared once too often, a cached split used for another
shape, a column sum taken from the wrong launch, a tail row of the last sample.

Reference: ``oracle.vit_ref`` in float64 under autograd, computed at test time on the CPU (one thread), once per (case, batch,
pooling) and shared; nothing modifies it.  Yardsticks: the same oracle in fp32 and under ``torch.autocast('cpu', bfloat16)``, in
the same metric on the same tensor.

Metrics
  gradients   relative L2 per parameter; where the float64 gradient is exactly zero the route's must be exactly zero
  features, logits, ``pos_embed`` gradient (per token row)
              per row: max_r |got_r - ref_r| / max_r |ref_r| (one bad row is not averaged away by the good ones)
Bounds (none taken from the code under test)
  fp32, fp32x3   <= 1e-4, the project's standing model-level bound (tests/test_vit_finetune.py); the ratio to the oracle's own fp32
                 gap is printed (``RATIO`` lines, run with -s), not asserted
  bf16           <= max(2 x the oracle's autocast gap, 1e-4); the factor 2 is the project's rule for every bf16 route, the floor is
                 for tensors with no contraction in them (``depth0`` under cls pooling: the autocast gap of the features is 6e-8)
  bf16 + act16   <= max(2 x max(autocast gap, error of the default bf16 route on the same case), 1e-4), the rule of
                 tests/test_vit_finetune_act16.py::test_route_gradients_and_logits; the default route is held to the oracle alone
                 in the same test
  exact checks   bit-equal where a result is reached by no float atomic, <= 1e-6 relative L2 where it is (the suite's bound for two
                 runs that differ only by the order of float atomics).  Forwards have none.  Backward: every bias and LayerNorm
                 gradient is a column sum finished by ``atomicAdd`` (csrc/norm.hip, gemm_glds.hip, attention_mfma.hip) on both
                 activation routes, and the fp32 route's GEMMs may split over atomics; on the act16 route the Linear and
                 patch-embedding weight gradients and ``pos_embed`` are ordered sums and must reproduce bit for bit."""
import functools

import numpy as np
import pytest
import torch

from oracle import vit_ref as V

POOL = {False: 'cls', True: 'gp'}
_BASE = dict(volume_size=(8, 8, 8), patch_size=4, in_chans=1, embed_dim=64, num_heads=2, mlp_ratio=4.0, depth=2)


def _case(B, act16, hd, qkv_bias=True, **kw):
    return {'cfg': dict(_BASE, **kw), 'B': B, 'act16': act16, 'hd': hd, 'qkv_bias': qkv_bias}


# name -> model, batch sizes, whether the bf16-activation route serves it, the head size the row is named for
CASES = {
    'n2': _case((1, 3), True, 32, volume_size=(4, 4, 4)),
    'hd16-m130': _case((2,), False, 16, volume_size=(16, 16, 16), in_chans=2, embed_dim=48, num_heads=3),
    'hd32-m65': _case((5,), False, 32, volume_size=(12, 8, 8), in_chans=2, embed_dim=96, num_heads=3),
    'hd128-m63': _case((7,), False, 128, embed_dim=128, num_heads=1),
    'n257-hd64': _case((2,), True, 64, volume_size=(32, 32, 16), num_heads=1, depth=1),
    'n449-hd32': _case((1,), True, 32, volume_size=(28, 32, 32), depth=1),
    'ratio1': _case((8,), True, 32, mlp_ratio=1.0),
    'h96': _case((3,), False, 64, num_heads=1, mlp_ratio=1.5),
    'aniso': _case((3,), True, 32, volume_size=(8, 12, 16), in_chans=3),
    'p8': _case((2,), True, 64, volume_size=(16, 16, 16), patch_size=8, num_heads=1),
    'depth0': _case((3,), True, 32, depth=0),
    'd256': _case((4,), True, 64, embed_dim=256, num_heads=4, depth=1),
    'nobias': _case((5,), False, 32, qkv_bias=False, volume_size=(12, 8, 8), in_chans=2, embed_dim=96, num_heads=3),
    # H = D at a width where the generic launcher splits K (M = 9, K = 512: two splits): proj, fc1 + GELU and fc2 differ by the epilogue alone
    'ratio1-d512': _case((1,), True, 64, embed_dim=512, num_heads=8, mlp_ratio=1.0, depth=1),
}
LONG = ('n257-hd64', 'n449-hd32')                 # above vitae_sdpa_bwd_fused_fits
TOKENS = {'n2': 2, 'hd16-m130': 65, 'hd32-m65': 13, 'hd128-m63': 9, 'n257-hd64': 257, 'n449-hd32': 449, 'ratio1': 9, 'h96': 9,
          'aniso': 25, 'p8': 9, 'depth0': 9, 'd256': 9, 'nobias': 13, 'ratio1-d512': 9}
ROWS = [(name, B) for name, c in CASES.items() for B in c['B']]
ROW_IDS = [f'{n}-b{B}' for n, B in ROWS]
PRECISIONS = ('fp32', 'fp32x3', 'bf16')
ROUTES = ('fp32', 'fp32x3', 'bf16', 'act16')      # training: (precision, activations)
ROUTE_ARGS = {'fp32': ('fp32', None), 'fp32x3': ('fp32x3', None), 'bf16': ('bf16', None), 'act16': ('bf16', 'bf16')}
ROUTE_NAME = {'fp32': 'fp32-activations', 'fp32x3': 'fp32-activations', 'bf16': 'fp32-activations', 'act16': 'bf16-activations'}
FP32_BOUND, BF16_FACTOR, BF16_FLOOR, ATOMIC_BOUND = 1e-4, 2.0, 1e-4, 1e-6
# depth0: what does not reach the loss (float64 gradient exactly zero)
DEPTH0_ZERO = {False: ['patch_embed.proj.bias', 'patch_embed.proj.weight'], True: ['cls_token']}


def _cfg(name, gp):
    return V.VitConfig(num_classes=3, global_pool=gp, **CASES[name]['cfg'])


def _data(name, B):
    cfg = _cfg(name, False)
    x = torch.randn(B, cfg.in_chans, *cfg.volume_size, generator=torch.Generator().manual_seed(11))
    return x, torch.arange(B) % 3


def _weights(name, gp):
    """The oracle's state dict (qkv_bias=False: a zero qkv bias) and the names the module has."""
    cfg = _cfg(name, gp)
    sd = V.init_vit_state_dict(cfg, seed=5)
    names = list(sd.keys())
    if not CASES[name]['qkv_bias']:
        for k in names:
            if k.endswith('attn.qkv.bias'):
                sd[k] = torch.zeros_like(sd[k])
        names = [k for k in names if not k.endswith('attn.qkv.bias')]
    return sd, names


# ----------------------------------------------------------------------------------------------- metrics
def _rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    n = float(np.linalg.norm(ref))
    if n == 0.0:                    # an exact zero of the reference has no scale: only an exact zero matches it
        return 0.0 if not got.any() else float('inf')
    return float(np.linalg.norm(got - ref) / n)


def _rows(got, ref):
    """Per row (the last axis is the row), relative to the largest reference row."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    got, ref = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    n = float(np.linalg.norm(ref, axis=1).max())
    if n == 0.0:
        return 0.0 if not got.any() else float('inf')
    return float(np.linalg.norm(got - ref, axis=1).max() / n)


def _metrics(run, ref, names):
    out = {'feat': _rows(run['feat'], ref['feat']), 'logits': _rows(run['logits'], ref['logits'])}
    for n in names:
        out['grad/' + n] = _rel(run['grad'][n], ref['grad'][n])
    if 'pos_embed' in names:
        out['pos_embed/rows'] = _rows(run['grad']['pos_embed'], ref['grad']['pos_embed'])
    return out


# ----------------------------------------------------------------------------------------------- oracle
def _oracle_run(cfg, sd0, x, y, dtype, autocast):
    sd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd0.items()}

    def fwd():
        f = V.forward_features(sd, x.to(dtype), cfg)
        logits = torch.nn.functional.linear(f, sd['head.weight'], sd['head.bias'])
        return f, logits, torch.nn.functional.cross_entropy(logits, y)

    if autocast:
        with torch.autocast('cpu', dtype=torch.bfloat16):
            f, logits, loss = fwd()
    else:
        f, logits, loss = fwd()
    loss.backward()
    return {'feat': f.detach().double().numpy(), 'logits': logits.detach().double().numpy(),
            'grad': {k: v.grad.detach().double().numpy() for k, v in sd.items()}}


@functools.lru_cache(maxsize=None)
def _oracle(name, B, gp):
    """float64 reference and the two yardsticks of one (case, batch, pooling); computed once and shared, nothing modifies it."""
    cfg = _cfg(name, gp)
    sd, names = _weights(name, gp)
    x, y = _data(name, B)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)        # one summation order
    try:
        r64 = _oracle_run(cfg, sd, x, y, torch.float64, False)
        r32 = _oracle_run(cfg, sd, x, y, torch.float32, False)
        r16 = _oracle_run(cfg, sd, x, y, torch.float32, True)
    finally:
        torch.set_num_threads(threads)
    return {'names': names, 'f64': r64, 'f32': r32, 'f16': r16, 'y32': _metrics(r32, r64, names), 'y16': _metrics(r16, r64, names)}


def _bound(route, key, orc, e_default=None):
    if route in ('fp32', 'fp32x3'):
        return FP32_BOUND
    gap = orc['y16'][key]
    if route == 'act16':
        gap = max(gap, e_default[key])
    return max(BF16_FACTOR * gap, BF16_FLOOR)


# ----------------------------------------------------------------------------------------------- CPU
def test_cases_reach_their_paths():
    """Host predicates only: the table above claims paths; a threshold that moves must not leave it claiming them in vain."""
    from vit_ae_plus_plus_amd._abi import lib
    from vit_ae_plus_plus_amd._launch import pad64
    from vit_ae_plus_plus_amd.encoder import act16_refusal
    assert sorted(TOKENS) == sorted(CASES)
    for name, c in CASES.items():
        cfg = _cfg(name, False)
        N, D = cfg.num_patches + 1, cfg.embed_dim
        hd, H, P = D // cfg.num_heads, int(D * cfg.mlp_ratio), cfg.in_chans * cfg.patch_size ** 3
        assert N == TOKENS[name] and hd == c['hd'] and hd * cfg.num_heads == D, name
        hidden = H if cfg.depth else D                      # what encoder.py passes for a model without blocks
        assert (act16_refusal('bf16', D, hidden, P, hd) is None) == c['act16'], name
        for precision in ('fp32', 'fp32x3'):
            assert act16_refusal(precision, D, hidden, P, hd) is not None, name
        # the query is about the MFMA attention backward: it answers 0 for a head size that kernel does not have (16, 128)
        assert lib.vitae_sdpa_bwd_fused_fits(N, hd) == (0 if name in LONG or hd not in (32, 64) else 1), name
        for B in c['B']:
            assert pad64(B * N) != B * N, (name, B)         # every row has pad rows
    # what each row is there for
    assert all(CASES[n]['act16'] for n in LONG)             # the streaming backward is the act16 route's
    assert lib.vitae_sdpa_bwd_fused_fits(256, 64) == 1 and lib.vitae_sdpa_bwd_fused_fits(448, 32) == 1      # ... and sits ON the edge
    assert 2 * TOKENS['n257-hd64'] == 514 and pad64(514) == 576
    assert 5 * TOKENS['hd32-m65'] == 65 and 7 * TOKENS['hd128-m63'] == 63 and 8 * TOKENS['ratio1'] == 72
    assert _cfg('hd32-m65', False).embed_dim % 64 and CASES['hd32-m65']['hd'] == 32     # refused for D alone
    c = _cfg('h96', False)
    assert int(c.embed_dim * c.mlp_ratio) == 96 and act16_refusal('bf16', 64, 64, 64, 64) is None           # refused for H alone
    c = _cfg('ratio1', False)
    assert int(c.embed_dim * c.mlp_ratio) == c.embed_dim
    assert lib.vitae_gemm_pick_split_k(9, 512, 512) > 1 and lib.vitae_gemm_bf16x3_pick_split_k(9, 512, 512) > 1      # ratio1-d512
    assert len(set(_cfg('aniso', False).grid)) == 3 and _cfg('aniso', False).in_chans * 64 == 192
    assert _cfg('p8', False).patch_size ** 3 == 512 and _cfg('depth0', False).depth == 0 and _cfg('d256', False).embed_dim == 256


# The oracle's own loss of precision against float64 over the whole table (relative L2 per tensor), as measured when the table was
# made; a factor of 3 of slack either way.  A yardstick outside its range is a broken oracle call, not a loose bound.
Y_GRAD32, Y_FEAT32, Y_GRAD16, Y_FEAT16, SLACK = (3e-7, 3.4e-6), (6e-8, 6e-7), (6e-4, 4.4e-2), (2.3e-3, 6.9e-3), 3.0


@pytest.mark.parametrize('name,B', ROWS, ids=ROW_IDS)
@pytest.mark.parametrize('gp', [False, True], ids=['cls', 'gp'])
def test_oracle_yardsticks(name, B, gp):
    orc = _oracle(name, B, gp)
    r64, r32, r16 = orc['f64'], orc['f32'], orc['f16']
    inside = lambda v, rng: rng[0] / SLACK <= v <= rng[1] * SLACK
    zero = DEPTH0_ZERO[gp] if name == 'depth0' else []
    assert sorted(n for n in r64['grad'] if not r64['grad'][n].any()) == zero
    f32, f16 = _rel(r32['feat'], r64['feat']), _rel(r16['feat'], r64['feat'])
    print(f'YARD {name}-b{B}-{POOL[gp]} features fp32 {f32:.2e} autocast {f16:.2e}')
    assert inside(f32, Y_FEAT32), f32
    if name == 'depth0' and not gp:         # cls row = LayerNorm(cls_token + pos_embed[0]): no contraction, nothing autocast rounds
        assert f16 <= Y_FEAT32[1] * SLACK, f16
    else:
        assert inside(f16, Y_FEAT16), f16
    worst32 = 0.0
    for n in orc['names']:
        if n in zero:
            assert not r32['grad'][n].any() and not r16['grad'][n].any(), n
            continue
        g32, g16 = _rel(r32['grad'][n], r64['grad'][n]), _rel(r16['grad'][n], r64['grad'][n])
        print(f'YARD {name}-b{B}-{POOL[gp]} {n} fp32 {g32:.2e} autocast {g16:.2e}')
        assert 0 < g32 <= Y_GRAD32[1] * SLACK, (n, g32)
        assert inside(g16, Y_GRAD16), (n, g16)
        worst32 = max(worst32, g32)
    assert inside(worst32, Y_GRAD32), worst32         # the fp32 range is that of a row's worst parameter
    # the metrics the GPU tests use are finite and positive wherever the reference is not an exact zero
    for k, v in orc['y16'].items():
        assert np.isfinite(v) and (v > 0 or k[5:] in zero or (k == 'feat' and name == 'depth0' and not gp)), (k, v)


# ----------------------------------------------------------------------------------------------- GPU plumbing
def _model(name, gp, route, train):
    from vit_ae_plus_plus_amd.model.vit import VisionTransformer3D
    cfg = _cfg(name, gp)
    precision, activations = ROUTE_ARGS[route]
    m = VisionTransformer3D(volume_size=tuple(cfg.volume_size), patch_size=cfg.patch_size, in_chans=cfg.in_chans,
                            num_classes=cfg.num_classes, embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads,
                            mlp_ratio=cfg.mlp_ratio, qkv_bias=CASES[name]['qkv_bias'], global_pool=cfg.global_pool,
                            precision=precision, activations=activations).cuda()
    sd, names = _weights(name, gp)
    assert [n for n, _ in m.named_parameters()] == names            # qkv_bias=False: no such parameter
    m.load_state_dict({k: sd[k] for k in names})
    return m.train() if train else m.eval()


def _infer(m, x):
    with torch.no_grad():
        f = m.forward_features(x)
    torch.cuda.synchronize()
    assert not f.requires_grad
    return f.cpu()


def _step(m, x, y):
    """One forward + backward in train(): features, logits, {name: gradient or None}."""
    m.zero_grad(set_to_none=True)
    feats, inner = [], type(m).forward_features.__get__(m)
    m.forward_features = lambda v: (feats.append(inner(v)), feats[-1])[1]       # forward() calls it once: keep what it returned
    try:
        logits = m(x)
    finally:
        del m.forward_features
    torch.nn.functional.cross_entropy(logits, y).backward()
    torch.cuda.synchronize()
    assert len(feats) == 1
    return {'feat': feats[0].detach().cpu().numpy(), 'logits': logits.detach().cpu().numpy(),
            'grad': {n: (None if p.grad is None else p.grad.detach().cpu().numpy()) for n, p in m.named_parameters()}}


def _held(label, route, run, orc, names, e_default=None):
    """Holds one training run to the float64 oracle; -> its errors by key."""
    errs = _metrics(run, orc['f64'], names)
    worst = (0.0, None)
    for k, e in errs.items():
        b = _bound(route, k, orc, e_default)
        worst = max(worst, (e / b, k))
        y32 = orc['y32'][k]
        print(f'RATIO {label} {route} {k}: err {e:.3e} bound {b:.3e} err/bound {e / b:.3f} oracle fp32 {y32:.3e} autocast {orc["y16"][k]:.3e}'
              + (f' err/fp32gap {e / y32:.2f}' if route in ('fp32', 'fp32x3') and y32 > 0 else ''))
    assert worst[0] <= 1.0, (label, route, worst)
    return errs


def _same(a, b, exact):
    """Two results of the same launches: bit-equal, or (``exact`` False) within the bound for another order of float atomics."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.isfinite(a).all()
    if exact:
        return a.tobytes() == b.tobytes()
    return _rel(a, b) <= ATOMIC_BOUND


def _ordered(route, n):
    """Gradients reached by no float atomic (see the module docstring)."""
    return route == 'act16' and (n == 'pos_embed' or (n.endswith('.weight') and 'norm' not in n and not n.startswith('head.')))


def _same_step(route, got, ref, label):
    assert _same(got['feat'], ref['feat'], True) and _same(got['logits'], ref['logits'], True), label        # forwards: no atomics
    assert got['grad'].keys() == ref['grad'].keys()
    for n, g in ref['grad'].items():
        assert (g is None) == (got['grad'][n] is None), (label, n)
        if g is not None:
            assert _same(got['grad'][n], g, _ordered(route, n)), (label, n, _rel(got['grad'][n], g))


# ----------------------------------------------------------------------------------------------- GPU: parity
@pytest.mark.gpu
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('gp', [False, True], ids=['cls', 'gp'])
@pytest.mark.parametrize('name,B', ROWS, ids=ROW_IDS)
def test_inference_parity(name, B, gp, precision):
    orc = _oracle(name, B, gp)
    m = _model(name, gp, precision, train=False)
    f = _infer(m, _data(name, B)[0].cuda()).numpy()
    assert f.shape == orc['f64']['feat'].shape and np.isfinite(f).all()
    assert m._encoder.act16 == (precision == 'bf16' and CASES[name]['act16'])
    e, b = _rows(f, orc['f64']['feat']), _bound(precision, 'feat', orc)
    print(f'RATIO {name}-b{B}-{POOL[gp]} infer-{precision} feat: err {e:.3e} bound {b:.3e} err/bound {e / b:.3f} '
          f'oracle fp32 {orc["y32"]["feat"]:.3e} autocast {orc["y16"]["feat"]:.3e}')
    assert e <= b, (e, b)


@pytest.mark.gpu
@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('gp', [False, True], ids=['cls', 'gp'])
@pytest.mark.parametrize('name,B', ROWS, ids=ROW_IDS)
def test_training_parity(name, B, gp, route):
    from vit_ae_plus_plus_amd._abi import VitaeError
    orc = _oracle(name, B, gp)
    names, label = orc['names'], f'{name}-b{B}-{POOL[gp]}'
    x, y = (t.cuda() for t in _data(name, B))
    if route == 'act16' and not CASES[name]['act16']:
        with pytest.raises(VitaeError):
            _model(name, gp, 'act16', train=True)
        m = _model(name, gp, 'bf16', train=True)
        with pytest.raises(VitaeError):
            m.set_precision('bf16', activations='bf16')
        assert m._precision == 'bf16' and m._activations is None        # a refused call changes nothing
        _held(label, 'bf16', _step(m, x, y), orc, names)
        assert m._trainer.stats['route'] == 'fp32-activations'
        return
    e_default = None
    if route == 'act16':            # its comparator, held to the oracle alone first
        e_default = _held(label, 'bf16', _step(_model(name, gp, 'bf16', train=True), x, y), orc, names)
    m = _model(name, gp, route, train=True)
    run = _step(m, x, y)
    assert m._trainer.stats['route'] == ROUTE_NAME[route] and m._trainer.stats['forwards'] == 1 and m._trainer.stats['backwards'] == 1
    assert sorted(n for n, g in run['grad'].items() if g is not None) == sorted(names)      # complete, and no gradient without a parameter
    assert not any(n.endswith('attn.qkv.bias') for n in run['grad']) or CASES[name]['qkv_bias']
    for n in names:
        assert np.isfinite(run['grad'][n]).all(), n
        if not orc['f64']['grad'][n].any():
            assert not run['grad'][n].any(), n          # what does not reach the loss gets an exact zero
    if name == 'depth0':
        assert [n for n in sorted(names) if not run['grad'][n].any()] == DEPTH0_ZERO[gp]
    _held(label, route, run, orc, names, e_default)


# ----------------------------------------------------------------------------------------------- GPU: partly trainable
_EMBED = ('cls_token', 'pos_embed', 'patch_embed.proj.weight', 'patch_embed.proj.bias')
SUBSETS = {
    'pos_embed': ('pos_embed',),
    'patch_bias': ('patch_embed.proj.bias',),
    'embeddings': _EMBED,
    'fc2_bias_0': ('blocks.0.mlp.fc2.bias',),
    'block1_biases': ('blocks.1.attn.qkv.bias', 'blocks.1.mlp.fc1.bias'),
}
PARTIAL = [('hd32-m65', 5, r) for r in ('fp32', 'fp32x3', 'bf16')] + [('n2', 3, 'act16')]


@pytest.mark.gpu
@pytest.mark.parametrize('subset', list(SUBSETS))
@pytest.mark.parametrize('gp', [False, True], ids=['cls', 'gp'])
@pytest.mark.parametrize('name,B,route', PARTIAL, ids=[f'{n}-b{B}-{r}' for n, B, r in PARTIAL])
def test_partly_trainable(name, B, route, gp, subset):
    """The float64 gradient of a parameter does not depend on which others are trainable: the reference is the full oracle run
    restricted to the subset, the bounds are those of test_training_parity."""
    orc = _oracle(name, B, gp)
    keep = SUBSETS[subset]
    x, y = (t.cuda() for t in _data(name, B))

    def run(r):
        m = _model(name, gp, r, train=True)
        for n, p in m.named_parameters():
            p.requires_grad = n in keep
        assert sum(p.requires_grad for p in m.parameters()) == len(keep)
        out = _step(m, x, y)
        assert m._trainer.stats['route'] == ROUTE_NAME[r]
        assert sorted(n for n, g in out['grad'].items() if g is not None) == sorted(keep)
        return out

    label = f'{name}-b{B}-{POOL[gp]}-only-{subset}'
    e_default = _held(label, 'bf16', run('bf16'), orc, keep) if route == 'act16' else None
    _held(label, route, run(route), orc, keep, e_default)


# ----------------------------------------------------------------------------------------------- GPU: exact checks
def _features(m, x, train):
    """The forward of a route: inference, or the forward of a training step (gradients enabled, activations kept)."""
    if not train:
        return _infer(m, x)
    f = m.forward_features(x)
    torch.cuda.synchronize()
    assert f.requires_grad
    return f.detach().cpu()


FORWARDS = [('infer', p) for p in PRECISIONS] + [('train', r) for r in ROUTES]
NAN_ROWS = [('hd32-m65', 5), ('n257-hd64', 2), ('hd128-m63', 7), ('n2', 3)]
NAN_GRID = [(n, B, mode, r) for n, B in NAN_ROWS for mode, r in FORWARDS if r != 'act16' or CASES[n]['act16']]


@pytest.mark.gpu
@pytest.mark.parametrize('gp', [False, True], ids=['cls', 'gp'])
@pytest.mark.parametrize('name,B,mode,route', NAN_GRID, ids=[f'{n}-b{B}-{mode}-{r}' for n, B, mode, r in NAN_GRID])
def test_one_nan_sample_stays_alone(name, B, mode, route, gp):
    """Sample j of the input is NaN: its feature row is all NaN, every other row has the bits of the clean run — an attention tail, a
    pooled row or a pad row that reads a neighbour (even times zero) would not.  The clean run after them finds nothing left over."""
    m = _model(name, gp, route, train=mode == 'train')
    x = _data(name, B)[0].cuda()
    clean = _features(m, x, mode == 'train')
    assert bool(torch.isfinite(clean).all())
    for j in (0, B - 1):
        xn = x.clone()
        xn[j] = float('nan')
        f = _features(m, xn, mode == 'train')
        assert bool(torch.isnan(f[j]).all()), j
        others = [b for b in range(B) if b != j]
        assert bool(torch.isfinite(f[others]).all()), j
        assert torch.equal(f[others], clean[others]), j
    assert torch.equal(_features(m, x, mode == 'train'), clean)


SEQ = [('aniso', mode, r) for mode, r in FORWARDS] + [('hd32-m65', mode, r) for mode, r in FORWARDS if r != 'act16']


@pytest.mark.gpu
@pytest.mark.parametrize('gp', [False, True], ids=['cls', 'gp'])
@pytest.mark.parametrize('name,mode,route', SEQ, ids=[f'{n}-{mode}-{r}' for n, mode, r in SEQ])
def test_batch_size_sequence(name, mode, route, gp):
    """B = 5, 1, 5 on ONE model: buffers cached on the batch size, splits cached per shape and pad rows zeroed per call must leave the
    third result equal to the first, and the B = 1 result equal to a fresh model's."""
    x, y = (t.cuda() for t in _data(name, 5))
    if mode == 'infer':
        m = _model(name, gp, route, train=False)
        a, one, b = _infer(m, x), _infer(m, x[:1]), _infer(m, x)
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
        assert torch.equal(one, _infer(_model(name, gp, route, train=False), x[:1]))
        assert one.shape == (1, a.shape[1])
        return
    m = _model(name, gp, route, train=True)
    a, one, b = _step(m, x, y), _step(m, x[:1], y[:1]), _step(m, x, y)
    assert m._trainer.stats['forwards'] == 3
    _same_step(route, b, a, 'third against first')
    _same_step(route, one, _step(_model(name, gp, route, train=True), x[:1], y[:1]), 'B = 1 against a fresh model')


SWITCHES = ('fp32', 'bf16', 'act16', 'fp32x3', 'fp32')


@pytest.mark.gpu
@pytest.mark.parametrize('gp', [False, True], ids=['cls', 'gp'])
def test_route_switches_on_one_model(gp):
    """set_precision fp32 -> bf16 -> bf16 + act16 -> fp32x3 -> fp32 on one model: after each switch it computes what a model built
    in that setting computes (no encoder, trainer, split or bf16 weight copy of the setting before survives)."""
    name, B = 'aniso', 3
    x, y = (t.cuda() for t in _data(name, B))
    m = _model(name, gp, 'fp32', train=True)
    for i, route in enumerate(SWITCHES):
        m.set_precision(*ROUTE_ARGS[route])
        fresh = _model(name, gp, route, train=True)
        _same_step(route, _step(m, x, y), _step(fresh, x, y), f'switch {i} to {route}: training')
        assert m._trainer.stats['route'] == ROUTE_NAME[route]
        assert torch.equal(_infer(m.eval(), x), _infer(fresh.eval(), x)), (i, route)
        assert m._encoder.act16 == (route in ('bf16', 'act16'))
        m.train()


@pytest.mark.gpu
@pytest.mark.parametrize('gp', [False, True], ids=['cls', 'gp'])
@pytest.mark.parametrize('mode,route', FORWARDS, ids=[f'{mode}-{r}' for mode, r in FORWARDS])
def test_input_forms(mode, route, gp):
    """A float64, a bf16 and a non-contiguous input give the bits of their ``.contiguous().float()`` copy."""
    name, B = 'aniso', 3
    x, y = (t.cuda() for t in _data(name, B))
    strided = x.permute(0, 1, 4, 3, 2).contiguous().permute(0, 1, 4, 3, 2)      # the same values, the innermost axis strided
    assert not strided.is_contiguous() and torch.equal(strided, x)
    forms = {'float64': x.double(), 'bf16': x.bfloat16(), 'strided': strided}
    m = _model(name, gp, route, train=mode == 'train')
    for form, xi in forms.items():
        plain = xi.contiguous().float()
        if mode == 'infer':
            assert torch.equal(_infer(m, xi), _infer(m, plain)), form
        else:
            _same_step(route, _step(m, xi, y), _step(m, plain, y), form)


@pytest.mark.gpu
@pytest.mark.parametrize('gp', [False, True], ids=['cls', 'gp'])
def test_head_size_nobody_built(gp):
    """D 48 with 2 heads (head size 24): every precision refuses, in inference and in training, and returns nothing."""
    from vit_ae_plus_plus_amd._abi import VitaeError
    from vit_ae_plus_plus_amd.model.vit import VisionTransformer3D
    make = lambda **kw: VisionTransformer3D(volume_size=(8, 8, 8), patch_size=4, in_chans=1, num_classes=3, embed_dim=48, depth=2,
                                            num_heads=2, global_pool=gp, **kw).cuda()
    x = torch.randn(2, 1, 8, 8, 8, generator=torch.Generator().manual_seed(11)).cuda()
    with pytest.raises(VitaeError):
        make(precision='bf16', activations='bf16')
    for precision in PRECISIONS:
        m = make(precision=precision)
        out = None
        with pytest.raises(VitaeError):
            with torch.no_grad():
                out = m.eval().forward_features(x)
        with pytest.raises(VitaeError):
            out = m.train()(x)
        with pytest.raises(VitaeError):
            m.set_precision('bf16', activations='bf16')
        assert out is None and m._precision == precision and m._activations is None
        torch.cuda.synchronize()
