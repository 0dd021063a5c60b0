"""Fine-tuning VisionTransformer3D on bf16 activations: ``precision='bf16', activations='bf16'`` (``HipEncoderTrainer16``), and the
hand-over kernel ``vitae_token_select_bwd16``.

Expectations: tests/golden/vit_finetune_act16.npz, written by tools/gen_finetune_act16_golden.py from the reference's own
VisionTransformer3D on two micro configurations the route accepts (embed 64, one head of 64 or two of 32, 16^3 volumes of one
channel, patch 4: 65 tokens, batch 3 = 195 rows, padded to 256).  Gradients of one configuration and pooling mode are 0.43 MB
of incompressible fp32, so the file holds two of the four pairs (``h32/cls`` and ``h64/gp``: both head sizes, both pooling
modes).  The other two (``h32/gp``, ``h64/cls``) come from the oracle restatement (``oracle.vit_ref.forward`` under autograd, and
under ``torch.autocast('cpu', bfloat16)`` for the reference's own loss of precision), computed once per session on the CPU;
``test_oracle_reproduces_the_fixture`` shows on the two stored pairs that it gives what the reference gives — gradients and loss
to 1e-6 and the three autocast figures to 1e-3 relative — so all four pairs are tested against the same quantities.

Bounds of the route tests (the comparators are the reference and the route this project already had, never the new code):
  gradients   per parameter, relative L2 error against fp32 <= 2 x max(``bf16_ref_relerr``, the error of the existing bf16 route
              (``activations=None``) in the same run); the factor 2 is the project's margin for bf16 gradients
              (tests/test_vit_finetune.py)
  logits      max-abs error, the same rule against ``bf16_ref_logits_err``
  AdamW       |loss - fp32 loss| of each of the four steps, the same rule step by step against ``bf16_ref_adamw_dev``: step i of the
              new route <= 2 x max(step i of the reference under autocast, step i of the existing route).  All twelve figures of
              a pair are printed; LABNOTES.md keeps them.
  1e-6        where two runs issue the same launches and differ only by the order of float atomics (the suite's bound).
Every route test prints both routes' figures per parameter (run with -s); LABNOTES.md keeps which parameters needed the
existing-route term of the max.

Kernel test: ``dx`` bitwise against vitae_token_select_bwd, ``dx_bf16`` bitwise against ``dx.bfloat16()``, zero pad rows in a
buffer that started as a sentinel, column sums in the metric and bound of tests/test_norm_kernels.py (|s - s64| / sum of the
|addends|, worst column, <= max(3 e32, 4 x 2^-24) with e32 the same metric of numpy's fp32 sum; the floor because e32 is exactly
zero where a column has one non-zero addend), sentinels behind every output, two calls bitwise equal, refusals write nothing."""
import functools
import os
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

from oracle import mae_ref as R
from oracle import vit_ref as V
from oracle.gen_golden import MICRO, VITB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'vit_finetune_act16.npz')
ENC = dict(volume_size=(16, 16, 16), patch_size=4, in_chans=1, embed_dim=64, depth=2)
HEADS = {'h32': 2, 'h64': 1}
TAGS = {False: 'cls', True: 'gp'}
PAIRS = [('h32', False), ('h32', True), ('h64', False), ('h64', True)]
PAIR_IDS = [f'{n}-{TAGS[g]}' for n, g in PAIRS]
STORED = [('h32', False), ('h64', True)]


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD, allow_pickle=False)


def _cfg(name, gp):
    return V.VitConfig(num_classes=3, global_pool=gp, num_heads=HEADS[name], **ENC)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ----------------------------------------------------------------------------------------------- expectations
def _oracle_run(cfg, x, y, cw, bf16, steps=0):
    """The oracle on the CPU: (loss, logits, {name: gradient}) of one forward + backward, or the losses of ``steps`` AdamW steps."""
    sd = {k: v.clone().requires_grad_(True) for k, v in V.init_vit_state_dict(cfg, seed=5).items()}
    ce = torch.nn.CrossEntropyLoss(weight=cw)

    def once():
        if bf16:
            with torch.autocast('cpu', dtype=torch.bfloat16):
                logits = V.forward(sd, x, cfg)
                loss = ce(logits, y)
        else:
            logits = V.forward(sd, x, cfg)
            loss = ce(logits, y)
        loss.backward()
        return loss.detach().float(), logits.detach().float()

    if not steps:
        loss, logits = once()
        return float(loss), logits.numpy(), {k: v.grad.detach().float().numpy() for k, v in sd.items()}
    opt = torch.optim.AdamW(list(sd.values()), lr=1e-3, weight_decay=0.05)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        losses.append(float(once()[0]))
        opt.step()
    return np.array(losses, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def _oracle_expect(name, gp):
    """What the fixture stores for a pair, from the oracle (computed once and shared; nothing modifies it)."""
    g = np.load(GOLD, allow_pickle=False)
    x, y, cw = torch.from_numpy(g['x']), torch.from_numpy(g['labels']), torch.from_numpy(g['class_weights'])
    cfg = _cfg(name, gp)
    one = torch.get_num_threads()
    torch.set_num_threads(1)        # as the generator: one summation order
    try:
        loss, logits, g32 = _oracle_run(cfg, x, y, cw, False)
        _, logits16, g16 = _oracle_run(cfg, x, y, cw, True)
        a32, a16 = _oracle_run(cfg, x, y, cw, False, 4), _oracle_run(cfg, x, y, cw, True, 4)
    finally:
        torch.set_num_threads(one)
    return {'names': list(g32.keys()), 'loss': loss, 'logits': logits, 'grad': g32,
            'relerr': {n: _rel(g16[n], g32[n]) for n in g32}, 'logits_err': float(np.abs(logits16 - logits).max()),
            'adamw_losses': a32, 'adamw_dev': np.abs(a16 - a32)}


def _expect(gold, name, gp):
    """The expectation of a pair: the fixture where it holds the pair, else the oracle."""
    p = f'{name}/{TAGS[gp]}'
    if (name, gp) not in STORED:
        return _oracle_expect(name, gp)
    names = [str(n) for n in gold[f'{p}/names']]
    return {'names': names, 'loss': float(gold[f'{p}/loss']), 'logits': gold[f'{p}/logits'],
            'grad': {n: gold[f'{p}/grad/{n}'] for n in names}, 'relerr': {n: float(gold[f'{p}/bf16_ref_relerr/{n}']) for n in names},
            'logits_err': float(gold[f'{p}/bf16_ref_logits_err']), 'adamw_losses': gold[f'{p}/adamw_losses'],
            'adamw_dev': gold[f'{p}/bf16_ref_adamw_dev']}


# ----------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize('name,gp', STORED, ids=[f'{n}-{TAGS[g]}' for n, g in STORED])
def test_oracle_reproduces_the_fixture(gold, name, gp):
    assert [str(p) for p in gold['pairs']] == [f'{n}/{TAGS[g]}' for n, g in STORED]
    ref, got = _expect(gold, name, gp), _oracle_expect(name, gp)
    assert got['names'] == ref['names']
    assert abs(got['loss'] - ref['loss']) <= 1e-6 * abs(ref['loss'])
    assert np.allclose(got['logits'], ref['logits'], atol=2e-6)
    for n in ref['names']:
        assert np.linalg.norm(ref['grad'][n]) > 0 and ref['relerr'][n] > 0, n
        assert _rel(got['grad'][n], ref['grad'][n]) <= 1e-6, n
        # the oracle under autocast loses what the reference loses under autocast: the comparator of the two pairs not stored
        assert abs(got['relerr'][n] - ref['relerr'][n]) <= 1e-3 * ref['relerr'][n], (n, got['relerr'][n], ref['relerr'][n])
    assert np.allclose(got['adamw_losses'], ref['adamw_losses'], rtol=1e-6, atol=0)
    assert abs(got['logits_err'] - ref['logits_err']) <= 1e-3 * ref['logits_err']
    assert abs(got['adamw_dev'].max() - ref['adamw_dev'].max()) <= 1e-3 * ref['adamw_dev'].max()


def test_fixture_regenerates_identically(gold, tmp_path):
    from oracle import _refharness as H
    if not H.reference_available():
        pytest.skip('the reference checkout is not on this machine')
    out = str(tmp_path / 'regen.npz')
    subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_finetune_act16_golden.py'), '--out', out], check=True, cwd=ROOT,
                   stdout=subprocess.DEVNULL)
    new = np.load(out, allow_pickle=False)
    assert sorted(new.files) == sorted(gold.files)
    for k in gold.files:
        assert new[k].dtype == gold[k].dtype and new[k].tobytes() == gold[k].tobytes(), k
    # 1 MiB is the most a file committed to this project may hold (tools/README.md): why the fixture stores two pairs, not four
    assert os.path.getsize(GOLD) <= 1 << 20


def test_abi_knows_the_handover_kernel():
    from vit_ae_plus_plus_amd import _abi
    assert 'vitae_token_select_bwd16' in _abi.PROTOS
    assert _abi.PROTOS['vitae_token_select_bwd16'] == ('int', ['ptr'] * 4 + ['int'] * 5 + ['ptr'])
    assert 'vitae_token_select_bwd16' in open(os.path.join(ROOT, 'include', 'vitae_hip.h')).read()
    assert _abi.CONSTS['VITAE_ABI_VERSION'] >= 53


def _module(cfg, precision='bf16', activations=None, **kw):
    from vit_ae_plus_plus_amd.model.vit import VisionTransformer3D
    return VisionTransformer3D(volume_size=cfg.volume_size[0], patch_size=cfg.patch_size, in_chans=cfg.in_chans,
                               num_classes=cfg.num_classes, embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads,
                               global_pool=cfg.global_pool, precision=precision, activations=activations, **kw)


def test_activations_interface_refusals():
    from vit_ae_plus_plus_amd._abi import VitaeError
    ok = _cfg('h32', True)
    m = _module(ok, 'bf16', 'bf16')                                   # an eligible model is accepted, at the constructor and the setter
    assert m._activations == 'bf16'
    m.set_precision('bf16', activations='bf16')
    m.set_precision('bf16')
    assert m._activations == 'bf16'                                   # left out, the choice stays (a k-fold loop that re-sets the precision)
    with pytest.raises(VitaeError):                                   # ... and is not dropped silently by a precision it cannot have
        m.set_precision('fp32')
    assert m._precision == 'bf16' and m._activations == 'bf16'
    m.set_precision('fp32', activations=None)
    assert m._precision == 'fp32' and m._activations is None
    m.set_precision('bf16')
    assert m._activations is None
    assert _module(ok, 'bf16')._activations is None                   # the default is today's route
    for precision in ('fp32', 'fp32x3'):
        with pytest.raises(VitaeError):
            _module(ok, precision, 'bf16')
        with pytest.raises(VitaeError):
            m.set_precision(precision, activations='bf16')
    assert m._precision == 'bf16' and m._activations is None          # a refused call changes nothing
    micro = V.VitConfig(num_classes=3, global_pool=True,
                        **{k: MICRO[k] for k in ('volume_size', 'patch_size', 'in_chans', 'embed_dim', 'depth', 'num_heads')})
    with pytest.raises(VitaeError):                                   # embed 48, head size 16
        _module(micro, 'bf16', 'bf16')
    with pytest.raises(VitaeError):
        _module(micro, 'bf16').set_precision('bf16', activations='bf16')
    with pytest.raises(VitaeError):                                   # head size 16 alone
        _module(V.VitConfig(num_classes=3, num_heads=4, **ENC), 'bf16', 'bf16')
    with pytest.raises(VitaeError):                                   # in_chans * patch^3 = 2 * 27
        _module(V.VitConfig(num_classes=3, num_heads=2, **dict(ENC, patch_size=3, volume_size=(12, 12, 12), in_chans=2)), 'bf16', 'bf16')
    for bad in ('fp32', 'bf16x', '', 16):
        with pytest.raises(VitaeError):
            _module(ok, 'bf16', bad)
        with pytest.raises(VitaeError):
            m.set_precision('bf16', activations=bad)


# ----------------------------------------------------------------------------------------------- GPU: kernel
GUARD, SENT = 64, 7.25           # SENT is exact in bf16
FACTOR, FLOOR = 3.0, 4.0 * 2.0 ** -24
KSHAPES = [(3, 65, 64), (4, 217, 768), (1, 513, 1024)]


def _kernel_buffers(B, N, D, Mp):
    dx = torch.full((B * N * D + GUARD,), SENT, device='cuda')
    dx16 = torch.full((Mp * D + GUARD,), SENT, dtype=torch.bfloat16, device='cuda')
    cs = torch.full((D + GUARD,), SENT, device='cuda')
    return dx, dx16, cs


@pytest.mark.gpu
@pytest.mark.parametrize('B,N,D', KSHAPES)
@pytest.mark.parametrize('mode', [0, 1])
def test_token_select_bwd16_kernel(B, N, D, mode):
    from vit_ae_plus_plus_amd._abi import lib
    M = B * N
    Mp = (M + 63) // 64 * 64
    assert Mp > M                                                     # every shape has pad rows
    g = torch.Generator().manual_seed(B * 1000 + N + mode)
    dsel = torch.randn(B, D, generator=g).cuda()
    st = torch.cuda.current_stream().cuda_stream
    old = torch.full((M, D), float('nan'), device='cuda')
    lib.vitae_token_select_bwd(dsel.data_ptr(), old.data_ptr(), B, N, D, mode, st)

    def run():
        dx, dx16, cs = _kernel_buffers(B, N, D, Mp)
        lib.vitae_token_select_bwd16(dsel.data_ptr(), dx.data_ptr(), dx16.data_ptr(), cs.data_ptr(), B, N, Mp, D, mode, st)
        torch.cuda.synchronize()
        return dx.cpu(), dx16.cpu(), cs.cpu()

    dx, dx16, cs = run()
    for buf, n in ((dx, M * D), (dx16, Mp * D), (cs, D)):             # nothing behind an output is touched
        assert bool((buf[n:].float() == SENT).all())
    dxm, dx16m = dx[:M * D].view(M, D), dx16[:Mp * D].view(Mp, D)
    assert torch.equal(dxm, old.cpu())                                # bit for bit what vitae_token_select_bwd writes
    assert torch.equal(dx16m[:M].view(torch.int16), dxm.bfloat16().view(torch.int16))
    assert bool((dx16m[M:].view(torch.int16) == 0).all())             # the pad rows, which started as the sentinel
    # column sums of the written dx
    s64 = dxm.double().sum(0)
    scale = dxm.double().abs().sum(0)
    s32 = torch.from_numpy(dxm.numpy().sum(axis=0, dtype=np.float32))
    ratio = lambda s: float(torch.where(scale > 0, (s.double() - s64).abs() / scale.clamp_min(1e-300),
                                        (s.double() != s64).double() * float('inf')).nan_to_num(nan=0.0).max())
    e, e32 = ratio(cs[:D]), ratio(s32)
    print(f'RATIO token_select_bwd16 colsum B={B} N={N} D={D} mode={mode}: e={e:.3e} e32={e32:.3e}')
    assert e <= max(FACTOR * e32, FLOOR), (e, e32)
    again = run()
    assert all(torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a, b.view(torch.int16) if b.dtype == torch.bfloat16 else b)
               for a, b in zip((dx, dx16, cs), again))                # no atomics: the same bits
    # colsum is optional
    dx2, dx162, cs2 = _kernel_buffers(B, N, D, Mp)
    lib.vitae_token_select_bwd16(dsel.data_ptr(), dx2.data_ptr(), dx162.data_ptr(), None, B, N, Mp, D, mode, st)
    torch.cuda.synchronize()
    assert torch.equal(dx2.cpu(), dx) and torch.equal(dx162.cpu().view(torch.int16), dx16.view(torch.int16))


@pytest.mark.gpu
def test_token_select_bwd16_refusals_write_nothing():
    from vit_ae_plus_plus_amd._abi import lib
    dll = lib.load()
    INVALID, UNSUPPORTED = -1, -2
    B, N, D, Mp = 3, 65, 64, 256
    dsel = torch.randn(B, D, device='cuda')
    dx, dx16, cs = _kernel_buffers(B, N, D, Mp)
    before = [t.clone() for t in (dsel, dx, dx16, cs)]
    s, x, x16, c = dsel.data_ptr(), dx.data_ptr(), dx16.data_ptr(), cs.data_ptr()
    cases = [((None, x, x16, c, B, N, Mp, D, 1), INVALID), ((s, None, x16, c, B, N, Mp, D, 1), INVALID),
             ((s, x, None, c, B, N, Mp, D, 1), INVALID),
             ((s, x, x16, c, 0, N, Mp, D, 1), INVALID), ((s, x, x16, c, B, 0, Mp, D, 1), INVALID),
             ((s, x, x16, c, B, N, Mp, 0, 1), INVALID), ((s, x, x16, c, B, N, 0, D, 1), INVALID),
             ((s, x, x16, c, -1, N, Mp, D, 0), INVALID), ((s, x, x16, c, B, N, -64, D, 0), INVALID),
             ((s, x, x16, c, B, N, 192, D, 1), INVALID),              # Mpad < B N = 195
             ((s, x, x16, c, B, N, 200, D, 1), INVALID),              # not a multiple of 64
             ((s, x, x16, c, B, N, Mp, D, 2), INVALID), ((s, x, x16, c, B, N, Mp, D, -1), INVALID),
             ((s, x, x16, c, B, 1, Mp, D, 1), INVALID),               # a mean over no token
             ((s + 4, x, x16, c, B, N, Mp, D, 1), INVALID), ((s, x, x16 + 2, c, B, N, Mp, D, 1), INVALID),     # misaligned
             ((s, x, x16, c, B, N, Mp, 60, 1), UNSUPPORTED)]          # D % 8
    for args, rc in cases:
        assert dll.vitae_token_select_bwd16(*args, None) == rc, args
    torch.cuda.synchronize()
    for t, b in zip((dsel, dx, dx16, cs), before):
        assert torch.equal(t.view(torch.int16) if t.dtype == torch.bfloat16 else t, b.view(torch.int16) if b.dtype == torch.bfloat16 else b)


# ----------------------------------------------------------------------------------------------- GPU: route
def _micro(name, gp, activations, **kw):
    cfg = _cfg(name, gp)
    m = _module(cfg, 'bf16', activations, **kw).cuda().train()
    m.load_state_dict(V.init_vit_state_dict(cfg, seed=5))
    return m


def _grads(m):
    return {n: (None if p.grad is None else p.grad.detach().cpu().numpy()) for n, p in m.named_parameters()}


def _step(m, x, y, crit):
    m.zero_grad(set_to_none=True)
    logits = m(x)
    loss = crit(logits, y)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), logits.detach().cpu().numpy(), _grads(m)


def _data(gold):
    return (torch.from_numpy(gold['x']).cuda(), torch.from_numpy(gold['labels']).cuda(),
            torch.nn.CrossEntropyLoss(weight=torch.from_numpy(gold['class_weights']).cuda()))


def _both_routes(gold, name, gp, prepare=None):
    """One forward + backward of the new route and of the existing bf16 route on the same weights and input."""
    x, y, crit = _data(gold)
    out = []
    for act in ('bf16', None):
        m = _micro(name, gp, act)
        if prepare:
            prepare(m)
        out.append(_step(m, x, y, crit) + (m,))
        assert m._trainer.stats['route'] == ('bf16-activations' if act else 'fp32-activations')
    return out


def _check_gradient_rule(exp, g_new, g_old, label, names=None):
    worst, needed_old = (0.0, None), []
    for n in names or exp['names']:
        assert g_new[n] is not None and np.isfinite(g_new[n]).all(), n
        e_new, e_old, e_ref = _rel(g_new[n], exp['grad'][n]), _rel(g_old[n], exp['grad'][n]), exp['relerr'][n]
        bound = 2.0 * max(e_ref, e_old)
        print(f'{label} {n}: new route {e_new:.3e}, existing route {e_old:.3e}, reference under autocast {e_ref:.3e}, '
              f'new / bound {e_new / bound:.2f}')
        if e_new > 2.0 * e_ref:
            needed_old.append(n)
        worst = max(worst, (e_new / bound, n))
    print(f'{label}: needed the existing-route term: {needed_old}')
    assert worst[0] <= 1.0, worst


@pytest.mark.gpu
@pytest.mark.parametrize('name,gp', PAIRS, ids=PAIR_IDS)
def test_route_gradients_and_logits(gold, name, gp):
    exp = _expect(gold, name, gp)
    (l_new, y_new, g_new, m_new), (l_old, y_old, g_old, _) = _both_routes(gold, name, gp)
    assert sorted(g_new.keys()) == sorted(exp['names'])               # no parameter is left out
    e_new, e_old = float(np.abs(y_new - exp['logits']).max()), float(np.abs(y_old - exp['logits']).max())
    print(f'{name}/{TAGS[gp]} logits: new route {e_new:.3e}, existing route {e_old:.3e}, reference under autocast {exp["logits_err"]:.3e}; '
          f'loss {l_new} / {l_old} (fp32 {exp["loss"]})')
    assert np.isfinite(l_new)
    assert e_new <= 2.0 * max(exp['logits_err'], e_old)
    _check_gradient_rule(exp, g_new, g_old, f'{name}/{TAGS[gp]}')
    assert m_new._trainer.stats['kept_bytes'] > 0 and m_new._trainer.stats['forwards'] == 1 and m_new._trainer.stats['backwards'] == 1


@pytest.mark.gpu
@pytest.mark.parametrize('name,gp', PAIRS, ids=PAIR_IDS)
def test_route_adamw_trajectory(gold, name, gp):
    exp = _expect(gold, name, gp)
    x, y, crit = _data(gold)
    dev = {}
    for act in ('bf16', None):
        m = _micro(name, gp, act)
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=0.05)
        losses = []
        for _ in range(4):
            opt.zero_grad()
            loss = crit(m(x), y)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        dev[act] = np.abs(np.array(losses) - exp['adamw_losses'])
        print(f'{name}/{TAGS[gp]} AdamW losses, activations={act}: {losses} (fp32 {list(exp["adamw_losses"])}); deviation {list(dev[act])}')
    print(f'reference under autocast deviates by {list(exp["adamw_dev"])}')
    assert np.isfinite(dev['bf16']).all()
    bound = 2.0 * np.maximum(np.asarray(exp['adamw_dev']), dev[None])
    print(f'new / bound per step: {list(np.round(dev["bf16"] / bound, 2))}')
    assert (dev['bf16'] <= bound).all(), (list(dev['bf16']), list(bound))


@pytest.mark.gpu
@pytest.mark.parametrize('name,gp', STORED, ids=[f'{n}-{TAGS[g]}' for n, g in STORED])
def test_route_frozen_parameters(gold, name, gp):
    exp = _expect(gold, name, gp)
    x, y, crit = _data(gold)
    full = _micro(name, gp, 'bf16')
    _, _, g_full = _step(full, x, y, crit)
    kept_full = full._trainer.stats['kept_bytes']
    # block 0 and the embeddings frozen: block 1 issues the launches of the all-trainable run
    frozen = lambda n: n.startswith(('patch_embed.', 'blocks.0.')) or n in ('pos_embed', 'cls_token')
    m = _micro(name, gp, 'bf16')
    for n, p in m.named_parameters():
        p.requires_grad = not frozen(n)
    _, _, g_part = _step(m, x, y, crit)
    assert 0 < m._trainer.stats['kept_bytes'] < kept_full
    for n in g_full:
        if frozen(n):
            assert g_part[n] is None, n
        else:
            assert _rel(g_part[n], g_full[n]) <= 1e-6, n
    # every Linear weight frozen, biases and norms trainable: dw = NULL in every paired launch, the fc1 and qkv bias gradients come
    # from other launches than in the all-trainable run.  The gradient rule against fp32, the existing route frozen the same way.
    is_w = lambda n: n.endswith('.weight') and 'norm' not in n and not n.startswith('head.')

    def freeze(mod):
        for n, p in mod.named_parameters():
            p.requires_grad = not is_w(n)

    (_, _, g_new, _), (_, _, g_old, _) = _both_routes(gold, name, gp, prepare=freeze)
    assert all(g_new[n] is None for n in g_new if is_w(n)) and any(is_w(n) for n in g_new)
    _check_gradient_rule(exp, g_new, g_old, f'{name}/{TAGS[gp]} weights frozen', names=[n for n in exp['names'] if not is_w(n)])
    # the whole encoder frozen: the inference path runs, nothing is kept
    m = _micro(name, gp, 'bf16')
    for n, p in m.named_parameters():
        p.requires_grad = n.startswith('head.')
    loss, _, g_head = _step(m, x, y, crit)
    assert m._trainer is None and np.isfinite(loss)
    assert all((g is not None) == n.startswith('head.') for n, g in g_head.items())


@pytest.mark.gpu
def test_route_dirty_pad_rows(gold):
    """B = 3 (195 rows in 256), then B = 1 (65 rows in 128) on ONE trainer: rows 65 .. 127 of every bf16 operand must be zero again."""
    x, y, crit = _data(gold)
    fresh = _micro('h32', True, 'bf16')
    _, _, g_fresh = _step(fresh, x[:1], y[:1], crit)
    m = _micro('h32', True, 'bf16')
    _step(m, x, y, crit)
    _, _, g = _step(m, x[:1], y[:1], crit)
    assert m._trainer.stats['forwards'] == 2
    for n in g_fresh:
        assert _rel(g[n], g_fresh[n]) <= 1e-6, n


@pytest.mark.gpu
def test_route_two_forwards_then_two_backwards(gold):
    x, y, crit = _data(gold)
    xa, ya = x, y
    xb, yb = (x.flip(0) * 0.5 + 0.1).contiguous()[:2], y[:2]          # another input, another batch size (130 rows in 192)
    m = _micro('h64', True, 'bf16')
    _, _, ga = _step(m, xa, ya, crit)
    _, _, gb = _step(m, xb, yb, crit)
    m.zero_grad(set_to_none=True)
    la, lb = crit(m(xa), ya), crit(m(xb), yb)
    lb.backward()                                                     # reverse order
    g2 = _grads(m)
    m.zero_grad(set_to_none=True)
    la.backward()
    g1 = _grads(m)
    torch.cuda.synchronize()
    for n in ga:
        assert _rel(g1[n], ga[n]) <= 1e-6 and _rel(g2[n], gb[n]) <= 1e-6, n


@pytest.mark.gpu
def test_route_refuses_stale_and_repeated_backward(gold):
    from vit_ae_plus_plus_amd._abi import VitaeError
    x, y, crit = _data(gold)
    m = _micro('h32', False, 'bf16')
    loss = crit(m(x), y)
    with torch.no_grad():
        m.blocks[1].mlp.fc2.weight.mul_(1.0)
    with pytest.raises(VitaeError):
        loss.backward()
    m = _micro('h32', False, 'bf16')
    feat = m.forward_features(x)
    feat.sum().backward(retain_graph=True)
    with pytest.raises(VitaeError):
        feat.sum().backward()
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_route_one_epoch_through_train_one_epoch(gold):
    """Soft targets, accum_iter = 2, AdamW over layer-decay groups.  Both losses of the epoch are taken at the initial weights (the
    step follows the second batch), so the logged loss of either route is a bf16 evaluation of one fp32 number: each deviates from
    it by about what the reference's autocast loss does (``bf16_ref_adamw_dev``, its largest step), and the new route's loss is held to
    the gradient rule's margin — twice that — of the existing route's."""
    from vit_ae_plus_plus_amd.post_training_utils.fine_tune_epoch import train_one_epoch
    from vit_ae_plus_plus_amd.utils.custom_loss import SoftCrossEntropyWithWeightsLoss
    from vit_ae_plus_plus_amd.utils.lr_decay import param_groups_lrd
    from vit_ae_plus_plus_amd.utils.misc import NativeScalerWithGradNormCount
    exp = _expect(gold, 'h64', True)
    x = torch.from_numpy(gold['x'])
    g = torch.Generator().manual_seed(23)
    t0, t1 = (torch.softmax(2.0 * torch.randn(3, 3, generator=g), dim=-1) for _ in range(2))
    batches = [(x, None, t0), (x.flip(0).contiguous(), None, t1)]
    args = Namespace(accum_iter=2, lr=1e-3, min_lr=0.0, warmup_epochs=1, epochs=4)
    stats = {}
    for act in ('bf16', None):
        m = _micro('h64', True, act)
        before = {n: p.detach().clone() for n, p in m.named_parameters()}
        opt = torch.optim.AdamW(param_groups_lrd(m, 0.05, no_weight_decay_list=m.no_weight_decay(), layer_decay=0.75), lr=args.lr)
        crit = SoftCrossEntropyWithWeightsLoss(torch.from_numpy(gold['class_weights'])).cuda()
        stats[act] = train_one_epoch(m, crit, batches, opt, torch.device('cuda'), 1, NativeScalerWithGradNormCount(), max_norm=None,
                                     args=args)
        assert m._trainer.stats['route'] == ('bf16-activations' if act else 'fp32-activations')
        assert m._trainer.stats['forwards'] == 2 and m._trainer.stats['backwards'] == 2
        assert all(not torch.equal(p.detach(), before[n]) for n, p in m.named_parameters())      # the step was taken
    print('epoch stats', stats, 'reference autocast loss deviation', list(exp['adamw_dev']))
    assert np.isfinite(stats['bf16']['loss'])
    assert abs(stats['bf16']['loss'] - stats[None]['loss']) <= 2.0 * exp['adamw_dev'].max()


@pytest.fixture(scope='module')
def vitb_oracle():
    """Loss and per-parameter gradient norms of ViT-B/16 on 96^3 x 4ch, batch 2, from the oracle's autograd on the CPU (the
    construction of tests/test_vit_finetune.py)."""
    cfg = V.VitConfig(num_classes=2, global_pool=True, **VITB)
    sd = {k: v.clone().requires_grad_(True) for k, v in V.init_vit_state_dict(cfg, seed=7).items()}
    xb, _ = R.synthetic_views((2, 4, 96, 96, 96), seed=1234)
    y = torch.tensor([1, 0])
    loss = torch.nn.functional.cross_entropy(V.forward(sd, xb, cfg), y)
    loss.backward()
    return cfg, xb, y, float(loss.detach()), {k: float(v.grad.double().norm()) for k, v in sd.items()}


@pytest.mark.gpu
def test_route_vitb(vitb_oracle):
    """The shape users run (434 rows in 448, D = 768: tiles and splits the micro configurations never reach).  Per parameter the
    error of the gradient norm <= 2 x max(the existing bf16 route's, the fp32 route's bound 2e-3); kept bytes below 0.7 x the
    existing route's (40 D against 64 D bytes per row and block = 0.625, times 448 / 434 for the padded operands)."""
    cfg, xb, y, ref_loss, ref_norms = vitb_oracle
    res = {}
    for act in ('bf16', None):
        m = _module(cfg, 'bf16', act).cuda().train()
        m.load_state_dict(V.init_vit_state_dict(cfg, seed=7))
        loss, _, grads = _step(m, xb.cuda(), y.cuda(), torch.nn.CrossEntropyLoss())
        errs = {}
        for n, refn in ref_norms.items():
            assert grads[n] is not None and np.isfinite(grads[n]).all(), n
            errs[n] = abs(float(np.linalg.norm(grads[n].astype(np.float64))) - refn) / refn
        res[act] = (loss, errs, m._trainer.stats['kept_bytes'], grads)
        del m
    (l_new, e_new, k_new, g_new), (l_old, e_old, k_old, g_old) = res['bf16'], res[None]
    # Norms do not see a sign or a permutation.  The oracle's ViT-B gradients themselves are not kept (345 MB), so the direction is
    # checked between the two routes: both are bf16 evaluations of one fp32 gradient and differ by the sum of their errors (1e-2 .. 1e-1
    # at this depth), while a flipped sign gives a relative L2 distance of 2 and rows or columns in another order give about sqrt(2).
    # 0.5 lies between.  The key third of attn.qkv.bias is left out: its gradient is zero in exact arithmetic (softmax ignores a shift
    # common to all keys), so what either route holds there is rounding noise (tests/test_vit_finetune.py).
    D = cfg.embed_dim
    far = (0.0, None)
    for n in ref_norms:
        a, b = g_new[n], g_old[n]
        if n.endswith('attn.qkv.bias'):
            a, b = np.delete(a, np.s_[D:2 * D]), np.delete(b, np.s_[D:2 * D])
        far = max(far, (_rel(a, b), n))
    print(f'ViT-B: largest relative L2 distance between the routes\' gradients {far[0]:.3e} ({far[1]})')
    assert far[0] <= 0.5, far
    worst, needed_old = (0.0, None), []
    for n in ref_norms:
        bound = 2.0 * max(e_old[n], 2e-3)
        worst = max(worst, (e_new[n] / bound, n))
        if e_new[n] > 2.0 * 2e-3:
            needed_old.append(n)
    print(f'ViT-B: loss new {l_new} / existing {l_old} (oracle {ref_loss}); worst new / bound {worst[0]:.2f} ({worst[1]}); worst errors '
          f'new {max(e_new.values()):.2e} existing {max(e_old.values()):.2e}; kept {k_new / 2 ** 20:.1f} / {k_old / 2 ** 20:.1f} MiB '
          f'= {k_new / k_old:.3f}; above 2 x 2e-3, i.e. passing on the existing-route term: {len(needed_old)} of {len(ref_norms)} parameters')
    assert np.isfinite(l_new)
    assert worst[0] <= 1.0, worst
    assert k_new < 0.7 * k_old
