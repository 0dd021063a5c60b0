"""``builder.MoCo_ResNet`` — MoCo v3 over this package's 3-D ResNet, the two views through the launch sequence one after the other —
against the reference's own ``MoCo_ResNet`` (tests/golden/moco_resnet.npz, tools/gen_moco_resnet_golden.py: micro ResNet-10 of widths
4 / 8 / 16 / 32, dim 16, mlp_dim 64, 16 samples of 1 x 32^3 per view, m = 0.99, three LARS steps, T = 1.0 and 0.2).

Parity is the project's rule for the bf16 routes (tests/test_resnet3d_model.py): the reference's own ``torch.autocast('cpu', bfloat16)``
run is the yardstick.  Each loss within 2 x that run's absolute gap from the float64 run, every step-1 gradient within 2 x ``gap16``
(relative L2 per parameter), every running statistic after step 1 within 2 x the autocast run's own max-norm distance from float64, per
tensor.  A gross-error check: there is no fp32 ResNet route that could be held to 1e-4.  ``RATIO`` lines are printed (run with -s).

Everything else is exact: the model's step equals the same statement written out with the package's public pieces, bit for bit; the
momentum update equals the torch statement; ``forward_features(batch_stats=True)`` gives the training node's bits and keeps nothing;
two fresh models repeat each other's bits; ``GradScaler`` gives the plain run's gradients to 1e-6 (scaling by 2^10 is exact up to the
rounding of values that leave the normal range) and skips a step with an inf gradient."""
import copy
import math
import os
import sys
from functools import partial

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'moco_resnet.npz')
TEMPS = [1.0, 0.2]


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD, allow_pickle=False)


def encoder_factory(z=None, depth=10, **kw):
    from vit_ae_plus_plus_amd.other_baselines.mocov3.moco.resent3d_base import generate_model
    wf = 0.0625 if z is None else float(z['widen_factor'])
    return partial(generate_model, model_depth=depth, n_input_channels=1, widen_factor=wf, **kw)


def make_model(T=1.0, z=None):
    from vit_ae_plus_plus_amd.other_baselines.mocov3.moco.builder import MoCo_ResNet
    return MoCo_ResNet(encoder_factory(z), 16, 64, T)


def init_state(z):
    """the fixture's initial state for the whole model: the momentum encoder starts as the base encoder"""
    sd = {}
    for n in z['names']:
        n = str(n)
        src = 'base_encoder.' + n[len('momentum_encoder.'):] if n.startswith('momentum_encoder.') else n
        sd[n] = torch.from_numpy(z['init/' + src]).clone()
    return sd


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


_VIEWS = {}


def views(z):
    """The two views from the frozen legacy stream, checked against the fixture's sums and samples before anything uses them."""
    if 'v' not in _VIEWS:
        B, C, V, _ = (int(v) for v in z['config'])
        rs = np.random.RandomState(int(z['seed']))
        x1 = rs.standard_normal((B, C, V, V, V))
        x2 = x1 + 0.3 * rs.standard_normal((B, C, V, V, V))
        x1, x2 = x1.astype(np.float32), x2.astype(np.float32)
        for i, x in enumerate((x1, x2)):
            assert math.fsum(x.reshape(-1).tolist()) == z['view_sum'][i]          # exactly rounded: no summation order in it
            assert np.array_equal(x.reshape(-1)[z['view_index']], z['view_samples'][i])
        _VIEWS['v'] = (x1, x2)
    return _VIEWS['v']


# ---------------------------------------------------------------------------- CPU
def test_fixture_is_small_and_complete(gold):
    assert os.path.getsize(GOLD) < 1 << 20
    names = [str(n) for n in gold['names']]
    assert len(names) == 171 and len(gold['shapes']) == 171
    assert [int(v) for v in gold['config']] == [16, 1, 32, 3] and [int(v) for v in gold['dims']] == [16, 64]
    assert float(gold['m']) == 0.99 and list(gold['lars']) == [0.3, 1e-6, 0.9] and list(gold['temps']) == TEMPS
    trainable = [n for n in names if not n.startswith('momentum_encoder.') and 'running_' not in n and 'num_batches' not in n]
    for n in names:
        if not n.startswith('momentum_encoder.'):
            assert 'init/' + n in gold.files, n
    for T in TEMPS:
        for k in ('losses64', 'losses32', 'losses16'):
            assert gold[f'T{T}/{k}'].shape == (3,)
        gaps = np.abs(gold[f'T{T}/losses16'] - gold[f'T{T}/losses64'])
        assert gaps.min() >= 0.25 * gaps.max()                                      # the generator's criterion for the seed
        for n in trainable:
            assert all(f'T{T}/{k}/{n}' in gold.files for k in ('grad64', 'gap32', 'gap16')), n
            assert float(gold[f'T{T}/gap32/{n}']) < 1e-4 and float(gold[f'T{T}/gap32/{n}']) < float(gold[f'T{T}/gap16/{n}'])
        for n in names:
            if 'running_' in n or 'num_batches' in n:
                assert f'T{T}/stat64/{n}' in gold.files and f'T{T}/stat16/{n}' in gold.files, n
    views(gold)


def test_state_dict_keys_and_shapes_are_the_references(gold):
    model = make_model()
    sd = model.state_dict()
    assert list(sd.keys()) == [str(n) for n in gold['names']]
    assert [','.join(str(s) for s in v.shape) for v in sd.values()] == [str(s) for s in gold['shapes']]
    assert sum(p.numel() for p in model.parameters()) == 123976
    for enc in ('base_encoder', 'momentum_encoder'):
        for k in ('conv1.weight', 'bn1.running_mean', 'layer2.0.downsample.0.weight', 'layer4.0.bn2.bias', 'fc.0.weight', 'fc.1.weight',
                  'fc.1.running_var', 'fc.3.weight', 'fc.4.running_mean', 'fc.4.running_var', 'fc.4.num_batches_tracked'):
            assert f'{enc}.{k}' in sd, k
        assert f'{enc}.fc.4.weight' not in sd and f'{enc}.fc.4.bias' not in sd and f'{enc}.fc.weight' not in sd      # BatchNorm1d(affine=False)
    assert sd['base_encoder.fc.0.weight'].shape == (64, 32) and sd['base_encoder.fc.3.weight'].shape == (16, 64)
    assert sd['predictor.0.weight'].shape == (64, 16) and sd['predictor.3.weight'].shape == (16, 64) and 'predictor.1.running_var' in sd
    assert not any(k.startswith('predictor.4.') for k in sd)                        # no last BatchNorm, unlike MoCo_ViT
    assert len(model.predictor) == 4 and len(model.base_encoder.fc) == 5


def test_momentum_encoder_starts_equal_and_frozen():
    torch.manual_seed(1)
    model = make_model()
    b, m = model.base_encoder.state_dict(), model.momentum_encoder.state_dict()
    assert list(b) == list(m) and all(torch.equal(b[k], m[k]) for k in b)
    assert all(p.data_ptr() != q.data_ptr() for p, q in zip(model.base_encoder.parameters(), model.momentum_encoder.parameters()))
    assert all(not p.requires_grad for p in model.momentum_encoder.parameters())
    assert all(p.requires_grad for p in model.base_encoder.parameters()) and all(p.requires_grad for p in model.predictor.parameters())
    assert model.T == 1.0 and callable(model.contrastive_loss) and callable(model._update_momentum_encoder)


def test_resent3d_base_is_the_package_resnet_with_num_classes():
    from vit_ae_plus_plus_amd.k_fold_training_scripts import resnet_3d as R
    from vit_ae_plus_plus_amd.other_baselines.mocov3.moco import resent3d_base as B
    m = B.generate_model(10, num_classes=7)
    assert isinstance(m, R.ResNet) and m.fc.out_features == 7 and m.fc.in_features == 512
    assert B.get_inplanes() == [64, 128, 256, 512] and B.BasicBlock is R.BasicBlock and B.Bottleneck is R.Bottleneck
    torch.manual_seed(5)
    a = B.generate_model(10, num_classes=3, n_input_channels=1, widen_factor=0.0625)
    torch.manual_seed(5)
    b = R.generate_model(10, n_classes=3, n_input_channels=1, widen_factor=0.0625)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)      # keys, shapes, initialisation
    for depth in (50, 101, 152, 200):
        with pytest.raises(NotImplementedError):
            B.generate_model(depth)
    with pytest.raises(AssertionError):
        B.generate_model(11)
    with pytest.raises(NotImplementedError):
        B.generate_model(10, shortcut_type='A')
    with pytest.raises(NotImplementedError):
        B.ResNet(B.Bottleneck, [3, 4, 6, 3], B.get_inplanes())
    with pytest.raises(NotImplementedError):
        B.generate_model(10, widen_factor=0.05)
    with pytest.raises(TypeError):
        B.generate_model(10, n_classes=2)                                           # the keyword of the other copy


def test_dropin_alias():
    from vit_ae_plus_plus_amd import dropin
    saved = {k: sys.modules.get(k) for k in dropin._ALIASES}
    try:
        dropin.install(force=True)
        import other_baselines.mocov3.moco.resent3d_base as r
        import other_baselines.mocov3.moco.builder as b
        import vit_ae_plus_plus_amd.other_baselines.mocov3.moco.resent3d_base as r2
        assert r is r2 and callable(r.generate_model) and callable(b.MoCo_ResNet)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_refused_encoders():
    from vit_ae_plus_plus_amd.model.vit import VisionTransformer3D
    from vit_ae_plus_plus_amd.other_baselines.mocov3.moco.builder import MoCo_ResNet

    class TorchResNet(torch.nn.Module):
        def __init__(self, num_classes):
            super().__init__()
            self.conv1 = torch.nn.Conv3d(1, 4, 3)
            self.fc = torch.nn.Linear(4, num_classes)

    for factory in (lambda num_classes: None, TorchResNet, encoder_factory(depth=50),
                    partial(VisionTransformer3D, volume_size=8, patch_size=4, in_chans=1, embed_dim=64, depth=2, num_heads=2)):
        with pytest.raises(NotImplementedError):
            MoCo_ResNet(factory, 16, 64)


def test_cpu_input_raises():
    from vit_ae_plus_plus_amd._abi import VitaeError
    model = make_model()
    x = torch.zeros(2, 1, 16, 16, 16)
    with pytest.raises(VitaeError, match='no CPU fallback'):
        model(x, x, 0.99)
    with pytest.raises(VitaeError, match='no CPU fallback'):
        model.eval()(x, x, 0.99)
    with pytest.raises(VitaeError, match='no CPU fallback'):
        model.base_encoder.train().forward_features(x)


def test_reference_checkpoint_loads_strictly(gold):
    model = make_model()
    init = init_state(gold)
    assert list(init) == [str(n) for n in gold['names']]
    model.load_state_dict(init, strict=True)
    out = model.state_dict()
    assert all(torch.equal(out[k], v) for k, v in init.items())
    assert all(not p.requires_grad for p in model.momentum_encoder.parameters())


# ---------------------------------------------------------------------------- GPU
def gpu_model(z, T):
    model = make_model(T, z)
    model.load_state_dict(init_state(z))
    return model.cuda().train()


def gpu_views(z):
    x1, x2 = views(z)
    return torch.from_numpy(x1).cuda(), torch.from_numpy(x2).cuda()


def lars_for(model, z):
    from vit_ae_plus_plus_amd.other_baselines.mocov3.moco.optimizer import LARS
    lr, wd, mom = (float(v) for v in z['lars'])
    return LARS(model.parameters(), lr, weight_decay=wd, momentum=mom)


_RUNS = {}


def run(z, T):
    """three LARS steps from the fixture's state, computed once per temperature: losses, step-1 gradients and buffers (all on the CPU)"""
    if T not in _RUNS:
        model = gpu_model(z, T)
        opt = lars_for(model, z)
        x1, x2 = gpu_views(z)
        r = dict(losses=[], loss_bits=[], grads3=[])
        for step in range(int(z['config'][3])):
            opt.zero_grad()
            loss = model(x1, x2, float(z['m']))
            loss.backward()
            r['losses'].append(float(loss))
            r['loss_bits'].append(loss.detach().cpu())
            r['grads3'].append({n: p.grad.detach().cpu().clone() for n, p in model.named_parameters() if p.grad is not None})
            if step == 0:
                r['stats'] = {n: b.detach().cpu().clone() for n, b in model.named_buffers()}
            opt.step()
        r['grads'] = r['grads3'][0]
        _RUNS[T] = r
    return _RUNS[T]


@pytest.mark.gpu
@pytest.mark.parametrize('T', TEMPS)
def test_within_twice_the_references_autocast_gap(gold, T):
    z, r, tag = gold, run(gold, T), f'T{T}/'
    l64, l16 = z[tag + 'losses64'], z[tag + 'losses16']
    outside = []
    for i, got in enumerate(r['losses']):
        e, gap = abs(got - l64[i]), abs(l16[i] - l64[i])
        print(f'RATIO moco_resnet T{T} loss step {i}: got {got:.6f} f64 {l64[i]:.6f} e={e:.3e} gap16={gap:.3e} ratio={e / gap:.2f}')
        if not (np.isfinite(got) and e <= 2 * gap):
            outside.append((f'loss {i}', e, gap))
    trainable = [n for n in (str(n) for n in z['names']) if tag + 'grad64/' + n in z.files]
    assert sorted(r['grads']) == sorted(trainable)
    worst = 0.0
    for n in trainable:
        e, gap = rel_l2(r['grads'][n], z[tag + 'grad64/' + n]), float(z[tag + 'gap16/' + n])
        worst = max(worst, e / gap)
        print(f'RATIO moco_resnet T{T} grad {n}: e={e:.3e} gap16={gap:.3e} ratio={e / gap:.2f}')
        if not e <= 2 * gap:
            outside.append((n, e, gap))
    print(f'RATIO moco_resnet T{T} worst gradient ratio {worst:.2f} of the allowed 2')
    for n in (str(n) for n in z['names']):
        if tag + 'stat64/' + n not in z.files:
            continue
        got, s64, s16 = r['stats'][n], z[tag + 'stat64/' + n], z[tag + 'stat16/' + n]
        if n.endswith('num_batches_tracked'):
            assert int(got) == int(s64) == 2, n                                     # both views counted
            continue
        e = float(np.abs(got.double().numpy() - s64.astype(np.float64)).max())
        gap = float(np.abs(s16.astype(np.float64) - s64.astype(np.float64)).max())
        print(f'RATIO moco_resnet T{T} stat {n}: e={e:.3e} gap16={gap:.3e} ratio={e / gap if gap else float("inf"):.2f}')
        if not e <= 2 * gap:
            outside.append((n, e, gap))
    assert not outside, outside


@pytest.mark.gpu
def test_forward_is_the_written_out_statement_bit_for_bit(gold):
    from vit_ae_plus_plus_amd.other_baselines.mocov3.moco.builder import _MocoLoss, run_mlp
    T, m = 0.2, float(gold['m'])
    model = gpu_model(gold, T)
    x1, x2 = gpu_views(gold)
    with torch.no_grad():                                                           # momentum encoder != base encoder, so that roles show
        for p in model.momentum_encoder.parameters():
            p.mul_(0.75)
    twin = copy.deepcopy(model)
    loss = model(x1, x2, m)
    loss.backward()
    # the same step with the public pieces
    b, me = twin.base_encoder, twin.momentum_encoder
    q1 = run_mlp(twin.predictor, run_mlp(b.fc, b.forward_features(x1)))
    q2 = run_mlp(twin.predictor, run_mlp(b.fc, b.forward_features(x2)))
    with torch.no_grad():
        twin._update_momentum_encoder(m)
        k1 = run_mlp(me.fc, me.forward_features(x1, batch_stats=True))
        k2 = run_mlp(me.fc, me.forward_features(x2, batch_stats=True))
    want = _MocoLoss.apply(q1, k2, q2, k1, T)
    want.backward()
    torch.cuda.synchronize()
    assert loss.dim() == 0 and torch.equal(loss.detach(), want.detach())
    n_grads = 0
    for (n, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
        assert torch.equal(p.detach(), q.detach()), n
        assert (p.grad is None) == (q.grad is None) == (not p.requires_grad), n
        if p.grad is not None:
            assert torch.equal(p.grad, q.grad) and bool(p.grad.abs().sum() > 0), n
            n_grads += 1
    assert n_grads == len(list(model.base_encoder.parameters())) + len(list(model.predictor.parameters()))
    for (n, u), (_, v) in zip(model.named_buffers(), twin.named_buffers()):
        assert torch.equal(u, v), n
    tracked = [(n, mod) for n, mod in model.named_modules() if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm)]
    assert len(tracked) == 2 * (12 + 2) + 1                                         # 12 BatchNorm3d + 2 in fc per encoder, 1 in the predictor
    for n, mod in tracked:
        assert int(mod.num_batches_tracked) == 2, n


@pytest.mark.gpu
def test_momentum_update_is_the_torch_statement(gold):
    m = float(gold['m'])
    model = gpu_model(gold, 1.0)
    opt = lars_for(model, gold)
    x1, x2 = gpu_views(gold)
    model(x1, x2, m).backward()
    opt.step()                                                                      # the encoders differ from here on
    pb = [p.detach().clone() for p in model.base_encoder.parameters()]
    pm = [p.detach().clone() for p in model.momentum_encoder.parameters()]
    bufs = {n: b.detach().clone() for n, b in model.momentum_encoder.named_buffers()}
    versions = [p._version for p in model.momentum_encoder.parameters()]
    model._update_momentum_encoder(m)
    for (n, p), b_, m_, v in zip(model.momentum_encoder.named_parameters(), pb, pm, versions):
        assert torch.equal(p.detach(), m_ * m + b_ * (1. - m)), n
        assert not torch.equal(p.detach(), m_), n
        assert p._version > v, n
    for n, b in model.momentum_encoder.named_buffers():                             # BatchNorm buffers are not averaged
        assert torch.equal(b, bufs[n]), n
    for p, b_ in zip(model.base_encoder.parameters(), pb):
        assert torch.equal(p.detach(), b_)


@pytest.mark.gpu
def test_batch_stats_route(gold):
    from vit_ae_plus_plus_amd._abi import VitaeError
    enc = gpu_model(gold, 1.0).base_encoder
    x = gpu_views(gold)[0]
    twin = copy.deepcopy(enc)
    node = enc.forward_features(x)                                                  # the training node
    assert node.grad_fn is not None and node.shape == (16, 32)
    before = {n: b.detach().clone() for n, b in twin.named_buffers()}
    with torch.no_grad():
        got = twin.forward_features(x, batch_stats=True)
    assert got.grad_fn is None and torch.equal(got, node.detach())                  # same bits on the same weights and buffers
    for (n, u), (_, v) in zip(enc.named_buffers(), twin.named_buffers()):
        if n.startswith('fc.'):
            assert torch.equal(v, before[n]), n                                     # below fc only
            continue
        assert torch.equal(u, v), n                                                 # moved by one update, as the node moves them
        assert not torch.equal(v, before[n]), n
        if n.endswith('num_batches_tracked'):
            assert int(v) == 1
    with torch.no_grad():
        running = twin.forward_features(x)                                          # under no_grad: inference on the running statistics
        twin.eval()
        assert torch.equal(twin.forward_features(x), running)
        twin.train()
    assert not torch.equal(running, got)
    # nothing retained: the allocator is back where it was, up to the returned features
    del got, running, node
    with torch.no_grad():
        twin.forward_features(x, batch_stats=True)                                  # (operand store and workspaces exist from here on)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        f = twin.forward_features(x, batch_stats=True)
        torch.cuda.synchronize()
        after = torch.cuda.memory_allocated()
    assert after - base <= max(512, f.numel() * f.element_size()), (base, after)
    kept = enc.forward_features(x)                                                  # the training node, for scale: it does hold activations
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() - after > 16 * 16 ** 3 * 4 * 4
    del kept
    with pytest.raises(VitaeError, match='no_grad'):
        twin.forward_features(x, batch_stats=True)                                  # gradients enabled
    with torch.no_grad(), pytest.raises(VitaeError, match='train'):
        twin.eval().forward_features(x, batch_stats=True)


@pytest.mark.gpu
def test_two_fresh_models_repeat_bit_for_bit(gold):
    a = run(gold, 0.2)
    _RUNS.pop(0.2)
    b = run(gold, 0.2)
    for step in range(3):
        assert torch.equal(a['loss_bits'][step], b['loss_bits'][step]), step
        assert list(a['grads3'][step]) == list(b['grads3'][step])
        for n, g in a['grads3'][step].items():
            assert torch.equal(g, b['grads3'][step][n]), (step, n)


def _scaled_first_step(z, T=1.0):
    """the reference's loop up to unscale_: -> (model, optimizer, scaler, loss)"""
    model = gpu_model(z, T)
    opt = lars_for(model, z)
    x1, x2 = gpu_views(z)
    scaler = torch.cuda.amp.GradScaler(init_scale=1024.0)
    opt.zero_grad()
    with torch.cuda.amp.autocast(True):             # as the reference's loop; the HIP launchers are not affected by autocast
        loss = model(x1, x2, float(z['m']))
    scaler.scale(loss).backward()
    scaler.unscale_(opt)
    return model, opt, scaler, loss


@pytest.mark.gpu
def test_grad_scaler_loop(gold):
    z, T = gold, 1.0
    plain = run(z, T)
    model, opt, scaler, loss = _scaled_first_step(z, T)
    figures = {n: rel_l2(p.grad, plain['grads'][n]) for n, p in model.named_parameters() if p.grad is not None}
    for n, e in sorted(figures.items(), key=lambda t: -t[1])[:6]:
        print(f'FIGURE scaler {n}: {e:.3g}')
    assert sorted(figures) == sorted(plain['grads'])
    over = {n: e for n, e in figures.items() if e > 1e-6}
    assert not over, over
    scaler.step(opt)
    scaler.update()
    moved = [n for n, p in model.named_parameters() if p.requires_grad and not torch.equal(p.detach().cpu(), torch.from_numpy(z['init/' + n]))]
    # LARS moves a matrix by lr x 0.001 of its norm whatever the gradient's size (a vector by lr x its gradient, which may round away)
    assert {n for n, p in model.named_parameters() if p.requires_grad and p.ndim > 1} <= set(moved)
    assert abs(float(loss) - plain['losses'][0]) <= 1e-6 * plain['losses'][0]
    # a step with an inf gradient: GradScaler finds it and skips; parameters and mu stay as they are
    x1, x2 = gpu_views(z)
    opt.zero_grad()
    loss = model(x1, x2, float(z['m']))
    scaler.scale(loss).backward()
    model.predictor[0].weight.grad[0, 0] = float('inf')
    snap = {n: p.detach().clone() for n, p in model.named_parameters()}
    mus = {n: opt.state[p]['mu'].clone() for n, p in model.named_parameters() if p in opt.state and 'mu' in opt.state[p]}
    scale = scaler.get_scale()
    scaler.step(opt)
    scaler.update()
    assert scaler.get_scale() < scale
    for n, p in model.named_parameters():
        assert torch.equal(p.detach(), snap[n]), n
        if n in mus:
            assert torch.equal(opt.state[p]['mu'], mus[n]), n
    assert mus


@pytest.mark.gpu
def test_eval_forward_uses_running_statistics_and_changes_none(gold):
    model = gpu_model(gold, 0.2)
    x1, x2 = gpu_views(gold)
    with torch.no_grad():
        train_loss = float(model(x1, x2, float(gold['m'])))                         # moves the running statistics off their initial values
    model.eval()
    before = {n: b.detach().clone() for n, b in model.named_buffers()}
    loss = model(x1, x2, 1.0)                                                       # gradients enabled, none needed (m = 1: no update)
    assert loss.dim() == 0 and loss.grad_fn is None and bool(torch.isfinite(loss)) and np.isfinite(train_loss)
    for n, b in model.named_buffers():
        assert torch.equal(b, before[n]), n
    assert torch.equal(model(x1, x2, 1.0), loss)
    model.base_encoder.layer3[0].bn2.running_var.mul_(4.0)                          # the result does depend on the running statistics
    assert not torch.equal(model(x1, x2, 1.0), loss)
