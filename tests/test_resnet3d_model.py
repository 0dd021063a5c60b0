"""The 3-D ResNet baseline (k_fold_training_scripts.resnet_3d / train_3d_resnet) against tests/golden/resnet3d.npz, which
tools/gen_resnet_golden.py wrote from the reference's own ``generate_model(10, n_classes=2, n_input_channels=1, widen_factor=0.0625)``
on a 4 x 1 x 32^3 input (float64, fp32 and torch.autocast('cpu', bfloat16) runs of the same three Adam steps).

Rule of the GPU comparisons (the one the fine-tuning and MoCo v3 routes are held to): this package's bf16 route may be as far from
the reference's float64 run as TWICE what the reference itself loses under bf16 autocast — relative L2 per tensor for the logits and
every parameter gradient, absolute per step for the three losses.  At this size the autocast run loses 0.8 - 63 % on the gradients
(ReLU and max-pool decisions flip, the last BatchNorms see 8 rows), so this is a gross-error check: correctness rests on the layer
tests of tests/test_resnet3d_kernels.py.  No tight whole-model bf16 comparison exists on purpose: bf16 rounding boundaries flip.

Observed on the MI355X: logits at 0.85 of the autocast gap, the 39 gradients at 0.07 - 0.97 of theirs, the three Adam-step losses at
1.09 / 0.64 / 0.21, the eval logits at 0.84 (allowed: 2).  A CPU statement of the route's rounding points (conv / fc operands and their dy
rounded to bf16, everything else fp32, torch's own ops) reproduces the GPU's figures to three digits.

Running statistics: |s - s64| <= RUN_TOL max|s64| per tensor with RUN_TOL = 10 x 2^-9 — a bf16 rounding is 2^-9 relative, and the
longest chain of bf16-rounded activations in front of a BatchNorm of ResNet-10 has 10 links (input, pooled stem, two per block).
"""
import os
import sys

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'resnet3d.npz')
RUN_TOL = 10 * 2.0 ** -9
KW = dict(n_classes=2, n_input_channels=1, widen_factor=0.0625)


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD, allow_pickle=False)


def make_model(**kw):
    from vit_ae_plus_plus_amd.k_fold_training_scripts.resnet_3d import generate_model
    return generate_model(10, **dict(KW, **kw))


def init_state(z):
    keys = [str(n) for n in z['names']] + [str(n) for n in z['buffer_names']]
    return {k: torch.from_numpy(z['init/' + k]) for k in keys}


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ---------------------------------------------------------------------------- CPU
def test_fixture_is_small_and_complete(gold):
    assert os.path.getsize(GOLD) < 1 << 20
    assert sum(int(np.prod(gold['init/' + str(n)].shape)) for n in gold['names']) == 57766
    assert gold['x'].shape == (4, 1, 32, 32, 32) and list(gold['class_weight']) == [3.0, 1.0]
    for k in ('logits64', 'logits32', 'logits16', 'loss64', 'loss32', 'loss16', 'eval64', 'eval32', 'eval16'):
        assert k in gold.files
    assert all(f'grad64/{n}' in gold.files and f'gap16/{n}' in gold.files for n in gold['names'])


def test_state_dict_keys_and_shapes_are_the_references(gold):
    m = make_model()
    assert [n for n, _ in m.named_parameters()] == [str(n) for n in gold['names']]
    assert [str(tuple(p.shape)) for _, p in m.named_parameters()] == [str(s) for s in gold['shapes']]
    assert [n for n, _ in m.named_buffers()] == [str(n) for n in gold['buffer_names']]
    sd = m.state_dict()
    for k in ('conv1.weight', 'bn1.running_var', 'layer1.0.conv1.weight', 'layer2.0.downsample.0.weight', 'layer2.0.downsample.1.bias',
              'layer4.0.bn2.num_batches_tracked', 'fc.weight', 'fc.bias'):
        assert k in sd
    assert 'layer1.0.downsample.0.weight' not in sd                              # stride 1, same width: identity shortcut
    assert all(isinstance(p, torch.nn.Parameter) and p.dtype == torch.float32 for p in m.parameters())


def test_state_dict_loads_both_ways(gold):
    m, init = make_model(), init_state(gold)
    m.load_state_dict(init, strict=True)
    out = m.state_dict()
    assert list(out.keys()) == list(make_model().state_dict().keys())
    for k, v in init.items():
        assert torch.equal(out[k], v), k
    m2 = make_model()
    m2.load_state_dict(out, strict=True)
    assert all(torch.equal(a, b) for a, b in zip(m2.state_dict().values(), out.values()))


def test_init_statistics():
    torch.manual_seed(0)
    from vit_ae_plus_plus_amd.k_fold_training_scripts.resnet_3d import generate_model, get_inplanes
    assert get_inplanes() == [64, 128, 256, 512]
    m = generate_model(18, n_classes=2, n_input_channels=4, widen_factor=0.25)
    assert [len(getattr(m, f'layer{i}')) for i in (1, 2, 3, 4)] == [2, 2, 2, 2]
    assert m.conv1.weight.shape == (16, 4, 7, 7, 7) and m.conv1.stride == (1, 2, 2) and m.conv1.padding == (3, 3, 3)
    for name, mod in m.named_modules():
        if isinstance(mod, torch.nn.Conv3d):
            fan_out = mod.out_channels * int(np.prod(mod.kernel_size))
            want = (2.0 / fan_out) ** 0.5                                        # Kaiming normal, fan_out, ReLU gain
            w, n = mod.weight.detach(), mod.weight.numel()
            assert abs(float(w.std()) / want - 1) < 4 / n ** 0.5 + 0.02, name
            assert abs(float(w.mean())) < 5 * want / n ** 0.5, name
            assert mod.bias is None
        elif isinstance(mod, torch.nn.BatchNorm3d):
            assert bool((mod.weight == 1).all()) and bool((mod.bias == 0).all()), name
    assert [len(getattr(generate_model(34), f'layer{i}')) for i in (1, 2, 3, 4)] == [3, 4, 6, 3]
    t2 = generate_model(10, conv1_t_size=3, conv1_t_stride=2, no_max_pool=True)
    assert t2.conv1.kernel_size == (3, 7, 7) and t2.conv1.stride == (2, 2, 2) and t2.conv1.padding == (1, 3, 3) and t2.no_max_pool


def test_refusals_at_construction():
    from vit_ae_plus_plus_amd.k_fold_training_scripts import resnet_3d as R
    for depth in (50, 101, 152, 200):
        with pytest.raises(NotImplementedError):
            R.generate_model(depth)
    with pytest.raises(AssertionError):
        R.generate_model(11)
    with pytest.raises(NotImplementedError):
        R.generate_model(10, shortcut_type='A')
    with pytest.raises(NotImplementedError):
        R.ResNet(R.Bottleneck, [3, 4, 6, 3], R.get_inplanes())
    with pytest.raises(NotImplementedError):
        R.generate_model(10, widen_factor=0.05)                                  # widths 3 / 6 / 12 / 25


def test_dropin_exposes_the_baseline():
    from vit_ae_plus_plus_amd import dropin
    saved = {k: sys.modules.get(k) for k in dropin._ALIASES}
    try:
        dropin.install(force=True)
        import k_fold_training_scripts.resnet_3d as r
        import k_fold_training_scripts.train_3d_resnet as t
        from k_fold_training_scripts.train_3d_resnet import get_all_feat_and_labels
        import vit_ae_plus_plus_amd.k_fold_training_scripts.resnet_3d as r2
        assert r is r2 and callable(r.generate_model) and callable(t.train_one_epoch) and callable(t.evaluate)
        import argparse
        data = [(torch.full((1, 2, 2, 2), float(i)), None, torch.tensor(i % 2)) for i in range(3)]
        f, l = get_all_feat_and_labels(data, argparse.Namespace(in_channels=1))
        assert f.shape == (3, 2, 2, 2) and l.tolist() == [0, 1, 0]
        data4 = [(torch.zeros(4, 2, 2, 2), None, torch.tensor(1))] * 2
        assert get_all_feat_and_labels(data4, argparse.Namespace(in_channels=4))[0].shape == (2, 4, 2, 2, 2)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_cpu_input_raises():
    from vit_ae_plus_plus_amd._abi import VitaeError
    m = make_model()
    x = torch.zeros(1, 1, 16, 16, 16)
    with pytest.raises(VitaeError, match='no CPU fallback'):
        m.train()(x)
    with pytest.raises(VitaeError, match='no CPU fallback'):
        m.eval()(x)
    for sub in (m.conv1, m.bn1, m.maxpool, m.layer1[0]):                         # the layers hold parameters; they do not compute
        with pytest.raises(VitaeError):
            sub(x)


# ---------------------------------------------------------------------------- GPU
def gpu_model(z):
    m = make_model()
    m.load_state_dict(init_state(z))
    return m.cuda()


def batch(z):
    return torch.from_numpy(z['x']).float().cuda(), torch.from_numpy(z['labels']).long().cuda()


def criterion(z):
    return torch.nn.CrossEntropyLoss(weight=torch.from_numpy(z['class_weight']).cuda())


def one_step(z, m=None):
    m = gpu_model(z).train() if m is None else m
    x, y = batch(z)
    logits = m(x)
    loss = criterion(z)(logits, y)
    loss.backward()
    torch.cuda.synchronize()
    return m, logits.detach(), loss.detach()


@pytest.mark.gpu
def test_train_step_within_twice_the_references_autocast_gap(gold):
    m, logits, loss = one_step(gold)
    gap = rel_l2(gold['logits16'], gold['logits64'])
    e = rel_l2(logits, gold['logits64'])
    print(f'RATIO resnet logits: e={e:.3e} gap16={gap:.3e} ratio={e / gap:.2f}')
    assert logits.shape == (4, 2) and logits.dtype == torch.float32
    assert e <= 2 * gap
    worst, outside = 0.0, []
    for n, p in m.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, n
        e, gap = rel_l2(p.grad, gold['grad64/' + n]), float(gold['gap16/' + n])
        worst = max(worst, e / gap)
        print(f'RATIO resnet grad {n}: e={e:.3e} gap16={gap:.3e} ratio={e / gap:.2f}')
        if not e <= 2 * gap:
            outside.append((n, e, gap))
    print(f'RATIO resnet worst gradient ratio {worst:.2f} of the allowed 2')
    # running statistics after the step
    for k in gold['buffer_names']:
        k = str(k)
        got, ref = m.state_dict()[k].cpu(), torch.from_numpy(gold['stat64/' + k])
        if k.endswith('num_batches_tracked'):
            assert int(got) == int(ref) == 1, k
            continue
        e = float((got.double() - ref.double()).abs().max() / ref.double().abs().max())
        print(f'RATIO resnet stat {k}: e={e:.3e} of {RUN_TOL:.3e}')
        if not e <= RUN_TOL:
            outside.append((k, e, RUN_TOL))
    assert not outside, outside


@pytest.mark.gpu
def test_three_adam_steps(gold):
    m = gpu_model(gold).train()
    x, y = batch(gold)
    crit = criterion(gold)
    opt = torch.optim.Adam(m.parameters(), lr=float(gold['lr']))
    for t in range(3):
        opt.zero_grad()
        loss = crit(m(x), y)
        loss.backward()
        opt.step()
        loss = float(loss.detach())
        e, gap = abs(loss - float(gold['loss64'][t])), abs(float(gold['loss16'][t]) - float(gold['loss64'][t]))
        print(f'RATIO resnet adam step {t}: loss={loss:.6f} ref64={float(gold["loss64"][t]):.6f} e={e:.3e} gap16={gap:.3e} ratio={e / gap:.2f}')
        assert e <= 2 * gap, (t, loss, e, gap)


@pytest.mark.gpu
def test_eval_logits(gold):
    m = gpu_model(gold).eval()
    x, _ = batch(gold)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    out = m(x)
    assert not out.requires_grad
    e, gap = rel_l2(out, gold['eval64']), rel_l2(gold['eval16'], gold['eval64'])
    print(f'RATIO resnet eval logits: e={e:.3e} gap16={gap:.3e} ratio={e / gap:.2f}')
    assert e <= 2 * gap
    with torch.no_grad():                                            # train() under no_grad is inference too
        assert torch.equal(m.train()(x), out)
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())     # nothing was updated


@pytest.mark.gpu
def test_forward_and_gradients_repeat_bit_for_bit(gold):
    m = gpu_model(gold).train()
    x, _ = batch(gold)
    a, b = m(x).detach(), m(x).detach()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    m1, l1, _ = one_step(gold)
    m2, l2, _ = one_step(gold)
    assert torch.equal(l1.view(torch.int32), l2.view(torch.int32))
    for (n, p), q in zip(m1.named_parameters(), m2.parameters()):
        assert torch.equal(p.grad.view(torch.int32), q.grad.view(torch.int32)), n


@pytest.mark.gpu
def test_accumulation_equals_the_sum_of_two_backward_passes(gold):
    x, y = batch(gold)
    xb, yb = x.flip(0).contiguous(), y.flip(0).contiguous()
    crit = criterion(gold)

    def grads(batches):
        m = gpu_model(gold).train()
        for xx, yy in batches:
            (crit(m(xx), yy) / 2).backward()
        return [p.grad.clone() for p in m.parameters()]

    ga, gb, both = grads([(x, y)]), grads([(xb, yb)]), grads([(x, y), (xb, yb)])
    for a, b, s in zip(ga, gb, both):
        assert torch.equal((a + b).view(torch.int32), s.view(torch.int32))


@pytest.mark.gpu
def test_second_backward_raises(gold):
    from vit_ae_plus_plus_amd._abi import VitaeError
    m = gpu_model(gold).train()
    x, y = batch(gold)
    loss = criterion(gold)(m(x), y)
    loss.backward(retain_graph=True)
    with pytest.raises(VitaeError, match='backward called twice'):
        loss.backward()


@pytest.mark.gpu
def test_evaluate_keys_and_full_size_channels(gold):
    """train_3d_resnet.evaluate over two batches, and one training step of an un-narrowed 4-channel ResNet-10 on a small volume
    (Cin = 4 stem, widths 64 .. 512, conv1_t_stride = 2)."""
    import argparse
    from vit_ae_plus_plus_amd.k_fold_training_scripts.train_3d_resnet import evaluate
    from vit_ae_plus_plus_amd.k_fold_training_scripts.resnet_3d import generate_model
    m = gpu_model(gold)
    x, y = batch(gold)
    stats = evaluate([(x[:2].cpu(), None, y[:2].cpu()), (x[2:].cpu(), None, y[2:].cpu())], m, torch.device('cuda'), argparse.Namespace())
    assert set(stats) == {'loss', 'roc_score', 'spec', 'sens'} and np.isfinite(stats['loss']) and 0 <= stats['roc_score'] <= 1
    logits = m.eval()(x)
    want = np.mean([float(torch.nn.functional.cross_entropy(logits[i:i + 2], y[i:i + 2])) for i in (0, 2)])
    assert abs(stats['loss'] - want) < 1e-5 * max(1.0, abs(want))
    torch.manual_seed(0)
    big = generate_model(10, n_classes=2, n_input_channels=4, conv1_t_stride=2).cuda().train()
    out = big(torch.randn(2, 4, 16, 16, 16, device='cuda'))
    out.sum().backward()
    torch.cuda.synchronize()
    assert out.shape == (2, 2) and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in big.parameters())
