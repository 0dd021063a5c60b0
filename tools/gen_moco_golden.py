"""Writes tests/golden/moco_v3.npz: what the REFERENCE's own MoCo v3 baseline (other_baselines/mocov3: MoCo_ViT over its
VisionTransformer3D, LARS) computes on a micro configuration (build container only: needs the reference checkout, see
oracle/_refharness.py; the ``.cuda()`` of its ``contrastive_loss`` is neutralised, everything runs on the CPU).

    python tools/gen_moco_golden.py [--out other.npz]

Configuration: volume 8, patch 4, 1 channel, embed 64, depth 2, 2 heads (head size 32), mlp_dim 64, dim 32, B = 8 per view, m = 0.99,
LARS(lr 0.3, weight_decay 1e-2, momentum 0.9), the same two views for 3 steps.  The initial weights are the reference's own
initialisation with the zero / one vectors (biases, norm weights) perturbed, so that no gradient is trivially zero.

    x1, x2, m, lars, names, shapes            inputs, hyper-parameters, the state-dict keys of the model and their shapes
    null_grads                                parameters whose gradient is zero in exact arithmetic (no gap32 / gap16 entries)
    init/<name>                               initial parameters of the base encoder and the predictor (the momentum encoder starts as a copy)
    T<t>/losses                               fp32 losses of the 3 steps                      (t = 1.0, 0.2)
    T<t>/losses64, T<t>/losses16              the same run in float64 / under torch.autocast('cpu', bfloat16)
    T<t>/grad/<name>                          step-1 gradients (fp32 run), SAMPLED: ``sample_index(numel)`` of the flattened tensor
    T<t>/mom/<name>                           momentum encoder's parameters after step 1, sampled the same way
    T<t>/stat/<key>                           every BatchNorm running_mean / running_var / num_batches_tracked after step 1 (whole)
    T<t>/param3/<name>                        trainable parameters after step 3, sampled
    T<t>/gap32/<name>, T<t>/gap16/<name>      relative L2 distance of the step-1 gradient of the fp32 / bf16 run from the float64 run's,
                                              on the sampled elements
    T<t>/f64/...                              pieces of the float64 run for the tests' own numpy restatement: q1, k2, q2, k1, loss, dq1, dq2
                                              of step 1 and p, g, mu_after, p_after of one LARS step for the tensors in ``f64/lars_names``

The generator ASSERTS that the three bf16 loss gaps of each temperature are within a factor 4 of each other (``INPUT_SEED``) and that
the reference's fp32 gradients are within a third of 1e-4 (relative L2, whole tensor, per parameter) of its
float64 ones: the tests hold this package to 1e-4 against the fp32 fixture.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import _refharness as H          # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'moco_v3.npz')
ENC = dict(volume_size=8, patch_size=4, in_chans=1, embed_dim=64, depth=2, num_heads=2)
MLP_DIM, DIM, B, M = 64, 32, 8, 0.99
LARS = dict(lr=0.3, weight_decay=1e-2, momentum=0.9)
TEMPS = (1.0, 0.2)
STEPS = 3
SAMPLES = 256
# The bf16 tests hold each step's loss to 2 x the reference's own bf16 <-> float64 gap of that step, so a seed whose reference run
# happens to cross the float64 trajectory at one step (seed 13: gaps 1.9e-3, 8.4e-4, 1.9e-2) makes a degenerate yardstick.  Of the
# seeds 13 and 21 .. 31 this one has the most even gaps (smallest / largest of the three, the worse of the two temperatures: 0.28);
# the generator asserts MIN_GAP_RATIO.
INPUT_SEED = 21
MIN_GAP_RATIO = 0.25
# the final LayerNorm's bias shifts every row alike and the projector's first BatchNorm (batch statistics) removes the shift
NULL_GRADS = ('base_encoder.norm.bias',)
F64_LARS_NAMES = ('predictor.0.weight', 'base_encoder.blocks.1.norm2.bias', 'base_encoder.cls_token')


def sample_index(numel: int) -> np.ndarray:
    """The flattened elements of a tensor the fixture keeps: all of a small one, else SAMPLES evenly spaced ones."""
    return np.arange(numel) if numel <= SAMPLES else np.linspace(0, numel - 1, SAMPLES).astype(np.int64)


def _sample(t) -> np.ndarray:
    a = t.detach().cpu().numpy().reshape(-1)
    return a[sample_index(a.size)].copy()


def _import_reference_moco():
    H.import_reference()                      # the timm stubs
    sys.path.insert(0, H.REFERENCE_ROOT)
    try:
        import other_baselines.mocov3.moco.builder as builder
        import other_baselines.mocov3.moco.optimizer as optimizer
        import other_baselines.mocov3.moco.vit_3d as vit_3d
    finally:
        sys.path.remove(H.REFERENCE_ROOT)
    for mod in (builder, optimizer, vit_3d):
        assert os.path.abspath(mod.__file__).startswith(os.path.abspath(H.REFERENCE_ROOT)), mod.__file__
    return builder, optimizer, vit_3d


def _model(builder, vit_3d, T, init=None, dtype=torch.float32):
    from functools import partial
    model = builder.MoCo_ViT(partial(vit_3d.VisionTransformer3D, **ENC), DIM, MLP_DIM, T)
    if init is not None:
        sd = model.state_dict()
        for n, v in init.items():
            sd[n] = v.clone()
            if n.startswith('base_encoder.'):
                sd['momentum_encoder.' + n[len('base_encoder.'):]] = v.clone()
        model.load_state_dict(sd)
    return model.to(dtype).train()


def _initial_weights(builder, vit_3d):
    torch.manual_seed(11)
    model = _model(builder, vit_3d, 1.0)
    g = torch.Generator().manual_seed(12)
    init = {}
    for n, p in model.named_parameters():
        if n.startswith('momentum_encoder.'):
            continue
        v = p.detach().clone()
        if v.ndim <= 1 or n.endswith('cls_token'):      # zeros / ones as initialised: move them
            v = v + 0.05 * torch.randn(v.shape, generator=g)
        init[n] = v
    return init


def _run(builder, optimizer, vit_3d, T, init, x1, x2, dtype=torch.float32, autocast=False):
    model = _model(builder, vit_3d, T, init, dtype)
    opt = optimizer.LARS(model.parameters(), LARS['lr'], weight_decay=LARS['weight_decay'], momentum=LARS['momentum'])
    x1, x2 = x1.to(dtype), x2.to(dtype)
    r = {'losses': []}
    cap = {}
    hook = model.predictor.register_forward_hook(lambda mod, inp, out: cap.setdefault('q', []).append(out))
    hook_k = model.momentum_encoder.register_forward_hook(lambda mod, inp, out: cap.setdefault('k', []).append(out))
    for step in range(STEPS):
        cap.clear()
        opt.zero_grad()
        with torch.autocast('cpu', dtype=torch.bfloat16, enabled=autocast):
            loss = model(x1, x2, M)
        if step == 0:
            q1, q2 = cap['q']
            k1, k2 = cap['k']
            q1.retain_grad(); q2.retain_grad()
        loss.backward()
        r['losses'].append(float(loss.detach()))
        if step == 0:
            r['grads'] = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
            r['mom'] = {n: p.detach().clone() for n, p in model.named_parameters() if n.startswith('momentum_encoder.')}
            r['stats'] = {n: b.detach().clone() for n, b in model.named_buffers()}
            r['qk'] = {'q1': q1.detach().clone(), 'k2': k2.detach().clone(), 'q2': q2.detach().clone(), 'k1': k1.detach().clone(),
                       'dq1': q1.grad.detach().clone(), 'dq2': q2.grad.detach().clone(), 'loss': loss.detach().clone()}
            r['lars'] = {n: {'p': p.detach().clone(), 'g': p.grad.detach().clone()} for n, p in model.named_parameters() if n in F64_LARS_NAMES}
        opt.step()
        if step == 0:
            for n, p in model.named_parameters():
                if n in F64_LARS_NAMES:
                    r['lars'][n]['p_after'] = p.detach().clone()
                    r['lars'][n]['mu_after'] = opt.state[p]['mu'].detach().clone()
    hook.remove(); hook_k.remove()
    r['params'] = {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
    return r, model


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def generate():
    torch.set_num_threads(1)      # one summation order whatever the machine's core count: the fixture regenerates byte for byte
    builder, optimizer, vit_3d = _import_reference_moco()
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self          # contrastive_loss: labels = arange(N).cuda()
    try:
        init = _initial_weights(builder, vit_3d)
        g = torch.Generator().manual_seed(INPUT_SEED)
        x1 = torch.randn(B, ENC['in_chans'], 8, 8, 8, generator=g)
        x2 = x1 + 0.5 * torch.randn(B, ENC['in_chans'], 8, 8, 8, generator=g)
        out = {'x1': x1.numpy(), 'x2': x2.numpy(), 'm': np.array(M), 'lars': np.array([LARS['lr'], LARS['weight_decay'], LARS['momentum']]),
               'temps': np.array(TEMPS), 'null_grads': np.array(NULL_GRADS), 'f64/lars_names': np.array(F64_LARS_NAMES)}
        for n, v in init.items():
            out[f'init/{n}'] = v.numpy()
        for T in TEMPS:
            tag = f'T{T}'
            r32, model = _run(builder, optimizer, vit_3d, T, init, x1, x2)
            r64, _ = _run(builder, optimizer, vit_3d, T, init, x1, x2, dtype=torch.float64)
            r16, _ = _run(builder, optimizer, vit_3d, T, init, x1, x2, autocast=True)
            if 'names' not in out:
                sd = model.state_dict()
                out['names'] = np.array(list(sd.keys()))
                out['shapes'] = np.array([','.join(str(s) for s in v.shape) for v in sd.values()])
            out[f'{tag}/losses'] = np.array(r32['losses'], dtype=np.float64)
            out[f'{tag}/losses64'] = np.array(r64['losses'], dtype=np.float64)
            out[f'{tag}/losses16'] = np.array(r16['losses'], dtype=np.float64)
            loss_gaps = np.abs(out[f'{tag}/losses16'] - out[f'{tag}/losses64']) / out[f'{tag}/losses64']
            assert loss_gaps.min() >= MIN_GAP_RATIO * loss_gaps.max(), f'{tag}: degenerate bf16 loss gaps {loss_gaps}: pick another INPUT_SEED'
            worst = 0.0
            for n, g32 in r32['grads'].items():
                g64 = r64['grads'][n]
                out[f'{tag}/grad/{n}'] = _sample(g32)
                if n in NULL_GRADS:
                    # a shift the next BatchNorm removes: the gradient is zero in exact arithmetic, round-off in any other
                    assert float(g64.norm()) <= 1e-12 * float(r64['grads'][n[:-4] + 'weight'].norm()), n
                    continue
                assert float(g64.norm()) > 0, n
                full = _rel(g32.numpy(), g64.numpy())
                worst = max(worst, full)
                assert full <= 1e-4 / 3, f'{tag} {n}: the reference fp32 gradient is {full:.3g} from its float64 one (bound {1e-4 / 3:.3g})'
                out[f'{tag}/gap32/{n}'] = np.array(_rel(_sample(g32), _sample(g64)))
                out[f'{tag}/gap16/{n}'] = np.array(_rel(_sample(r16['grads'][n].float()), _sample(g64)))
            for n, v in r32['mom'].items():
                out[f'{tag}/mom/{n}'] = _sample(v)
            for n, v in r32['stats'].items():
                out[f'{tag}/stat/{n}'] = v.numpy()
            for n, v in r32['params'].items():
                out[f'{tag}/param3/{n}'] = _sample(v)
            for k, v in r64['qk'].items():
                out[f'{tag}/f64/{k}'] = v.numpy()
            for n, d in r64['lars'].items():
                for k, v in d.items():
                    out[f'{tag}/f64/lars/{n}/{k}'] = v.numpy()
            gaps16 = [float(out[f'{tag}/gap16/{n}']) for n in r32['grads'] if n not in NULL_GRADS]
            print(tag, 'losses', r32['losses'], 'f64', r64['losses'], 'bf16', r16['losses'])
            print(tag, 'worst fp32 gradient gap %.3g' % worst, 'bf16 gaps %.3g..%.3g' % (min(gaps16), max(gaps16)),
                  'min |grad| %.3g' % min(float(v.norm()) for v in r32['grads'].values()))
    finally:
        torch.Tensor.cuda = real_cuda
    return out


def main():
    path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else OUT
    out = generate()
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < (1 << 20), 'the fixture must stay under the committed-file limit'


if __name__ == '__main__':
    main()
