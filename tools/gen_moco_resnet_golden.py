"""Writes tests/golden/moco_resnet.npz: what the REFERENCE's own MoCo v3 baseline computes with its default backbone
(other_baselines/mocov3: ``MoCo_ResNet`` over ``resent3d_base.generate_model``, LARS) on a micro configuration (build container only:
needs the reference checkout, see oracle/_refharness.py; the ``.cuda()`` of its ``contrastive_loss`` is neutralised, everything runs on
the CPU).

    python tools/gen_moco_resnet_golden.py [--out other.npz] [--seed N]

Configuration: ``MoCo_ResNet(partial(generate_model, model_depth=10, n_input_channels=1, widen_factor=0.0625), dim=16, mlp_dim=64, T)``
— widths 4 / 8 / 16 / 32, 123,976 parameters in both encoders and the predictor, 171 state-dict entries — on two views of 16 x 1 x 32^3,
m = 0.99, three ``LARS(lr=0.3, weight_decay=1e-6, momentum=0.9)`` steps on the same views, T = 1.0 and T = 0.2.  The initial parameters
are the reference's own initialisation, untouched.  16 samples per view: with fewer rows the last BatchNorms make the reference's own
bf16 run lose most of a gradient, and at 4 per view even its fp32 run forks from the float64 one.

The views are NOT stored (4 MiB).  Generator and tests build them from the frozen legacy stream:
``rs = numpy.random.RandomState(seed); x1 = rs.standard_normal(shape); x2 = x1 + 0.3 * rs.standard_normal(shape)``, cast to fp32.

    seed, config (per view, channels, volume, steps), dims (dim, mlp_dim), m, lars, temps
    view_sum (exactly rounded float64 sums of x1, x2: math.fsum), view_index, view_samples [2, 16]       what the tests assert before they use their views
    names, shapes                      all state-dict keys of the model, in order, and their shapes
    init/<name>                        initial state of the base encoder and the predictor (the momentum encoder starts as a copy)
    T<t>/losses64, losses32, losses16  the losses of the 3 steps in float64, fp32 and under torch.autocast('cpu', bfloat16)
    T<t>/grad64/<name>                 step-1 gradients of the float64 run (stored as fp32)
    T<t>/gap32/<name>, gap16/<name>    relative L2 distance of the fp32 / autocast run's step-1 gradient from the float64 one
    T<t>/stat64/<key>, stat16/<key>    every BatchNorm running statistic after step 1 (float64 run stored as fp32; autocast run)

The generator picks the first seed from ``--seed`` upwards whose three autocast loss gaps are within MIN_GAP_RATIO of each other at both
temperatures and whose fp32 gradients are all within MAX_GAP32 of the float64 ones (a run that happens to cross the float64 trajectory at one step would make a degenerate yardstick for the tests, which
hold each step to 2 x the reference's own gap of that step) and asserts it; a criterion on the reference's own runs alone.
"""
import argparse
import math
import os
import sys
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import _refharness as H          # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'moco_resnet.npz')
ENC = dict(model_depth=10, n_input_channels=1, widen_factor=0.0625)
DIM, MLP_DIM, B, VOLUME, M, STEPS = 16, 64, 16, 32, 0.99, 3
LARS = dict(lr=0.3, weight_decay=1e-6, momentum=0.9)
TEMPS = (1.0, 0.2)
INIT_SEED = 11
# the first seed from 1 upwards that meets both criteria below (`--seed 1 --tries 39` prints the figures of the 38 it passes over: their
# loss-gap ratios are 0.002 .. 0.25, most below 0.1; the fp32 criterion alone refuses 3 of them)
INPUT_SEED = 39
MIN_GAP_RATIO = 0.25      # tools/gen_resnet_golden.py's
MAX_GAP32 = 1e-4          # and the reference's fp32 run must be clean: every step-1 gradient this close to the float64 run's
VIEW_SAMPLES = 16


def views(seed):
    """The two views, from the frozen legacy stream; the tests build the same."""
    rs = np.random.RandomState(seed)
    shape = (B, ENC['n_input_channels'], VOLUME, VOLUME, VOLUME)
    x1 = rs.standard_normal(shape)
    x2 = x1 + 0.3 * rs.standard_normal(shape)
    return x1.astype(np.float32), x2.astype(np.float32)


def view_index(numel):
    return np.linspace(0, numel - 1, VIEW_SAMPLES).astype(np.int64)


def _import_reference():
    H.import_reference()
    sys.path.insert(0, H.REFERENCE_ROOT)
    sys.dont_write_bytecode = True
    try:
        import other_baselines.mocov3.moco.builder as builder
        import other_baselines.mocov3.moco.optimizer as optimizer
        import other_baselines.mocov3.moco.resent3d_base as resnet
    finally:
        sys.path.remove(H.REFERENCE_ROOT)
    for mod in (builder, optimizer, resnet):
        assert os.path.abspath(mod.__file__).startswith(os.path.abspath(H.REFERENCE_ROOT)), mod.__file__
    return builder, optimizer, resnet


def _model(builder, resnet, T, init=None, dtype=torch.float32):
    model = builder.MoCo_ResNet(partial(resnet.generate_model, **ENC), DIM, MLP_DIM, T)
    if init is not None:
        sd = model.state_dict()
        for n, v in init.items():
            sd[n] = v.clone()
            if n.startswith('base_encoder.'):
                sd['momentum_encoder.' + n[len('base_encoder.'):]] = v.clone()
        model.load_state_dict(sd)
    return model.to(dtype).train()


def _run(builder, optimizer, resnet, T, init, x1, x2, mode):
    """mode: 'f64' | 'f32' | 'bf16' -> dict(losses, grads, stats)"""
    dtype = torch.float64 if mode == 'f64' else torch.float32
    model = _model(builder, resnet, T, init, dtype)
    opt = optimizer.LARS(model.parameters(), LARS['lr'], weight_decay=LARS['weight_decay'], momentum=LARS['momentum'])
    x1, x2 = x1.to(dtype), x2.to(dtype)
    r = {'losses': []}
    for step in range(STEPS):
        opt.zero_grad()
        with torch.autocast('cpu', dtype=torch.bfloat16, enabled=mode == 'bf16'):
            loss = model(x1, x2, M)
        loss.backward()
        r['losses'].append(float(loss.detach()))
        if step == 0:
            r['grads'] = {n: p.grad.detach().double().clone() for n, p in model.named_parameters() if p.grad is not None}
            r['stats'] = {n: b.detach().clone() for n, b in model.named_buffers()}
        opt.step()
    return r


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def generate(seed, init, ref):
    """-> (the fixture's entries for this seed, the worse of the two temperatures' loss-gap ratios, the worst fp32 gradient gap)"""
    x1, x2 = views(seed)
    idx = view_index(x1.size)
    out = {'seed': np.int64(seed), 'view_sum': np.array([math.fsum(x1.reshape(-1).tolist()), math.fsum(x2.reshape(-1).tolist())]), 'view_index': idx,
           'view_samples': np.stack([x1.reshape(-1)[idx], x2.reshape(-1)[idx]])}
    t1, t2 = torch.from_numpy(x1), torch.from_numpy(x2)
    ratio, worst32 = 1.0, 0.0
    for T in TEMPS:
        tag = f'T{T}'
        runs = {mode: _run(*ref, T, init, t1, t2, mode) for mode in ('f64', 'f32', 'bf16')}
        for k, mode in (('64', 'f64'), ('32', 'f32'), ('16', 'bf16')):
            out[f'{tag}/losses{k}'] = np.array(runs[mode]['losses'], dtype=np.float64)
        gaps = np.abs(out[f'{tag}/losses16'] - out[f'{tag}/losses64'])
        ratio = min(ratio, float(gaps.min() / gaps.max()))
        g32, g16 = [], []
        for n, g64 in runs['f64']['grads'].items():
            assert float(g64.norm()) > 0, n
            out[f'{tag}/grad64/{n}'] = g64.float().numpy()
            out[f'{tag}/gap32/{n}'] = np.float64(_rel(runs['f32']['grads'][n], g64))
            out[f'{tag}/gap16/{n}'] = np.float64(_rel(runs['bf16']['grads'][n], g64))
            g32.append(out[f'{tag}/gap32/{n}']); g16.append(out[f'{tag}/gap16/{n}'])
        for n, v in runs['f64']['stats'].items():
            kind = np.int64 if 'num_batches' in n else np.float32
            out[f'{tag}/stat64/{n}'] = v.numpy().astype(kind)
            out[f'{tag}/stat16/{n}'] = runs['bf16']['stats'][n].numpy().astype(kind)
        print(f'seed {seed} {tag}: losses64 {out[tag + "/losses64"]} loss gaps32 {np.abs(out[tag + "/losses32"] - out[tag + "/losses64"])} '
              f'gaps16 {gaps} (ratio {gaps.min() / gaps.max():.3g}); gradient gap32 max {max(g32):.3g}, gap16 {min(g16):.3g} .. {max(g16):.3g}')
        worst32 = max(worst32, float(max(g32)))
    return out, ratio, worst32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=OUT)
    ap.add_argument('--seed', type=int, default=INPUT_SEED, help='the first seed tried')
    ap.add_argument('--tries', type=int, default=1, help='how many seeds upwards are tried (a search; the default run asserts INPUT_SEED)')
    a = ap.parse_args()
    torch.set_num_threads(1)      # one summation order whatever the machine's core count: the fixture regenerates byte for byte
    ref = _import_reference()
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *args, **kw: self          # contrastive_loss: labels = arange(N).cuda()
    try:
        torch.manual_seed(INIT_SEED)
        first = _model(ref[0], ref[2], 1.0)
        sd = first.state_dict()
        init = {n: v.detach().clone() for n, v in sd.items() if not n.startswith('momentum_encoder.')}
        assert len(sd) == 171 and sum(p.numel() for p in first.parameters()) == 123976
        for seed in range(a.seed, a.seed + a.tries):
            out, ratio, worst32 = generate(seed, init, ref)
            if ratio >= MIN_GAP_RATIO and worst32 <= MAX_GAP32:
                break
            print(f'seed {seed}: refused (autocast loss-gap ratio {ratio:.3g}, wanted >= {MIN_GAP_RATIO}; worst fp32 gradient gap {worst32:.3g}, '
                  f'wanted <= {MAX_GAP32}), trying the next', flush=True)
        assert ratio >= MIN_GAP_RATIO, 'degenerate autocast loss gaps: search another seed with --seed N --tries K'
        assert worst32 <= MAX_GAP32, 'the fp32 run of this seed is not clean: search another seed with --seed N --tries K'
    finally:
        torch.Tensor.cuda = real_cuda
    out.update(names=np.array(list(sd.keys())), shapes=np.array([','.join(str(s) for s in v.shape) for v in sd.values()]),
               config=np.array([B, ENC['n_input_channels'], VOLUME, STEPS], dtype=np.int64), dims=np.array([DIM, MLP_DIM], dtype=np.int64),
               m=np.float64(M), lars=np.array([LARS['lr'], LARS['weight_decay'], LARS['momentum']]), temps=np.array(TEMPS),
               widen_factor=np.float64(ENC['widen_factor']))
    for n, v in init.items():
        out[f'init/{n}'] = v.numpy()
    np.savez_compressed(a.out, **out)
    size = os.path.getsize(a.out)
    print(f'wrote {a.out}: seed {int(out["seed"])}, {size} bytes')
    assert size < 1 << 20, 'the fixture must stay under the committed-file limit'


if __name__ == '__main__':
    main()
