"""Writes tests/golden/resnet3d_x3.npz and tests/golden/moco_resnet_x3.npz: how far a float64 EMULATION of the fp32x3 route sits from
the float64 run, over the REFERENCE's own models and the inputs of resnet3d.npz / moco_resnet.npz (build container only: needs the
reference checkout, see oracle/_refharness.py; everything runs on the CPU, nothing of the reference is copied).

    python tools/gen_resnet_x3_golden.py [--only resnet|moco]

The emulation is the reference's float64 run with ``torch.nn.functional.conv3d`` and ``linear`` replaced by an autograd function that
forms every product as the route does: both operands split into bf16 halves, ``hi = bf16(v)``, ``lo = bf16(v - hi)``, the product as
``hi.hi + hi.lo + lo.hi`` — forward, input gradient (dy split against the weight) and weight gradient (dy split against the input).
Everything else (sums, BatchNorm, pooling, loss, optimiser) stays float64, so the figures isolate what the split drops.  ``run()`` of
tools/gen_resnet_golden.py and ``_run()`` of tools/gen_moco_resnet_golden.py produce all three runs (float64, emulation, fp32).

resnet3d_x3.npz (data only, a few KiB); "gapx3" is the emulation's distance from the float64 run, "gap32" that of the reference's
own fp32 run:
    grad_names, stat_names                  the parameters / the running statistics (without num_batches_tracked), in order
    gapx3/grad [grad_names]                 relative L2 per step-1 gradient (gap32/<name> of the gradients is in resnet3d.npz)
    gapx3/stat, gap32/stat [stat_names]     max |s - s64| per running statistic after step 1
    gapx3/loss, gap32/loss [3]              |loss - loss64| of the three Adam steps
    gapx3/logits, gapx3/eval, gap32/...     relative L2 of the step-1 train logits and of the eval logits of the initial state
moco_resnet_x3.npz: the same entries (no logits) under ``T<t>/`` for both temperatures, over the three LARS steps.

The generator asserts that its float64 run reproduces the losses of the existing fixtures, i.e. that it runs their configuration.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_moco_resnet_golden as GM          # noqa: E402
import gen_resnet_golden as GR               # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
F64 = torch.float64


def split(t):
    """float64 -> (hi, lo) as float64: the two bf16 halves the kernels form from the fp32 value"""
    hi = t.float().bfloat16().double()
    lo = (t - hi).float().bfloat16().double()
    return hi, lo


def three(op, a, b):
    """op over the split operands: hi.hi + hi.lo + lo.hi"""
    ah, al = split(a)
    bh, bl = split(b)
    return op(ah, bh) + op(ah, bl) + op(al, bh)


class _ConvX3(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, w, stride, padding, conv):
        ctx.save_for_backward(x, w)
        ctx.stride, ctx.padding = stride, padding
        return three(lambda a, b: conv(a, b, None, stride, padding), x, w)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        s, p = ctx.stride, ctx.padding
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = three(lambda g, b: torch.nn.grad.conv3d_input(x.shape, b, g, s, p), dy, w)
        if ctx.needs_input_grad[1]:
            dw = three(lambda g, a: torch.nn.grad.conv3d_weight(a, w.shape, g, s, p), dy, x)
        return dx, dw, None, None, None


class _LinearX3(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return three(lambda a, b: a @ b.t(), x, w)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dx = three(lambda g, b: g @ b, dy, w) if ctx.needs_input_grad[0] else None
        dw = three(lambda g, a: g.t() @ a, dy, x) if ctx.needs_input_grad[1] else None
        return dx, dw


class emulation:
    """Context: conv3d and linear of torch.nn.functional form three-term split products (float64 operands only)."""

    def __enter__(self):
        F = torch.nn.functional
        self.saved = (F.conv3d, F.linear)
        conv = F.conv3d

        def conv3d(x, w, bias=None, stride=1, padding=0, dilation=1, groups=1):
            assert x.dtype == F64 and bias is None and groups == 1 and set(np.atleast_1d(dilation).tolist()) == {1}
            return _ConvX3.apply(x, w, stride, padding, conv)

        def linear(x, w, bias=None):
            assert x.dtype == F64 and x.dim() == 2
            y = _LinearX3.apply(x, w)
            return y if bias is None else y + bias

        F.conv3d, F.linear = conv3d, linear
        return self

    def __exit__(self, *exc):
        torch.nn.functional.conv3d, torch.nn.functional.linear = self.saved


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def maxabs(a, b):
    return float((torch.as_tensor(a).double() - torch.as_tensor(b).double()).abs().max())


def gaps(tag, r64, r32, rx3):
    """-> the entries of one configuration: per run (gapx3 = the emulation, gap32 = the reference's fp32 run) its distance from r64;
    and the fp32 run's gradient gaps, which the existing fixtures hold already"""
    grads = list(r64['grads'])
    stats = [k for k in r64['stats'] if 'num_batches' not in k]
    out = {tag + 'grad_names': np.array(grads), tag + 'stat_names': np.array(stats)}
    for kind, r in (('gapx3/', rx3), ('gap32/', r32)):
        assert all(int(r['stats'][k]) == int(v) for k, v in r64['stats'].items() if 'num_batches' in k)
        g = np.array([rel(r['grads'][n], r64['grads'][n]) for n in grads])
        if kind == 'gapx3/':
            out[tag + 'gapx3/grad'] = g
        else:
            g32 = g
        out[tag + kind + 'stat'] = np.array([maxabs(r['stats'][k], r64['stats'][k]) for k in stats])
        out[tag + kind + 'loss'] = np.abs(np.array(r['losses']) - np.array(r64['losses']))
        for k in ('logits', 'eval'):
            if k in r64:
                out[tag + kind + k] = np.float64(rel(r[k], r64[k]))
    g, s = out[tag + 'gapx3/grad'], out[tag + 'gapx3/stat']
    print(f'{tag or "resnet"}: gradient gapx3 {g.min():.3g} .. {g.max():.3g} (worst {grads[int(g.argmax())]}), gap32 at most '
          f'{g32.max():.3g}; statistics gapx3 at most {s.max():.3g}, gap32 {out[tag + "gap32/stat"].max():.3g}; losses gapx3 '
          f'{out[tag + "gapx3/loss"]}, gap32 {out[tag + "gap32/loss"]}')
    for k in ('logits', 'eval'):
        if k in r64:
            print(f'    {k}: gapx3 {out[tag + "gapx3/" + k]:.3g}, gap32 {out[tag + "gap32/" + k]:.3g}')
    return out, g32


def write(path, out):
    np.savez_compressed(path, **out)
    print(f'wrote {path}: {os.path.getsize(path)} bytes')
    assert os.path.getsize(path) < 16 << 10


def resnet():
    z = np.load(os.path.join(GOLD, 'resnet3d.npz'), allow_pickle=False)
    ref = GR.reference_resnet()
    keys = [str(n) for n in z['names']] + [str(n) for n in z['buffer_names']]
    sd = {k: torch.from_numpy(z['init/' + k]) for k in keys}
    x, labels = torch.from_numpy(z['x']).float(), torch.from_numpy(z['labels']).long()
    r64 = GR.run(ref, sd, x, labels, 'f64')
    r32 = GR.run(ref, sd, x, labels, 'f32')
    with emulation():
        rx3 = GR.run(ref, sd, x, labels, 'f64')
    assert np.allclose(r64['losses'], z['loss64'], rtol=1e-9, atol=0), 'this is not the configuration of resnet3d.npz'
    out, g32 = gaps('', r64, r32, rx3)
    for n, g in zip(out['grad_names'], g32):           # the fp32 run is resnet3d.npz's (up to the summation order of this machine)
        assert abs(g - float(z['gap32/' + str(n)])) <= 0.25 * float(z['gap32/' + str(n)]), n
    write(os.path.join(GOLD, 'resnet3d_x3.npz'), out)


def moco():
    z = np.load(os.path.join(GOLD, 'moco_resnet.npz'), allow_pickle=False)
    torch.set_num_threads(1)      # as the generator of moco_resnet.npz: one summation order
    ref = GM._import_reference()
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *args, **kw: self          # contrastive_loss: labels = arange(N).cuda()
    try:
        init = {k[len('init/'):]: torch.from_numpy(z[k]) for k in z.files if k.startswith('init/')}
        x1, x2 = (torch.from_numpy(v) for v in GM.views(int(z['seed'])))
        out = {}
        for T in GM.TEMPS:
            r64 = GM._run(*ref, T, init, x1, x2, 'f64')
            r32 = GM._run(*ref, T, init, x1, x2, 'f32')
            with emulation():
                rx3 = GM._run(*ref, T, init, x1, x2, 'f64')
            assert np.allclose(r64['losses'], z[f'T{T}/losses64'], rtol=1e-9, atol=0), 'this is not the configuration of moco_resnet.npz'
            out.update(gaps(f'T{T}/', r64, r32, rx3)[0])
    finally:
        torch.Tensor.cuda = real_cuda
    write(os.path.join(GOLD, 'moco_resnet_x3.npz'), out)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', choices=('resnet', 'moco'))
    a = ap.parse_args()
    if a.only != 'moco':
        resnet()
    if a.only != 'resnet':
        moco()
