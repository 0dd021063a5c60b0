"""MoCo v3 pre-training step of ViT-B/16 on 96^3 x 4ch (mlp_dim 4096, dim 256) on the MI355X, through the reference's loop
(autocast, GradScaler: scale -> backward -> step(optimizer) -> update), LARS(lr 0.3, weight_decay 1e-6, momentum 0.9).

    python tools/moco_bench.py [batch=4,16] [routes=bf16,act16] [reps=9] [inner=5] [depth=12]

Two variants of the SAME step alternate in one process (A, B, A, B, ...; the median of ``reps`` windows of ``inner`` steps each, every
window between two device synchronisations):
  kernels   vitae_ema_multi (1 launch) + vitae_lars_multi (2 launches) + vitae_moco_loss (3 launches)
  torch     the same model with the momentum update and LARS restated here as the per-tensor torch statements a plain port would
            run (``torch_ema`` / ``TorchLARS`` below: two products and a sum per parameter pair; decay, two norms, the trust
            ratio, momentum and the step per parameter); loss, encoder and MLPs are the package's in both.  (The parent commit has no MoCo
            to compare with.)
Then the three launch groups alone on the tensors of that step, with achieved bytes / s from the bytes the algorithm has to move:
EMA 12 B per parameter (read pm, pb; write pm), LARS 8 B (norm pass: p, g) + 20 B (update pass: p, g, mu read; p, mu written) per
parameter of a scaled tensor, 20 B of an unscaled one; the loss 4 N C * 4 B in + 2 N C * 4 B out.  ``vitae_adamw_multi`` reaches
4.6 TB/s on the fine-tuning model (LABNOTES.md) — the yardstick for the two streaming groups.

    python tools/moco_bench.py shadow=0,1 [batch=4,16] [routes=act16] [reps=9] [inner=5] [depth=12]

``shadow=0,1``: the bf16 weight shadows (``VITAE_WEIGHT_SHADOW``) off against on instead of kernels against torch statements: two
kernel models, one always stepped with the switch at 0 and one with it at 1 (so the slots of the first are never current and those of
the second always), in the same alternating windows; then the EMA and LARS launch groups alone, off (12 B; 8 + 20 B per parameter)
against on (14 B; 8 + 22 B for the weights that have a slot: the GEMM weights of the encoders).

    python tools/moco_bench.py arch=resnet [batch=4,16] [reps=9] [inner=5]

``arch=resnet``: ``MoCo_ResNet`` over ResNet-10 on 96^3 x 4 channels (mlp_dim 4096, dim 256), the script's default ``--arch``, through
the same loop.  Two tables, each of two models alternating in this process: kernels against the torch statements (as above), and the
convolution operand store (``resnet.ConvPackStore``, one ``vitae_conv3d_pack_weights_multi`` launch per encoder and step) against a pack
per convolution call (``VITAE_CONV_PACK_STORE=0``).

    python tools/moco_bench.py arch=resnet precision=bf16,fp32x3 [batch=4,16] [reps=5] [inner=1]

``precision=``: one ``MoCo_ResNet`` per listed precision of the encoders instead, the same step, alternating windows after 2 warm-ups.
"""
import os
import statistics
import sys
import time
from functools import partial

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from vit_ae_plus_plus_amd.model.vit import VisionTransformer3D                                      # noqa: E402
from vit_ae_plus_plus_amd.other_baselines.mocov3.moco.builder import MoCo_ResNet, MoCo_ViT           # noqa: E402
from vit_ae_plus_plus_amd.other_baselines.mocov3.moco.optimizer import LARS                          # noqa: E402

ROUTES = {'bf16': dict(precision='bf16'), 'act16': dict(precision='bf16', activations='bf16')}
HP = dict(lr=0.3, weight_decay=1e-6, momentum=0.9)
M = 0.99


def _option(name, default):
    for a in sys.argv[1:]:
        if a.startswith(name + '='):
            return a.split('=', 1)[1]
    return default


@torch.no_grad()
def torch_ema(model, m):
    """pm <- pm m + pb (1 - m), three torch launches per parameter pair."""
    pms = list(model.momentum_encoder.parameters())
    for pb, pm in zip(model.base_encoder.parameters(), pms):
        torch.add(pm * m, pb * (1. - m), out=pm)
    torch.autograd.graph.increment_version(pms)        # as the kernel variant: the encoder's bf16 weight copies are made again


class TorchLARS(torch.optim.Optimizer):
    """LARS as per-tensor torch statements, written from the formula ``optimizer.LARS`` documents; for the comparison only."""

    def __init__(self, params, lr=0, weight_decay=0, momentum=0.9, trust_coefficient=0.001):
        super().__init__(params, dict(lr=lr, weight_decay=weight_decay, momentum=momentum, trust_coefficient=trust_coefficient))

    @torch.no_grad()
    def step(self):
        for group in self.param_groups:
            lr, wd, momentum, trust = (group[k] for k in ('lr', 'weight_decay', 'momentum', 'trust_coefficient'))
            for p in group['params']:
                if p.grad is None:
                    continue
                update = p.grad
                if p.ndim > 1:              # matrices: decay, then the trust ratio |p| / |update| (1 when either norm is 0)
                    update = update + wd * p
                    p_norm, u_norm = p.norm(), update.norm()
                    ratio = trust * p_norm / u_norm
                    update = update * torch.where((p_norm > 0) & (u_norm > 0), ratio, torch.ones_like(ratio))
                mu = self.state[p].setdefault('mu', None)
                if mu is None:
                    mu = self.state[p]['mu'] = torch.zeros_like(p)
                mu.mul_(momentum).add_(update)
                p.sub_(mu, alpha=lr)


def windows(fns, reps, inner):
    """alternating windows -> [(median, min, max) ms per call] per function"""
    tss = [[] for _ in fns]
    for _ in range(reps):
        for ts, fn in zip(tss, fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3 / inner)
    return [(statistics.median(ts), min(ts), max(ts)) for ts in tss]


def make(route, depth, kernels, precision='bf16'):
    if route == 'resnet':
        from vit_ae_plus_plus_amd.other_baselines.mocov3.moco.resent3d_base import generate_model
        kw = {} if precision == 'bf16' else dict(precision=precision)
        model = MoCo_ResNet(partial(generate_model, model_depth=10, n_input_channels=4, **kw), 256, 4096, 0.2).cuda().train()
    else:
        enc = partial(VisionTransformer3D, in_chans=4, volume_size=96, depth=depth, **ROUTES[route])
        model = MoCo_ViT(enc, 256, 4096, 0.2).cuda().train()
    if not kernels:
        model._update_momentum_encoder = lambda m, model=model: torch_ema(model, m)
    opt = (LARS if kernels else TorchLARS)(model.parameters(), **HP)
    scaler = torch.cuda.amp.GradScaler()
    return model, opt, scaler


def step_fn(model, opt, scaler, x1, x2):
    def f():
        with torch.cuda.amp.autocast(True):
            loss = model(x1, x2, M)
        opt.zero_grad()
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
    return f


def under(switch, fn, name='VITAE_WEIGHT_SHADOW'):
    """fn with VITAE_WEIGHT_SHADOW (or another switch read at call time) = switch"""
    def f():
        os.environ[name] = switch
        fn()
    return f


def resnet_precision_main(batches, precisions, reps, inner):
    """the routes of the 3-D ResNet under the same MoCo step, one model each, alternating"""
    fmt = lambda t: f'{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})'
    print('| MoCo_ResNet, ResNet-10 | batch / view | ' + ' | '.join(f'{p} ms (min .. max)' for p in precisions) + ' | last / first |')
    print('|---|---|' + '---|' * (len(precisions) + 1))
    for B in batches:
        g = torch.Generator().manual_seed(B)
        x1 = torch.randn(B, 4, 96, 96, 96, generator=g).cuda()
        x2 = torch.randn(B, 4, 96, 96, 96, generator=g).cuda()
        fns = [step_fn(*make('resnet', 0, True, p), x1, x2) for p in precisions]
        for _ in range(2):
            for f in fns:
                f()
        ts = windows(fns, reps, inner)
        print(f'| step | {B} | ' + ' | '.join(fmt(t) for t in ts) + f' | {ts[-1][0] / ts[0][0]:.3f} |', flush=True)
        del fns
        torch.cuda.empty_cache()


def resnet_main(batches, reps, inner):
    if _option('precision', ''):
        return resnet_precision_main(batches, _option('precision', '').split(','), reps, inner)
    fmt = lambda t: f'{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})'
    rows = []
    print('| MoCo_ResNet, ResNet-10 | batch / view | kernels ms (min .. max) | torch statements ms (min .. max) | ratio |')
    print('|---|---|---|---|---|')
    for B in batches:
        g = torch.Generator().manual_seed(B)
        x1 = torch.randn(B, 4, 96, 96, 96, generator=g).cuda()
        x2 = torch.randn(B, 4, 96, 96, 96, generator=g).cuda()
        a, b = make('resnet', 0, True), make('resnet', 0, False)
        fa, fb = step_fn(*a, x1, x2), step_fn(*b, x1, x2)
        for _ in range(3):
            fa(); fb()
        ka, tb = windows([fa, fb], reps, inner)
        print(f'| step | {B} | {fmt(ka)} | {fmt(tb)} | {tb[0] / ka[0]:.3f} |', flush=True)
        del b, fb
        torch.cuda.empty_cache()
        c = make('resnet', 0, True)
        f0, f1 = under('0', fa, 'VITAE_CONV_PACK_STORE'), under('1', step_fn(*c, x1, x2), 'VITAE_CONV_PACK_STORE')
        for _ in range(3):
            f0(); f1()
        off, on = windows([f0, f1], reps, inner)
        os.environ.pop('VITAE_CONV_PACK_STORE', None)
        rows.append(f'| step | {B} | {fmt(off)} | {fmt(on)} | {on[0] / off[0]:.4f} | {off[2] - off[1]:.3f} |')
        del a, c, fa, f0, f1
        torch.cuda.empty_cache()
    print()
    print('| MoCo_ResNet, ResNet-10 | batch / view | a pack per call ms (min .. max) | operand store ms (min .. max) | store / per call | spread of per call ms |')
    print('|---|---|---|---|---|---|')
    for row in rows:
        print(row)


def shadow_main(batches, routes, reps, inner, depth):
    from vit_ae_plus_plus_amd import shadow
    fmt = lambda t: f'{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})'
    print('| route | batch / view | shadow off ms (min .. max) | shadow on ms (min .. max) | on / off | spread of off ms |')
    print('|---|---|---|---|---|---|')
    alone = []
    for route in routes:
        for B in batches:
            g = torch.Generator().manual_seed(B)
            x1 = torch.randn(B, 4, 96, 96, 96, generator=g).cuda()
            x2 = torch.randn(B, 4, 96, 96, 96, generator=g).cuda()
            a, b = make(route, depth, True), make(route, depth, True)
            fa, fb = under('0', step_fn(*a, x1, x2)), under('1', step_fn(*b, x1, x2))
            for _ in range(3):
                fa(); fb()
            off, on = windows([fa, fb], reps, inner)
            print(f'| {route} | {B} | {fmt(off)} | {fmt(on)} | {on[0] / off[0]:.4f} | {off[2] - off[1]:.3f} |', flush=True)
            if not alone:
                n_all = sum(p.numel() for p in a[0].base_encoder.parameters())
                slot = lambda ps: sum(p.numel() for p in ps if shadow.slot_for(p) is not None and shadow.slot_for(p).current())
                train = [p for p in b[0].parameters() if p.grad is not None]
                n_scaled, n_plain = sum(p.numel() for p in train if p.ndim > 1), sum(p.numel() for p in train if p.ndim <= 1)
                s_ema, s_lars = slot(b[0].momentum_encoder.parameters()), slot(train)
                e0, e1 = windows([under('0', lambda: a[0]._update_momentum_encoder(M)), under('1', lambda: b[0]._update_momentum_encoder(M))], reps, 20)
                by0, by1 = 12 * n_all, 12 * n_all + 2 * s_ema
                alone.append(f'| EMA, {n_all / 1e6:.1f} M parameters ({s_ema / 1e6:.1f} M with a slot) | {fmt(e0)} | {fmt(e1)} | {by0 / 1e6:.0f} / {by1 / 1e6:.0f} MB | '
                             f'{by0 / e0[0] / 1e9:.2f} / {by1 / e1[0] / 1e9:.2f} |')
                l0, l1 = windows([under('0', a[1].step), under('1', b[1].step)], reps, 20)
                by0 = 28 * n_scaled + 20 * n_plain
                by1 = by0 + 2 * s_lars
                alone.append(f'| LARS, {(n_scaled + n_plain) / 1e6:.1f} M parameters ({s_lars / 1e6:.1f} M with a slot) | {fmt(l0)} | {fmt(l1)} | {by0 / 1e6:.0f} / {by1 / 1e6:.0f} MB | '
                             f'{by0 / l0[0] / 1e9:.2f} / {by1 / l1[0] / 1e9:.2f} |')
            del a, b, fa, fb
            torch.cuda.empty_cache()
    print()
    print('| launch group alone | shadow off ms (min .. max) | shadow on ms (min .. max) | bytes moved off / on | TB/s off / on |')
    print('|---|---|---|---|---|')
    for row in alone:
        print(row)


def main():
    batches = [int(b) for b in _option('batch', '4,16').split(',')]
    routes = _option('routes', 'act16' if _option('shadow', '') else 'bf16,act16').split(',')
    reps, inner, depth = int(_option('reps', '9')), int(_option('inner', '5')), int(_option('depth', '12'))
    print(f'# device {torch.cuda.get_device_name(0)}; reps {reps} x {inner} steps per window; depth {depth}')
    if _option('arch', 'vit') == 'resnet':
        return resnet_main(batches, reps, inner)
    if _option('shadow', ''):
        if _option('shadow', '') != '0,1':
            sys.exit("moco_bench.py: shadow takes '0,1'")
        return shadow_main(batches, routes, reps, inner, depth)
    print('| route | batch / view | kernels ms (min .. max) | torch statements ms (min .. max) | ratio |')
    print('|---|---|---|---|---|')
    for route in routes:
        for B in batches:
            g = torch.Generator().manual_seed(B)
            x1 = torch.randn(B, 4, 96, 96, 96, generator=g).cuda()
            x2 = torch.randn(B, 4, 96, 96, 96, generator=g).cuda()
            a = make(route, depth, True)
            b = make(route, depth, False)
            fa, fb = step_fn(*a, x1, x2), step_fn(*b, x1, x2)
            for _ in range(3):
                fa(); fb()
            (ma, la, ha), (mb, lb, hb) = windows([fa, fb], reps, inner)
            print(f'| {route} | {B} | {ma:.3f} ({la:.3f} .. {ha:.3f}) | {mb:.3f} ({lb:.3f} .. {hb:.3f}) | {mb / ma:.3f} |', flush=True)
            if route == routes[0] and B == batches[0]:
                alone = groups_alone(a, b, reps)
            del a, b, fa, fb
            torch.cuda.empty_cache()
    print()
    print('| launch group alone | kernels us | torch statements us | bytes moved | kernels TB/s |')
    print('|---|---|---|---|---|')
    for row in alone:
        print(row)


def groups_alone(a, b, reps):
    model, opt, _ = a
    tmodel, topt, _ = b
    n_all = sum(p.numel() for p in model.base_encoder.parameters())
    train = [p for p in model.parameters() if p.grad is not None]
    n_scaled = sum(p.numel() for p in train if p.ndim > 1)
    n_plain = sum(p.numel() for p in train if p.ndim <= 1)
    rows = []
    (ka, _, _), (ta, _, _) = windows([lambda: model._update_momentum_encoder(M), lambda: torch_ema(tmodel, M)], reps, 20)
    by = 12 * n_all
    rows.append(f'| EMA, {n_all / 1e6:.1f} M parameters in {len(list(model.base_encoder.parameters()))} tensors | {ka * 1e3:.1f} | {ta * 1e3:.1f} | {by / 1e6:.0f} MB | {by / (ka * 1e-3) / 1e12:.2f} |')
    (kl, _, _), (tl, _, _) = windows([opt.step, topt.step], reps, 20)
    by = 28 * n_scaled + 20 * n_plain
    rows.append(f'| LARS, {(n_scaled + n_plain) / 1e6:.1f} M parameters in {len(train)} tensors | {kl * 1e3:.1f} | {tl * 1e3:.1f} | {by / 1e6:.0f} MB | {by / (kl * 1e-3) / 1e12:.2f} |')
    for N in (4, 16, 64):
        g = torch.Generator().manual_seed(N)
        q1, k2, q2, k1 = (torch.randn(N, 256, generator=g).cuda() for _ in range(4))
        q1.requires_grad_(); q2.requires_grad_()
        from vit_ae_plus_plus_amd.other_baselines.mocov3.moco.builder import _MocoLoss

        def ours():
            _MocoLoss.apply(q1, k2, q2, k1, 0.2).backward()

        def plain():
            def term(q, k):
                qn, kn = torch.nn.functional.normalize(q, dim=1), torch.nn.functional.normalize(k, dim=1)
                return torch.nn.functional.cross_entropy(qn @ kn.T / 0.2, torch.arange(N, device=q.device)) * 0.4
            (term(q1, k2) + term(q2, k1)).backward()
        (kk, _, _), (tt, _, _) = windows([ours, plain], reps, 20)
        by = 6 * N * 256 * 4
        rows.append(f'| loss + gradients, N = {N}, C = 256 (with the autograd node) | {kk * 1e3:.1f} | {tt * 1e3:.1f} | {by / 1e3:.0f} kB | latency-bound |')
    return rows


if __name__ == '__main__':
    main()
