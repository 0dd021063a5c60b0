"""Time of a fine-tuning step of VisionTransformer3D (ViT-B/16, 96^3 x 4ch, global pool: 217 tokens per volume) on the HIP
training path: forward + backward, and the full step with torch.optim.AdamW over layer-decay groups; batch 4 and 16, fp32 and
bf16, and the --fix_backbone case (head only: the inference path runs and nothing is kept).  Eager launches, as
post_training_utils/fine_tune_epoch.train_one_epoch issues them.  Per case: 5 warm-up iterations, then 50 timed ones, each
between two device synchronisations; the median and the min .. max spread are printed.

Three more rows for the rest of the fine-tuning loop (csrc/classify.hip), each pair timed alternating A / B inside this process:
Mixup of a batch (vitae_mixup_pairs against the torch three-op formulation x.flip(0).mul_(1 - lam); x.mul_(lam).add_(...)), the
criteria (HipCrossEntropyLoss / HipSoftCrossEntropyWithWeightsLoss against torch's, forward + backward on [16, 2] logits) and
evaluate() in volumes/s (batch 16, 4 batches, bf16 and fp32).

    python tools/finetune_bench.py [step] [mixup] [criterion] [evaluate]      (no argument: every row)

``--activations bf16`` (with ``step``): the bf16-activation training route (``VisionTransformer3D(precision='bf16',
activations='bf16')``) against the default bf16 route, timed alternating A / B on two models in this process, with the inference
forward of the same model beside them; ``--batch B`` picks one batch size (default 4 and 16).

    python tools/finetune_bench.py step --activations bf16 [--batch 4]

``optimizer`` (only when named): the whole step of the bf16-activation route through ``NativeScalerWithGradNormCount`` over layer-decay
groups with (a) ``torch.optim.AdamW``, (b) ``torch.optim.AdamW(fused=True)`` where this torch build accepts it, (c)
``optim.MultiTensorAdamW``, the three in turns inside this process, with and without ``clip_grad``; then the optimiser part alone
(norm [+ clipping] + step on the gradients of the last backward) and ``MultiTensorAdamW`` alone at several chunk lengths.

    python tools/finetune_bench.py optimizer [--batch 4]

``optimizer --shadow 0,1``: the bf16 weight shadows (``VITAE_WEIGHT_SHADOW``) off against on: two models with ``MultiTensorAdamW``, one
stepped with the switch at 0 and one with it at 1, in alternating windows of ``--inner`` steps (default 5) in this process, ``--reps``
windows each (default 9); median (min .. max) of the whole step and of the optimiser alone (28 B per parameter off, 30 B on).

    python tools/finetune_bench.py optimizer --shadow 0,1 [--batch 4] [--reps 9] [--inner 5]"""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vit_ae_plus_plus_amd.model.vit import VisionTransformer3D
from vit_ae_plus_plus_amd.utils.lr_decay import param_groups_lrd

WARMUP, ITERS = 5, 50
ARGV = sys.argv[1:]


def _option(name):
    """Value of ``name VALUE`` on the command line (removed from ARGV), or None."""
    if name not in ARGV:
        return None
    i = ARGV.index(name)
    if i + 1 >= len(ARGV):
        sys.exit(f'finetune_bench.py: {name} needs a value')
    value = ARGV[i + 1]
    del ARGV[i:i + 2]
    return value


def _usage(msg):
    sys.exit(f'finetune_bench.py: {msg}\nusage: finetune_bench.py [step] [mixup] [criterion] [evaluate] | step --activations bf16 [--batch B] | optimizer [--batch B]')


ACTIVATIONS, BATCH = _option('--activations'), _option('--batch')
SHADOW, REPS_OPT, INNER_OPT = _option('--shadow'), _option('--reps'), _option('--inner')
ROWS = ARGV or ['step', 'mixup', 'criterion', 'evaluate']
KNOWN = ('step', 'mixup', 'criterion', 'evaluate', 'optimizer')
if [r for r in ROWS if r not in KNOWN]:
    _usage(f'unknown argument(s) {[r for r in ROWS if r not in KNOWN]}')
if ACTIVATIONS is not None and ACTIVATIONS != 'bf16':
    _usage(f"--activations takes 'bf16' (got {ACTIVATIONS!r})")
if ACTIVATIONS and ROWS != ['step'] or BATCH and ROWS not in (['step'], ['optimizer']):
    _usage('--activations / --batch go with the step row alone: finetune_bench.py step --activations bf16 [--batch B]')
if SHADOW is not None and (SHADOW != '0,1' or ROWS != ['optimizer']):
    _usage("--shadow takes '0,1' and goes with the optimizer row: finetune_bench.py optimizer --shadow 0,1 [--batch B] [--reps R] [--inner I]")
if (REPS_OPT or INNER_OPT) and not SHADOW:
    _usage('--reps / --inner go with --shadow')
if BATCH is not None and (not (ACTIVATIONS or ROWS == ['optimizer']) or not BATCH.isdigit() or int(BATCH) < 1):
    _usage('--batch takes a positive integer and goes with --activations or with the optimizer row')


def timed(fn):
    for _ in range(WARMUP):
        fn()
    ts = []
    for _ in range(ITERS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)



def timed_ab(*fns):
    """Medians (and min .. max) of two or more callables timed in turns: A, B, A, B ... so drift of the clocks hits all alike."""
    for _ in range(WARMUP):
        for fn in fns:
            fn()
    tss = [[] for _ in fns]
    for _ in range(ITERS):
        for fn, ts in zip(fns, tss):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    return [(statistics.median(ts), min(ts), max(ts)) for ts in tss]


def mixup_rows():
    from vit_ae_plus_plus_amd._abi import lib
    lam = 0.3
    for B in (4, 16):
        x = torch.randn(B, 4, 96, 96, 96, device='cuda')
        n, st = x.numel() // B, torch.cuda.current_stream().cuda_stream

        def kernel():
            lib.vitae_mixup_pairs(x.data_ptr(), None, lam, B, n, st)

        def three_op():
            flipped = x.flip(0).mul_(1.0 - lam)
            x.mul_(lam).add_(flipped)

        (a, b) = timed_ab(kernel, three_op)
        gb = 2 * x.numel() * 4 / 1e9          # one read and one write of the batch
        print(f'mixup B={B}: vitae_mixup_pairs {a[0] * 1e3:.1f} us ({a[1] * 1e3:.1f} .. {a[2] * 1e3:.1f}; {gb / a[0] * 1e3:.0f} GB/s of its '
              f'own traffic), torch three-op {b[0] * 1e3:.1f} us ({b[1] * 1e3:.1f} .. {b[2] * 1e3:.1f}), ratio {b[0] / a[0]:.2f}', flush=True)
        del x


def criterion_rows():
    from vit_ae_plus_plus_amd.utils.custom_loss import (HipCrossEntropyLoss, HipSoftCrossEntropyWithWeightsLoss,
                                                        SoftCrossEntropyWithWeightsLoss)
    w = torch.tensor([1.0, 2.5])
    logits = torch.randn(16, 2, device='cuda', requires_grad=True)
    hard = torch.randint(0, 2, (16,), device='cuda')
    soft = torch.softmax(torch.randn(16, 2, device='cuda'), dim=-1)
    for name, hip, ref, target in (('cross entropy', HipCrossEntropyLoss(w).cuda(), torch.nn.CrossEntropyLoss(weight=w).cuda(), hard),
                                   ('soft cross entropy', HipSoftCrossEntropyWithWeightsLoss(w).cuda(),
                                    SoftCrossEntropyWithWeightsLoss(w).cuda(), soft)):
        def run(crit):
            def f():
                logits.grad = None
                crit(logits, target).backward()
            return f

        (a, b) = timed_ab(run(hip), run(ref))
        print(f'criterion {name} [16, 2], forward + backward: HIP {a[0] * 1e3:.1f} us ({a[1] * 1e3:.1f} .. {a[2] * 1e3:.1f}), torch '
              f'{b[0] * 1e3:.1f} us ({b[1] * 1e3:.1f} .. {b[2] * 1e3:.1f}), ratio {b[0] / a[0]:.2f}', flush=True)


def evaluate_rows():
    import contextlib, io
    from argparse import Namespace
    from vit_ae_plus_plus_amd.post_training_utils.fine_tune_epoch import evaluate
    B, n_batches = 16, 4
    loader = [(torch.randn(B, 4, 96, 96, 96, device='cuda'), None, torch.randint(0, 2, (B,), device='cuda')) for _ in range(n_batches)]
    loader[0][2][:2] = torch.tensor([0, 1])          # both classes, whatever the draw
    args = Namespace(cross_entropy_wt=torch.tensor([1.0, 2.5]))
    models = {}
    for precision in ('bf16', 'fp32'):
        m = VisionTransformer3D(volume_size=96, patch_size=16, in_chans=4, num_classes=2, global_pool=True, precision=precision).cuda()
        torch.nn.init.normal_(m.head.weight, std=0.02)
        models[precision] = m

    def run(precision):
        def f():
            with contextlib.redirect_stdout(io.StringIO()):
                evaluate(loader, models[precision], torch.device('cuda'), args)
        return f

    global ITERS
    saved, ITERS = ITERS, 10
    (a, b) = timed_ab(run('bf16'), run('fp32'))
    ITERS = saved
    for precision, t in (('bf16', a), ('fp32', b)):
        print(f'evaluate {precision} B={B} x {n_batches} batches: {t[0]:.2f} ms ({t[1]:.2f} .. {t[2]:.2f}), '
              f'{B * n_batches / t[0] * 1e3:.0f} volumes/s', flush=True)


def act16_rows():
    """The two bf16 training routes in turns: forward + backward, the step with AdamW, kept MiB; and the inference forward."""
    for B in ([int(BATCH)] if BATCH else [4, 16]):
        x = torch.randn(B, 4, 96, 96, 96, device='cuda')
        y = torch.randint(0, 2, (B,), device='cuda')
        crit = torch.nn.CrossEntropyLoss()
        fns, models = {}, {}
        for act in (None, ACTIVATIONS):
            m = VisionTransformer3D(volume_size=96, patch_size=16, in_chans=4, num_classes=2, global_pool=True, precision='bf16',
                                    activations=act, drop_path_rate=0.1).cuda().train()
            torch.nn.init.normal_(m.head.weight, std=0.02)        # a zero head gives zero encoder gradients
            opt = torch.optim.AdamW(param_groups_lrd(m, 0.05, m.no_weight_decay(), 0.75), lr=1e-3)

            def fwd_bwd(m=m, opt=opt):
                opt.zero_grad(set_to_none=True)
                crit(m(x), y).backward()

            def step(m=m, opt=opt, fwd_bwd=fwd_bwd):
                fwd_bwd()
                opt.step()

            fns[act], models[act] = (fwd_bwd, step), m

        def infer(m=models[ACTIVATIONS]):
            with torch.no_grad():
                m(x)

        fb = timed_ab(fns[None][0], fns[ACTIVATIONS][0])
        st = timed_ab(fns[None][1], fns[ACTIVATIONS][1])
        inf = timed(infer)
        for (name, act), a, b in zip((('default', None), (ACTIVATIONS, ACTIVATIONS)), fb, st):
            print(f'bf16 B={B} activations={name!s:8s}: forward+backward {a[0]:.2f} ms ({a[1]:.2f} .. {a[2]:.2f}), step with AdamW {b[0]:.2f} ms '
                  f'({b[1]:.2f} .. {b[2]:.2f}), {B / b[0] * 1e3:.0f} volumes/s, kept {models[act]._trainer.stats["kept_bytes"] / 2 ** 20:.0f} MiB',
                  flush=True)
        print(f'bf16 B={B} inference forward {inf[0]:.2f} ms ({inf[1]:.2f} .. {inf[2]:.2f}); forward+backward / forward: default '
              f'{fb[0][0] / inf[0]:.1f}x, {ACTIVATIONS} {fb[1][0] / inf[0]:.1f}x; new / default {fb[1][0] / fb[0][0]:.3f} (forward+backward), '
              f'{st[1][0] / st[0][0]:.3f} (step)', flush=True)
        del fns, models, x


def optimizer_rows():
    """torch.optim.AdamW, its fused form and MultiTensorAdamW in turns: the whole step through the scaler, then the optimiser part alone."""
    from vit_ae_plus_plus_amd.optim import MultiTensorAdamW
    from vit_ae_plus_plus_amd.utils.misc import NativeScalerWithGradNormCount, get_grad_norm_
    LR = 1e-5        # several hundred steps on one batch: small enough that no route ever sees a non-finite gradient (checked below)
    makers = [('torch.optim.AdamW', lambda g: torch.optim.AdamW(g, lr=LR))]
    try:
        probe = torch.nn.Parameter(torch.zeros(4, device='cuda'))
        probe.grad = torch.zeros_like(probe)
        torch.optim.AdamW([probe], fused=True).step()
        makers.append(('torch.optim.AdamW(fused=True)', lambda g: torch.optim.AdamW(g, lr=LR, fused=True)))
    except Exception as e:      # this build has no fused AdamW for the device: the row is left out, and said so
        print(f'optimizer: torch.optim.AdamW(fused=True) is not available here ({type(e).__name__}: {e})', flush=True)
    makers.append(('MultiTensorAdamW', lambda g: MultiTensorAdamW(g, lr=LR)))
    scaler = NativeScalerWithGradNormCount()
    for B in ([int(BATCH)] if BATCH else [4, 16]):
        x = torch.randn(B, 4, 96, 96, 96, device='cuda')
        y = torch.randint(0, 2, (B,), device='cuda')
        crit = torch.nn.CrossEntropyLoss()
        runs = []
        for name, make in makers:
            m = VisionTransformer3D(volume_size=96, patch_size=16, in_chans=4, num_classes=2, global_pool=True, precision='bf16',
                                    activations='bf16', drop_path_rate=0.1).cuda().train()
            torch.nn.init.normal_(m.head.weight, std=0.02)
            runs.append((name, m, make(param_groups_lrd(m, 0.05, m.no_weight_decay(), 0.75))))
        n_params = sum(p.numel() for p in runs[0][1].parameters())
        print(f'optimizer B={B}: {n_params / 1e6:.1f} M parameters in {len(list(runs[0][1].parameters()))} tensors, '
              f'{len(runs[0][2].param_groups)} groups', flush=True)
        medians = {}
        for clip in (None, 1.0):
            def whole(m, opt):
                def f():
                    opt.zero_grad(set_to_none=True)
                    scaler(crit(m(x), y), opt, clip_grad=clip, parameters=m.parameters())
                return f

            def alone(m, opt):      # on the gradients the last whole step left behind
                params = list(m.parameters())
                if hasattr(opt, 'norm_clip_step'):
                    return lambda: opt.norm_clip_step(clip)

                def f():
                    if clip is not None:
                        torch.nn.utils.clip_grad_norm_(params, clip)
                    else:
                        get_grad_norm_(params)
                    opt.step()
                return f

            ws = timed_ab(*[whole(m, opt) for _, m, opt in runs])
            os_ = timed_ab(*[alone(m, opt) for _, m, opt in runs])
            for (name, _, _), w, o in zip(runs, ws, os_):
                medians[(name, clip)] = w
                print(f'optimizer B={B} clip_grad={clip!s:4s} {name:30s}: whole step {w[0]:.3f} ms ({w[1]:.3f} .. {w[2]:.3f}), optimiser alone '
                      f'{o[0]:.3f} ms ({o[1]:.3f} .. {o[2]:.3f}) = {28 * n_params / o[0] / 1e9:.2f} TB/s at 28 B per parameter', flush=True)
            a, c = medians[(makers[0][0], clip)], medians[('MultiTensorAdamW', clip)]
            spread = max(a[2] - a[1], c[2] - c[1])
            print(f'optimizer B={B} clip_grad={clip}: MultiTensorAdamW / torch.optim.AdamW = {c[0] / a[0]:.3f} (whole step; gain {a[0] - c[0]:.3f} ms, '
                  f'larger min .. max spread {spread:.3f} ms)', flush=True)
        _, m, opt = runs[-1]
        lengths = (4096, 8192, 16384, 32768, 65536)

        REPS = 8     # calls issued back to back per sample: the host prepares call k + 1 while the device runs call k

        def with_chunk(c, reps):
            def f():
                opt._chunk = c
                for _ in range(reps):
                    opt.norm_clip_step(None)
            return f

        one = timed_ab(*[with_chunk(c, 1) for c in lengths])
        many = timed_ab(*[with_chunk(c, REPS) for c in lengths])
        for c, t, q in zip(lengths, one, many):
            print(f'optimizer B={B} MultiTensorAdamW alone, chunk {c:6d}: one call {t[0]:.3f} ms ({t[1]:.3f} .. {t[2]:.3f}); {REPS} calls back to '
                  f'back {q[0] / REPS:.3f} ms each ({q[1] / REPS:.3f} .. {q[2] / REPS:.3f}) = {28 * n_params / q[0] * REPS / 1e9:.2f} TB/s', flush=True)
        finite = all(bool(torch.isfinite(p).all()) for p in m.parameters())
        print(f'optimizer B={B}: MultiTensorAdamW applied {opt.applied_steps()} steps, skipped {opt.skipped_steps()}; parameters finite: {finite}',
              flush=True)
        del runs, m, opt, x


def shadow_rows():
    """MultiTensorAdamW with the bf16 weight shadows off and on, in alternating windows: whole step and optimiser alone."""
    from vit_ae_plus_plus_amd.optim import MultiTensorAdamW
    from vit_ae_plus_plus_amd.utils.misc import NativeScalerWithGradNormCount
    reps, inner = int(REPS_OPT or 9), int(INNER_OPT or 5)
    scaler = NativeScalerWithGradNormCount()
    crit = torch.nn.CrossEntropyLoss()

    def windows(fns, inner):
        tss = [[] for _ in fns]
        for _ in range(reps):
            for fn, ts in zip(fns, tss):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(inner):
                    fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3 / inner)
        return [(statistics.median(ts), min(ts), max(ts)) for ts in tss]

    print(f'shadow: {reps} alternating windows of {inner} steps per variant; ms per step, median (min .. max)', flush=True)
    print('| batch | clip_grad | what | shadow off | shadow on | on / off | spread of off |')
    print('|---|---|---|---|---|---|---|')
    for B in ([int(BATCH)] if BATCH else [4, 16]):
        x = torch.randn(B, 4, 96, 96, 96, device='cuda')
        y = torch.randint(0, 2, (B,), device='cuda')
        runs = []
        for switch in ('0', '1'):       # each model lives under one setting: its slots are never current (off) or always (on)
            m = VisionTransformer3D(volume_size=96, patch_size=16, in_chans=4, num_classes=2, global_pool=True, precision='bf16',
                                    activations='bf16', drop_path_rate=0.1).cuda().train()
            torch.nn.init.normal_(m.head.weight, std=0.02)
            runs.append((switch, m, MultiTensorAdamW(param_groups_lrd(m, 0.05, m.no_weight_decay(), 0.75), lr=1e-5)))
        n_params = sum(p.numel() for p in runs[0][1].parameters())
        for clip in (None, 1.0):
            def whole(switch, m, opt):
                def f():
                    os.environ['VITAE_WEIGHT_SHADOW'] = switch
                    opt.zero_grad(set_to_none=True)
                    scaler(crit(m(x), y), opt, clip_grad=clip, parameters=m.parameters())
                return f

            def alone(switch, m, opt):      # on the gradients the last whole step left behind
                def f():
                    os.environ['VITAE_WEIGHT_SHADOW'] = switch
                    opt.norm_clip_step(clip)
                return f

            for fn in [whole(*r) for r in runs] * 3:
                fn()
            (a, b) = windows([whole(*r) for r in runs], inner)
            (c, d) = windows([alone(*r) for r in runs], 4 * inner)
            fmt = lambda t: f'{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})'
            print(f'| {B} | {clip} | whole step | {fmt(a)} | {fmt(b)} | {b[0] / a[0]:.4f} | {a[2] - a[1]:.3f} |', flush=True)
            print(f'| {B} | {clip} | optimiser alone, {n_params / 1e6:.1f} M parameters | {fmt(c)} = {28 * n_params / c[0] / 1e9:.2f} TB/s at 28 B | '
                  f'{fmt(d)} = {30 * n_params / d[0] / 1e9:.2f} TB/s at 30 B | {d[0] / c[0]:.4f} | {c[2] - c[1]:.3f} |', flush=True)
        for switch, m, opt in runs:
            print(f'shadow {switch} B={B}: applied {opt.applied_steps()} steps, skipped {opt.skipped_steps()}', flush=True)
        del runs, x
        torch.cuda.empty_cache()


if 'optimizer' in ROWS and SHADOW:
    shadow_rows()
elif 'optimizer' in ROWS:
    optimizer_rows()
if 'step' in ROWS and ACTIVATIONS:
    act16_rows()
elif 'step' in ROWS:
    for precision in ('fp32', 'bf16'):
        for B in (4, 16):
            for fix_backbone in (False, True):
                m = VisionTransformer3D(volume_size=96, patch_size=16, in_chans=4, num_classes=2, global_pool=True, precision=precision,
                                        drop_path_rate=0.1).cuda().train()
                torch.nn.init.normal_(m.head.weight, std=0.02)        # a zero head gives zero encoder gradients
                if fix_backbone:
                    for n, p in m.named_parameters():
                        p.requires_grad = n.startswith('head.')
                opt = torch.optim.AdamW(param_groups_lrd(m, 0.05, m.no_weight_decay(), 0.75), lr=1e-3)
                crit = torch.nn.CrossEntropyLoss()
                x = torch.randn(B, 4, 96, 96, 96, device='cuda')
                y = torch.randint(0, 2, (B,), device='cuda')

                def fwd_bwd():
                    opt.zero_grad(set_to_none=True)
                    crit(m(x), y).backward()

                def step():
                    fwd_bwd()
                    opt.step()

                a, b = timed(fwd_bwd), timed(step)
                kept = m._trainer.stats['kept_bytes'] / 2 ** 20 if m._trainer is not None else 0.0
                print(f'{precision} B={B} {"fix_backbone" if fix_backbone else "full":12s}: forward+backward {a[0]:.2f} ms ({a[1]:.2f} .. {a[2]:.2f}), '
                      f'step with AdamW {b[0]:.2f} ms ({b[1]:.2f} .. {b[2]:.2f}), {B / b[0] * 1e3:.0f} volumes/s, kept {kept:.0f} MiB', flush=True)
                del m, opt

if 'mixup' in ROWS:
    mixup_rows()
if 'criterion' in ROWS:
    criterion_rows()
if 'evaluate' in ROWS:
    evaluate_rows()
