"""Time of a fine-tuning step of VisionTransformer3D (ViT-B/16, 96^3 x 4ch, global pool: 217 tokens per volume) on the HIP
training path: forward + backward, and the full step with torch.optim.AdamW over layer-decay groups; batch 4 and 16, fp32 and
bf16, and the --fix_backbone case (head only: the inference path runs and nothing is kept).  Eager launches, as
post_training_utils/fine_tune_epoch.train_one_epoch issues them.  Per case: 5 warm-up iterations, then 50 timed ones, each
between two device synchronisations; the median and the min .. max spread are printed.

Three more rows for the rest of the fine-tuning loop (csrc/classify.hip), each pair timed alternating A / B inside this process:
Mixup of a batch (vitae_mixup_pairs against the torch three-op formulation x.flip(0).mul_(1 - lam); x.mul_(lam).add_(...)), the
criteria (HipCrossEntropyLoss / HipSoftCrossEntropyWithWeightsLoss against torch's, forward + backward on [16, 2] logits) and
evaluate() in volumes/s (batch 16, 4 batches, bf16 and fp32).

    python tools/finetune_bench.py [step] [mixup] [criterion] [evaluate]      (no argument: every row)"""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vit_ae_plus_plus_amd.model.vit import VisionTransformer3D
from vit_ae_plus_plus_amd.utils.lr_decay import param_groups_lrd

WARMUP, ITERS = 5, 50
ROWS = sys.argv[1:] or ['step', 'mixup', 'criterion', 'evaluate']


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



def timed_ab(fa, fb):
    """Medians (and min .. max) of two callables timed in turns: A, B, A, B ... so drift of the clocks hits both alike."""
    for _ in range(WARMUP):
        fa()
        fb()
    ta, tb = [], []
    for _ in range(ITERS):
        for fn, ts in ((fa, ta), (fb, tb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    return [(statistics.median(ts), min(ts), max(ts)) for ts in (ta, tb)]


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


if 'step' in ROWS:
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
