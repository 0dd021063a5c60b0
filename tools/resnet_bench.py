"""Time of a training step of the 3-D ResNet-10 baseline (96^3 x 4 channels, 2 classes) on the HIP route of
k_fold_training_scripts/resnet_3d.py against a module of the same structure built here from plain nn.Conv3d / nn.BatchNorm3d /
nn.MaxPool3d and run under torch.autocast(bfloat16) (MIOpen): forward + backward, the whole step with torch.optim.Adam, the two
routes timed in turns A, B, A, B ... inside this process, each timed call between two device synchronisations; kept MiB of the HIP
route; then a per-kernel table of one HIP step (every launch sequence of vit_ae_plus_plus_amd.resnet between two synchronisations).

    python tools/resnet_bench.py [step] [kernels] [--batch B] [--iters N]        (no argument: both rows, batch 4 and 16)
    python tools/resnet_bench.py pack [--batch B] [--iters N]

``pack``: the HIP step with the per-model operand store (``resnet.ConvPackStore``: every stale convolution operand in one
``vitae_conv3d_pack_weights_multi`` launch per step) against a pack per convolution call (``VITAE_CONV_PACK_STORE=0``), two models
alternating in this process.

    python tools/resnet_bench.py precision [--batch B] [--iters N]

``precision``: the HIP model on its two routes (``precision='bf16'`` and ``'fp32x3'``), one model each, alternating in this process.
"""
import collections
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn

from vit_ae_plus_plus_amd import resnet as seq
from vit_ae_plus_plus_amd.k_fold_training_scripts.resnet_3d import generate_model

ARGV = sys.argv[1:]


def _option(name, default):
    if name not in ARGV:
        return default
    i = ARGV.index(name)
    value = int(ARGV[i + 1])
    del ARGV[i:i + 2]
    return value


BATCH, ITERS, WARMUP = _option('--batch', None), _option('--iters', 10), 2
ROWS = ARGV or ['step', 'kernels']
VOLUME, CHANNELS = 96, 4


class TorchBlock(nn.Module):
    def __init__(self, cin, planes, stride):
        super().__init__()
        self.conv1 = nn.Conv3d(cin, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm3d(planes)
        self.conv2 = nn.Conv3d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm3d(planes)
        self.downsample = None
        if stride != 1 or cin != planes:
            self.downsample = nn.Sequential(nn.Conv3d(cin, planes, 1, stride, bias=False), nn.BatchNorm3d(planes))

    def forward(self, x):
        out = self.bn2(self.conv2(torch.relu(self.bn1(self.conv1(x)))))
        return torch.relu(out + (x if self.downsample is None else self.downsample(x)))


class TorchResNet10(nn.Module):
    """The same structure on torch's own operators (the comparison, never the product)."""

    def __init__(self, cin, n_classes):
        super().__init__()
        self.conv1 = nn.Conv3d(cin, 64, 7, (1, 2, 2), 3, bias=False)
        self.bn1 = nn.BatchNorm3d(64)
        self.maxpool = nn.MaxPool3d(3, 2, 1)
        self.layers = nn.Sequential(TorchBlock(64, 64, 1), TorchBlock(64, 128, 2), TorchBlock(128, 256, 2), TorchBlock(256, 512, 2))
        self.fc = nn.Linear(512, n_classes)

    def forward(self, x):
        x = self.layers(self.maxpool(torch.relu(self.bn1(self.conv1(x)))))
        return self.fc(x.mean((2, 3, 4)))


def timed_ab(*fns):
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


def kept_mib(kept):
    seen, total = set(), 0

    def walk(o):
        nonlocal total
        if torch.is_tensor(o):
            if o.data_ptr() not in seen:
                seen.add(o.data_ptr())
                total += o.numel() * o.element_size()
        elif isinstance(o, dict):
            for v in o.values():
                walk(v)
        elif isinstance(o, (list, tuple)):
            for v in o:
                walk(v)
    walk(kept)
    return total / 2 ** 20


def step_rows(B):
    x = torch.randn(B, CHANNELS, VOLUME, VOLUME, VOLUME, device='cuda')
    y = torch.randint(0, 2, (B,), device='cuda')
    crit = nn.CrossEntropyLoss(weight=torch.tensor([3.0, 1.0], device='cuda'))
    hip = generate_model(10, n_classes=2, n_input_channels=CHANNELS).cuda().train()
    ref = TorchResNet10(CHANNELS, 2).cuda().train()
    opts = [torch.optim.Adam(m.parameters(), lr=1e-4) for m in (hip, ref)]

    def fb_hip():
        opts[0].zero_grad(set_to_none=True)
        crit(hip(x), y).backward()

    def fb_ref():
        opts[1].zero_grad(set_to_none=True)
        with torch.autocast('cuda', dtype=torch.bfloat16):
            loss = crit(ref(x), y)
        loss.backward()

    def step_hip():
        fb_hip()
        opts[0].step()

    def step_ref():
        fb_ref()
        opts[1].step()

    fb, st = timed_ab(fb_hip, fb_ref), timed_ab(step_hip, step_ref)
    _, kept = seq.HipResNetRunner(hip).forward_keep(x)
    for name, a, b in (('HIP', fb[0], st[0]), ('torch autocast (MIOpen)', fb[1], st[1])):
        print(f'resnet10 B={B} {name:24s}: forward+backward {a[0]:.2f} ms ({a[1]:.2f} .. {a[2]:.2f}), step with Adam {b[0]:.2f} ms '
              f'({b[1]:.2f} .. {b[2]:.2f}), {B / b[0] * 1e3:.1f} volumes/s', flush=True)
    print(f'resnet10 B={B}: HIP / torch = {fb[0][0] / fb[1][0]:.2f} (forward+backward), {st[0][0] / st[1][0]:.2f} (step); HIP keeps '
          f'{kept_mib(kept):.0f} MiB for the backward', flush=True)


def pack_rows(B):
    x = torch.randn(B, CHANNELS, VOLUME, VOLUME, VOLUME, device='cuda')
    y = torch.randint(0, 2, (B,), device='cuda')
    crit = nn.CrossEntropyLoss(weight=torch.tensor([3.0, 1.0], device='cuda'))
    models = [generate_model(10, n_classes=2, n_input_channels=CHANNELS).cuda().train() for _ in range(2)]
    opts = [torch.optim.Adam(m.parameters(), lr=1e-4) for m in models]

    def step(i, switch):
        def f():
            os.environ['VITAE_CONV_PACK_STORE'] = switch
            opts[i].zero_grad(set_to_none=True)
            crit(models[i](x), y).backward()
            opts[i].step()
        return f

    off, on = timed_ab(step(0, '0'), step(1, '1'))
    os.environ.pop('VITAE_CONV_PACK_STORE', None)
    fmt = lambda t: f'{t[0]:.3f} ms ({t[1]:.3f} .. {t[2]:.3f})'
    print(f'resnet10 B={B} step with Adam: a pack per call {fmt(off)}, operand store {fmt(on)}, store / per call = {on[0] / off[0]:.4f}; '
          f'{seq.pack_store_of(models[1]).launches} pack launches in {ITERS + WARMUP} steps', flush=True)


def precision_rows(B):
    """The two routes of the HIP model, one model each, alternating: forward + backward and the step with Adam; kept MiB of each."""
    x = torch.randn(B, CHANNELS, VOLUME, VOLUME, VOLUME, device='cuda')
    y = torch.randint(0, 2, (B,), device='cuda')
    crit = nn.CrossEntropyLoss(weight=torch.tensor([3.0, 1.0], device='cuda'))
    models = [generate_model(10, n_classes=2, n_input_channels=CHANNELS, precision=p).cuda().train() for p in seq.PRECISIONS]
    opts = [torch.optim.Adam(m.parameters(), lr=1e-4) for m in models]

    def fb(i):
        def f():
            opts[i].zero_grad(set_to_none=True)
            crit(models[i](x), y).backward()
        return f

    def step(i):
        def f():
            fb(i)()
            opts[i].step()
        return f

    n = range(len(models))
    tf, ts = timed_ab(*(fb(i) for i in n)), timed_ab(*(step(i) for i in n))
    for i, p in enumerate(seq.PRECISIONS):
        _, kept = seq.HipResNetRunner(models[i]).forward_keep(x)
        print(f'resnet10 B={B} precision {p:7s}: forward+backward {tf[i][0]:.2f} ms ({tf[i][1]:.2f} .. {tf[i][2]:.2f}), step with Adam {ts[i][0]:.2f} ms '
              f'({ts[i][1]:.2f} .. {ts[i][2]:.2f}), keeps {kept_mib(kept):.0f} MiB', flush=True)
        del kept
    print(f'resnet10 B={B}: {seq.PRECISIONS[1]} / {seq.PRECISIONS[0]} = {tf[1][0] / tf[0][0]:.2f} (forward+backward), {ts[1][0] / ts[0][0]:.2f} (step)', flush=True)


def kernel_rows(B):
    """One HIP step with every launch sequence of vit_ae_plus_plus_amd.resnet timed on its own (synchronised before and after)."""
    table = collections.OrderedDict()

    def wrap(name, label):
        fn = getattr(seq, name)

        def timed(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            key = label(*a, **k)
            table.setdefault(key, []).append((time.perf_counter() - t0) * 1e3)
            return out
        setattr(seq, name, timed)
        return fn

    conv_label = lambda kind: lambda t, N, vol, conv, **k: (f'{kind} {conv.in_channels}->{conv.out_channels} k{conv.kernel_size[1]} '
                                                             f's{conv.stride[1]} in {vol}')
    saved = {n: wrap(n, l) for n, l in (('conv_fwd', conv_label('conv fwd')), ('conv_bwd_input', conv_label('conv dX')),
                                        ('conv_bwd_weight', lambda d, x, N, vol, conv, **k: conv_label('conv dW')(d, N, vol, conv)),
                                        ('bn_tail_train', lambda x, res, bn, relu, w16: f'bn tail fwd {tuple(x.shape)}'),
                                        ('bn_tail_bwd', lambda dy, x, *a, **k: f'bn tail bwd {tuple(x.shape)}'))}
    try:
        x = torch.randn(B, CHANNELS, VOLUME, VOLUME, VOLUME, device='cuda')
        y = torch.randint(0, 2, (B,), device='cuda')
        m = generate_model(10, n_classes=2, n_input_channels=CHANNELS).cuda().train()
        for it in range(3):
            if it == 2:
                table.clear()
            m.zero_grad(set_to_none=True)
            nn.functional.cross_entropy(m(x), y).backward()
        torch.cuda.synchronize()
    finally:
        for n, fn in saved.items():
            setattr(seq, n, fn)
    total = sum(sum(v) for v in table.values())
    print(f'resnet10 B={B} per launch sequence of one step (each alone on an idle device; sum {total:.2f} ms):')
    for key, v in sorted(table.items(), key=lambda kv: -sum(kv[1])):
        print(f'  {sum(v):9.3f} ms  {100 * sum(v) / total:5.1f} %  x{len(v)}  {key}', flush=True)


for B in ([BATCH] if BATCH else [4, 16]):
    if 'step' in ROWS:
        step_rows(B)
    if 'kernels' in ROWS:
        kernel_rows(B)
    if 'pack' in ROWS:
        pack_rows(B)
    if 'precision' in ROWS:
        precision_rows(B)
    torch.cuda.empty_cache()
