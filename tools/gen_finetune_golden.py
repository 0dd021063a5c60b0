"""Writes tests/golden/vit_finetune.npz: what the REFERENCE's own VisionTransformer3D computes when it is fine-tuned on the
micro encoder configuration (build container only: needs the reference checkout, see oracle/_refharness.py).

    python tools/gen_finetune_golden.py [--out other.npz]

Configuration: the micro encoder of vit_features.npz (oracle.gen_golden.MICRO, 3 classes), weights
``oracle.vit_ref.init_vit_state_dict(cfg, seed=5)`` (non-zero head), input ``micro/x`` of vit_features.npz, labels [0, 2, 1],
class weights [1, 2, 0.5].  Per pooling mode (``cls`` / ``gp``):

    <tag>/loss, <tag>/logits, <tag>/names, <tag>/grad/<name>     cross_entropy(weight) forward + backward
    <tag>/adamw_losses                                           4 steps of torch.optim.AdamW(lr=1e-3, weight_decay=0.05)
    <tag>/bf16_ref_relerr/<name>                                 relative L2 error of the gradients under
                                                                 torch.autocast('cpu', bfloat16) against the fp32 ones
    <tag>/soft/loss, <tag>/soft/grad_norm                        SoftCrossEntropyWithWeightsLoss on soft targets

``gp`` only: ``epoch/*`` — one epoch of the reference's fine-tune iteration (fine_tune_epoch.py:34-100: per-iteration
lr_sched.adjust_learning_rate, loss / accum_iter, step and zero_grad on the last iteration of a group) with accum_iter = 2
over two batches, soft targets, AdamW over the reference's param_groups_lrd groups; the parameters after the epoch are
stored as deltas.  ``lrd/*``: the reference's param_groups_lrd table for this depth-2 model.
"""
import importlib
import os
import sys
import types
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import _refharness as H          # noqa: E402
from oracle import vit_ref as V              # noqa: E402
from oracle.gen_golden import MICRO, _build_reference_vit, _np, load_into_reference   # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'vit_finetune.npz')
ENC = {k: MICRO[k] for k in ('volume_size', 'patch_size', 'in_chans', 'embed_dim', 'depth', 'num_heads')}
LABELS = [0, 2, 1]
CLASS_WEIGHTS = [1.0, 2.0, 0.5]
EPOCH_ARGS = dict(accum_iter=2, lr=1e-3, min_lr=0.0, warmup_epochs=1, epochs=4)
EPOCH, LAYER_DECAY, WEIGHT_DECAY = 1, 0.75, 0.05


def soft_targets():
    """Two batches of mixed-up-looking targets (rows sum to 1)."""
    g = torch.Generator().manual_seed(23)
    return [torch.softmax(2.0 * torch.randn(3, 3, generator=g), dim=-1) for _ in range(2)]


def epoch_batches(x):
    ta, tb = soft_targets()
    return [(x, None, ta), (x.flip(0).contiguous(), None, tb)]


def _reference_extras(ref):
    """utils.lr_decay and utils.custom_loss of the reference (the latter imports timm.loss for a self-check only)."""
    if 'timm.loss' not in sys.modules:
        m = types.ModuleType('timm.loss')
        m.SoftTargetCrossEntropy = type('SoftTargetCrossEntropy', (torch.nn.Module,), {})
        sys.modules['timm.loss'] = m
    utils_pkg = sys.modules[ref.lr_sched.__name__.rsplit('.', 1)[0]]
    assert os.path.dirname(utils_pkg.__file__).startswith(H.REFERENCE_ROOT), utils_pkg.__file__
    return importlib.import_module('utils.lr_decay'), importlib.import_module('utils.custom_loss')


def _model(ref, cfg):
    model = _build_reference_vit(ref, cfg)
    load_into_reference(model, V.init_vit_state_dict(cfg, seed=5))
    return model.train()


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def generate():
    torch.manual_seed(0)
    torch.set_num_threads(1)      # one summation order whatever the machine's core count: the fixture regenerates byte for byte
    ref = H.import_reference()
    lrd, custom_loss = _reference_extras(ref)
    x = torch.from_numpy(np.load(os.path.join(ROOT, 'tests', 'golden', 'vit_features.npz'))['micro/x'])
    y = torch.tensor(LABELS)
    cw = torch.tensor(CLASS_WEIGHTS)
    ce = torch.nn.CrossEntropyLoss(weight=cw)
    out = {'labels': np.array(LABELS, dtype=np.int64), 'class_weights': np.array(CLASS_WEIGHTS, dtype=np.float32)}
    for gp in (False, True):
        tag = 'gp' if gp else 'cls'
        cfg = V.VitConfig(num_classes=3, global_pool=gp, **ENC)
        # loss, logits, gradients
        model = _model(ref, cfg)
        logits = model(x)
        loss = ce(logits, y)
        loss.backward()
        g32 = _grads(model)
        names = list(g32.keys())
        out[f'{tag}/names'] = np.array(names)
        out[f'{tag}/loss'] = _np(loss)
        out[f'{tag}/logits'] = _np(logits)
        for n in names:
            assert float(g32[n].norm()) > 0, n
            out[f'{tag}/grad/{n}'] = _np(g32[n])
        # the reference's own loss of precision under bf16 autocast
        model = _model(ref, cfg)
        with torch.autocast('cpu', dtype=torch.bfloat16):
            l16 = ce(model(x), y)
        l16.backward()
        g16 = _grads(model)
        for n in names:
            out[f'{tag}/bf16_ref_relerr/{n}'] = _np((g16[n].float() - g32[n]).norm() / g32[n].norm())
        # 4 steps of AdamW on the same batch
        model = _model(ref, cfg)
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=0.05)
        losses = []
        for _ in range(4):
            opt.zero_grad()
            l = ce(model(x), y)
            l.backward()
            opt.step()
            losses.append(float(l.detach()))
        out[f'{tag}/adamw_losses'] = np.array(losses, dtype=np.float64)
        # soft targets
        model = _model(ref, cfg)
        soft = custom_loss.SoftCrossEntropyWithWeightsLoss(weights=cw.clone())
        ls = soft(model(x), soft_targets()[0])
        ls.backward()
        out[f'{tag}/soft/loss'] = _np(ls)
        out[f'{tag}/soft/grad_norm'] = np.array([float(p.grad.norm()) for _, p in model.named_parameters()], dtype=np.float64)
        print(tag, 'loss', float(loss), 'adamw', losses, 'soft', float(ls),
              'bf16 relerr %.4f..%.4f' % (min(float(out[f'{tag}/bf16_ref_relerr/{n}']) for n in names),
                                          max(float(out[f'{tag}/bf16_ref_relerr/{n}']) for n in names)),
              'min |grad| %.3g' % min(float(g32[n].norm()) for n in names))

    # one epoch with gradient accumulation, soft targets and layer-decay groups (global pool)
    cfg = V.VitConfig(num_classes=3, global_pool=True, **ENC)
    model = _model(ref, cfg)
    groups = lrd.param_groups_lrd(model, WEIGHT_DECAY, no_weight_decay_list=model.no_weight_decay(), layer_decay=LAYER_DECAY)
    name_of = {id(p): n for n, p in model.named_parameters()}
    rows = [(name_of[id(p)], gi, g['lr_scale'], g['weight_decay']) for gi, g in enumerate(groups) for p in g['params']]
    out['lrd/names'] = np.array([r[0] for r in rows])
    out['lrd/group'] = np.array([r[1] for r in rows], dtype=np.int64)
    out['lrd/lr_scale'] = np.array([r[2] for r in rows], dtype=np.float64)
    out['lrd/weight_decay'] = np.array([r[3] for r in rows], dtype=np.float64)
    out['lrd/args'] = np.array([WEIGHT_DECAY, LAYER_DECAY], dtype=np.float64)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    args = Namespace(**EPOCH_ARGS)
    opt = torch.optim.AdamW(groups, lr=args.lr)
    soft = custom_loss.SoftCrossEntropyWithWeightsLoss(weights=cw.clone())
    batches = epoch_batches(x)
    opt.zero_grad()
    losses, lrs = [], []
    for it, (samples, _, targets) in enumerate(batches):
        if it % args.accum_iter == 0:
            ref.lr_sched.adjust_learning_rate(opt, it / len(batches) + EPOCH, args)
        l = soft(model(samples), targets)
        losses.append(float(l.detach()))
        (l / args.accum_iter).backward()
        if (it + 1) % args.accum_iter == 0:
            opt.step()
            opt.zero_grad()
        lrs.append(max(g['lr'] for g in opt.param_groups))
    out['epoch/targets'] = np.stack([_np(t) for _, _, t in batches])     # batch 0: x, batch 1: x flipped along the batch
    out['epoch/losses'] = np.array(losses, dtype=np.float64)
    out['epoch/loss'] = np.array(np.mean(losses), dtype=np.float64)       # MetricLogger's global_avg
    out['epoch/lr'] = np.array(np.mean(lrs), dtype=np.float64)
    out['epoch/args'] = np.array([EPOCH_ARGS[k] for k in ('accum_iter', 'lr', 'min_lr', 'warmup_epochs', 'epochs')] + [EPOCH],
                                 dtype=np.float64)
    for n, p in model.named_parameters():
        out[f'epoch/delta/{n}'] = _np(p.detach() - before[n])
    print('epoch losses', losses, 'lr', lrs)
    return out


def main():
    path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else OUT
    out = generate()
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
