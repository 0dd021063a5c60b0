"""Writes tests/golden/finetune_eval.npz: what the REFERENCE's own metrics and criteria return on small logit sets (build
container only: needs the reference checkout, see oracle/_refharness.py, and scikit-learn, which the reference's
utils/used_metrics.py imports).

    python tools/gen_finetune_eval_golden.py [--out other.npz]

Recorded results only, float64 / int64:

    cases                                   names of the metric cases
    <case>/logits [n, 2], <case>/labels     scores rounded to quarters (so ties occur) and two-class labels; n in {2, 3, 37, 130},
                                            plus ``onesided``: every argmax is class 1 while the labels have both classes
    <case>/roc_auc                          [auc, specificity, sensitivity] of the reference's utils.used_metrics.roc_auc
    <case>/acc                              utils.used_metrics.acc_pred
    class_weights                           the weights of the two criteria below
    <case>/ce                               torch.nn.functional.cross_entropy(logits, labels, weight) evaluated in float64
    <case>/soft_targets [n, 2], <case>/soft the reference's SoftCrossEntropyWithWeightsLoss (utils/custom_loss.py:12-18) on
                                            those targets, evaluated in float64
"""
import contextlib
import importlib
import io
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import _refharness as H          # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'finetune_eval.npz')
CLASS_WEIGHTS = [1.0, 2.5]
SIZES = (2, 3, 37, 130)


def _reference_modules():
    ref = H.import_reference()
    if 'timm.loss' not in sys.modules:          # utils/custom_loss.py imports it for a self-check only
        m = types.ModuleType('timm.loss')
        m.SoftTargetCrossEntropy = type('SoftTargetCrossEntropy', (torch.nn.Module,), {})
        sys.modules['timm.loss'] = m
    utils_pkg = sys.modules[ref.lr_sched.__name__.rsplit('.', 1)[0]]
    assert os.path.dirname(utils_pkg.__file__).startswith(H.REFERENCE_ROOT), utils_pkg.__file__
    return importlib.import_module('utils.used_metrics'), importlib.import_module('utils.custom_loss')


def cases():
    """name -> (logits fp32 [n, 2], labels int64 [n])"""
    g = torch.Generator().manual_seed(41)
    out = {}
    for n in SIZES:
        logits = (torch.randn(n, 2, generator=g) * 1.5 * 4).round() / 4
        labels = (torch.rand(n, generator=g) < 0.4).long()
        labels[0], labels[-1] = 0, 1            # both classes, whatever the draw
        out[f'n{n}'] = (logits, labels)
    logits = (torch.randn(9, 2, generator=g) * 4).round() / 4
    logits[:, 1] = logits[:, 0] + 0.25 + logits[:, 1].abs()       # every argmax is class 1
    out['onesided'] = (logits, torch.tensor([0, 1, 1, 0, 1, 0, 0, 1, 1]))
    return out


def generate():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    used_metrics, custom_loss = _reference_modules()
    cw = torch.tensor(CLASS_WEIGHTS, dtype=torch.float64)
    soft = custom_loss.SoftCrossEntropyWithWeightsLoss(weights=cw.clone())
    g = torch.Generator().manual_seed(43)
    out = {'class_weights': cw.numpy().copy(), 'cases': np.array(list(cases().keys()))}
    for name, (logits, labels) in cases().items():
        with contextlib.redirect_stdout(io.StringIO()), np.errstate(divide='ignore', invalid='ignore'):     # its debugging prints
            auc, spec, sens = used_metrics.roc_auc(predictions=logits, target=labels)
            acc = used_metrics.acc_pred(logits, labels)
        out[f'{name}/logits'] = logits.double().numpy()
        out[f'{name}/labels'] = labels.numpy().astype(np.int64)
        out[f'{name}/roc_auc'] = np.array([auc, spec, sens], dtype=np.float64)
        out[f'{name}/acc'] = np.array(float(acc), dtype=np.float64)
        out[f'{name}/ce'] = np.array(float(torch.nn.functional.cross_entropy(logits.double(), labels, weight=cw)), dtype=np.float64)
        lam = torch.rand(logits.shape[0], 1, generator=g, dtype=torch.float64)
        t = lam * torch.nn.functional.one_hot(labels, 2) + (1 - lam) * torch.nn.functional.one_hot(labels.flip(0), 2)
        t = t.float().double()                  # fp32-representable, as the kernel reads them
        out[f'{name}/soft_targets'] = t.numpy()
        out[f'{name}/soft'] = np.array(float(soft(logits.double(), t)), dtype=np.float64)
        print(name, 'roc_auc', out[f'{name}/roc_auc'], 'acc', float(acc), 'ce', float(out[f'{name}/ce']), 'soft', float(out[f'{name}/soft']))
    return out


def main():
    path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else OUT
    out = generate()
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
