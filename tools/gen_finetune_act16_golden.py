"""Writes tests/golden/vit_finetune_act16.npz: what the REFERENCE's own VisionTransformer3D computes when it is fine-tuned on two
micro configurations that the bf16-activation training route accepts (build container only: needs the reference checkout, see
oracle/_refharness.py).

    python tools/gen_finetune_act16_golden.py [--out other.npz]

The route needs embed_dim, the MLP hidden size and in_chans * patch^3 to be multiples of 64 and a head size of 32 or 64, which the
micro encoder of vit_finetune.npz (embed 48, head size 16) is not.  Both configurations: 16^3 volumes, patch 4, 1 channel
(P = 64), embed 64, depth 2, 3 classes; ``h32``: 2 heads of 32, ``h64``: 1 head of 64.  Batch 3: M = 3 * 65 = 195 token rows
(padded to 256 by the route), N = 65 tokens — one past a 64-row tile.  Weights ``oracle.vit_ref.init_vit_state_dict(cfg, seed=5)``,
input ``oracle.mae_ref.synthetic_views((3, 1, 16, 16, 16), seed=77)[0]`` (stored as ``x``), labels [0, 2, 1], class weights
[1, 2, 0.5] as in vit_finetune.npz.  Per configuration and pooling mode (``<cfg>/cls`` / ``<cfg>/gp``; the ``PAIRS`` below):

    <p>/loss, <p>/logits, <p>/names, <p>/grad/<name>     cross_entropy(weight) forward + backward in fp32
    <p>/adamw_losses                                     4 steps of torch.optim.AdamW(lr=1e-3, weight_decay=0.05)
    <p>/bf16_ref_relerr/<name>                           the reference's own loss of precision under
    <p>/bf16_ref_logits_err                              torch.autocast('cpu', bfloat16): relative L2 error of each gradient, max-abs
    <p>/bf16_ref_adamw_dev                               error of the logits, |loss - fp32 loss| of each of the 4 AdamW steps

The tool asserts that every fp32 gradient norm and every ``bf16_ref_relerr`` is > 0.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import _refharness as H          # noqa: E402
from oracle import mae_ref as R              # noqa: E402
from oracle import vit_ref as V              # noqa: E402
from oracle.gen_golden import _build_reference_vit, _np, load_into_reference   # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'vit_finetune_act16.npz')
ENC = dict(volume_size=(16, 16, 16), patch_size=4, in_chans=1, embed_dim=64, depth=2)
HEADS = {'h32': 2, 'h64': 1}
# (configuration, global_pool).  One pair holds 0.43 MB of fp32 gradients, which do not compress, and a file committed to this project
# may hold 1 MiB (tools/README.md): three pairs are 1.32 MB, two are 0.90 MB.  Kept: both head sizes and both pooling modes, once each.  tests/test_vit_finetune_act16.py takes the other two pairs
# (h32/gp, h64/cls) from the oracle, after showing on these two that the oracle reproduces every stored quantity.
PAIRS = [('h32', False), ('h64', True)]
LABELS = [0, 2, 1]
CLASS_WEIGHTS = [1.0, 2.0, 0.5]
X_SHAPE, X_SEED = (3, 1, 16, 16, 16), 77


def config(name, gp):
    return V.VitConfig(num_classes=3, global_pool=gp, num_heads=HEADS[name], **ENC)


def _model(ref, cfg):
    model = _build_reference_vit(ref, cfg)
    load_into_reference(model, V.init_vit_state_dict(cfg, seed=5))
    return model.train()


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def _step(model, x, y, ce, bf16):
    if bf16:
        with torch.autocast('cpu', dtype=torch.bfloat16):
            logits = model(x)
            loss = ce(logits, y)
    else:
        logits = model(x)
        loss = ce(logits, y)
    loss.backward()
    return loss.detach().float(), logits.detach().float()


def _adamw(ref, cfg, x, y, ce, bf16):
    model = _model(ref, cfg)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=0.05)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        losses.append(float(_step(model, x, y, ce, bf16)[0]))
        opt.step()
    return np.array(losses, dtype=np.float64)


def generate():
    torch.manual_seed(0)
    torch.set_num_threads(1)      # one summation order whatever the machine's core count: the fixture regenerates byte for byte
    ref = H.import_reference()
    x = R.synthetic_views(X_SHAPE, seed=X_SEED)[0]
    y = torch.tensor(LABELS)
    ce = torch.nn.CrossEntropyLoss(weight=torch.tensor(CLASS_WEIGHTS))
    out = {'x': _np(x), 'labels': np.array(LABELS, dtype=np.int64), 'class_weights': np.array(CLASS_WEIGHTS, dtype=np.float32),
           'pairs': np.array([f'{name}/{"gp" if gp else "cls"}' for name, gp in PAIRS])}
    for name, gp in PAIRS:
        p = f'{name}/{"gp" if gp else "cls"}'
        cfg = config(name, gp)
        model = _model(ref, cfg)
        loss, logits = _step(model, x, y, ce, False)
        g32 = _grads(model)
        names = list(g32.keys())
        out[f'{p}/names'] = np.array(names)
        out[f'{p}/loss'] = _np(loss)
        out[f'{p}/logits'] = _np(logits)
        for n in names:
            assert float(g32[n].norm()) > 0, n
            out[f'{p}/grad/{n}'] = _np(g32[n])
        # the reference's own loss of precision under bf16 autocast
        model = _model(ref, cfg)
        _, logits16 = _step(model, x, y, ce, True)
        g16 = _grads(model)
        for n in names:
            e = (g16[n].float() - g32[n]).norm() / g32[n].norm()
            assert float(e) > 0, n
            out[f'{p}/bf16_ref_relerr/{n}'] = _np(e)
        out[f'{p}/bf16_ref_logits_err'] = _np((logits16 - logits).abs().max())
        # 4 steps of AdamW on the same batch, fp32 and under autocast
        out[f'{p}/adamw_losses'] = _adamw(ref, cfg, x, y, ce, False)
        out[f'{p}/bf16_ref_adamw_dev'] = np.abs(_adamw(ref, cfg, x, y, ce, True) - out[f'{p}/adamw_losses'])
        rel = [float(out[f'{p}/bf16_ref_relerr/{n}']) for n in names]
        print(p, 'loss', float(loss), 'adamw', list(out[f'{p}/adamw_losses']), 'bf16: relerr %.4f..%.4f' % (min(rel), max(rel)),
              'logits %.3g' % float(out[f'{p}/bf16_ref_logits_err']), 'adamw dev', list(out[f'{p}/bf16_ref_adamw_dev']),
              'min |grad| %.3g' % min(float(g32[n].norm()) for n in names))
    return out


def main():
    path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else OUT
    out = generate()
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
