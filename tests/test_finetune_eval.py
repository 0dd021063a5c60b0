"""Fine-tuning end to end: ``evaluate()``, its metrics, Mixup and the class-weighted criteria on the HIP kernels of
csrc/classify.hip (reference post_training_utils/fine_tune_epoch.py:58-63,104-145,366-376,441-463, utils/used_metrics.py:12-41,
utils/custom_loss.py:12-18).

CPU part: the metrics against tests/golden/finetune_eval.npz (written by tools/gen_finetune_eval_golden.py from the reference's
own functions), the host side of Mixup, the ABI and drop-in surface, the refusals on CPU tensors.  GPU part: the three kernels
through the C ABI, then the criteria, ``evaluate()``, ``train_one_epoch`` with Mixup and checkpoint selection on the micro
encoder of tests/golden/vit_finetune.npz.

Bounds of ``vitae_cls_loss``: with ``loss64`` the same formula in float64 on the fp32 inputs, |loss - loss64| may be 3 x the error
of torch's own fp32 CPU evaluation of the same inputs (the margin of the norm and optimiser kernel tests), and never less than one
fp32 ulp of ``loss64``; ``dlogits`` and ``probs`` likewise row by row, in units of the row's largest term.  Every case prints its
worst ratio (observed error / allowed error); the kernel evaluates in double and rounds once, so its error is at most half an ulp
of each value.  LABNOTES.md, "vitae_cls_loss against float64", is where the observed figures are kept.
``vitae_mixup_pairs``: 4 * 2^-24 * (|lam x[i]| + |(1 - lam) x[B-1-i]|) per element — one rounding of lam, one of 1 - lam, two of the
arithmetic.  ``vitae_mixup_targets``: 2^-23 per entry, C * 2^-23 on a row sum."""
import ctypes
import os
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vit_ref as V
from oracle.gen_golden import MICRO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'finetune_eval.npz')
FINETUNE = os.path.join(ROOT, 'tests', 'golden', 'vit_finetune.npz')
FEAT = os.path.join(ROOT, 'tests', 'golden', 'vit_features.npz')
ENC = {k: MICRO[k] for k in ('volume_size', 'patch_size', 'in_chans', 'embed_dim', 'depth', 'num_heads')}
INVALID, UNSUPPORTED = -1, -2
SENTINEL = 12345.0


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD, allow_pickle=False)


@pytest.fixture(scope='module')
def finetune_gold():
    return np.load(FINETUNE, allow_pickle=False)


@pytest.fixture(scope='module')
def x_micro():
    return torch.from_numpy(np.load(FEAT, allow_pickle=False)['micro/x'])


def _same(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


# ----------------------------------------------------------------------------------------------- CPU: metrics
def test_metrics_match_the_reference_on_every_case(gold):
    from vit_ae_plus_plus_amd.utils import used_metrics as U
    assert len(gold['cases']) == 5
    for case in (str(c) for c in gold['cases']):
        logits = torch.from_numpy(gold[f'{case}/logits']).float()
        labels = torch.from_numpy(gold[f'{case}/labels'])
        ref_auc, ref_spec, ref_sens = (float(v) for v in gold[f'{case}/roc_auc'])
        auc, spec, sens = U.roc_auc(predictions=logits, target=labels)
        assert abs(auc - ref_auc) <= 1e-12, case
        assert _same(spec, ref_spec) and _same(sens, ref_sens), (case, spec, sens)
        fs, fn = U.find_vals(logits, labels)
        assert _same(fs, ref_spec) and _same(fn, ref_sens), case
        assert float(U.acc_pred(logits, labels)) == float(gold[f'{case}/acc']), case
        # the float labels evaluate() of the reference collects (torch.FloatTensor) give the same
        assert U.roc_auc(logits, labels.float())[0] == auc


def test_metrics_edge_cases():
    from vit_ae_plus_plus_amd.utils import used_metrics as U
    logits = torch.tensor([[0.5, 0.25], [0.5, 0.5], [0.0, 1.0], [2.0, 1.0]])
    for one_class in (torch.zeros(4, dtype=torch.int64), torch.ones(4, dtype=torch.int64)):
        with pytest.raises(ValueError):
            U.roc_auc(logits, one_class)
    # a tie goes to the lowest index, as torch.max: row 1 is predicted 0
    spec, sens = U.find_vals(logits, torch.tensor([0, 0, 1, 1]))
    assert (spec, sens) == (1.0, 0.5)
    # no sample of a class among the labels: 0 / 0 = NaN, as numpy gives the reference
    spec, sens = U.find_vals(logits, torch.zeros(4, dtype=torch.int64))
    assert spec == 0.75 and np.isnan(sens)
    # identical scores everywhere: every rank is tied, the AUC is 1/2
    assert U.roc_auc(torch.zeros(6, 2), torch.tensor([0, 1, 0, 1, 1, 0]))[0] == 0.5


def test_fixture_regenerates_identically(gold, tmp_path):
    from oracle import _refharness as H
    if not H.reference_available():
        pytest.skip('the reference checkout is not on this machine')
    pytest.importorskip('sklearn')             # the reference's utils/used_metrics.py imports it
    out = str(tmp_path / 'regen.npz')
    subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_finetune_eval_golden.py'), '--out', out], check=True, cwd=ROOT,
                   stdout=subprocess.DEVNULL)
    new = np.load(out, allow_pickle=False)
    assert sorted(new.files) == sorted(gold.files)
    for k in gold.files:
        assert new[k].dtype == gold[k].dtype and new[k].tobytes() == gold[k].tobytes(), k
    assert all(gold[k].dtype in (np.float64, np.int64) or gold[k].dtype.kind == 'U' for k in gold.files)
    assert os.path.getsize(GOLD) < 100 * 1024


# ----------------------------------------------------------------------------------------------- CPU: Mixup, ABI, refusals
@pytest.mark.parametrize('seed', [0, 7, 1234])
def test_mixup_draws_lam_in_timm_order(seed):
    from vit_ae_plus_plus_amd.utils.mixup import Mixup
    np.random.seed(seed)
    np.random.rand()
    expected = np.random.beta(0.1, 0.1)
    np.random.seed(seed)
    assert Mixup(mixup_alpha=0.1, num_classes=2)._params_per_batch() == expected
    np.random.seed(seed)
    assert Mixup(mixup_alpha=0.1, prob=0.0, num_classes=2)._params_per_batch() == 1.0
    assert np.random.rand() == np.random.RandomState(seed).rand(2)[1]          # exactly one draw was taken
    m = Mixup(mixup_alpha=0.1, num_classes=2)
    m.mixup_enabled = False
    assert m._params_per_batch() == 1.0


def test_mixup_refusals():
    from vit_ae_plus_plus_amd._abi import VitaeError
    from vit_ae_plus_plus_amd.utils.mixup import Mixup
    with pytest.raises(NotImplementedError):
        Mixup(mixup_alpha=0.1, cutmix_alpha=1.0, num_classes=2)
    with pytest.raises(NotImplementedError):
        Mixup(mixup_alpha=0.1, cutmix_minmax=(0.2, 0.8), num_classes=2)
    for mode in ('elem', 'pair'):
        with pytest.raises(NotImplementedError):
            Mixup(mixup_alpha=0.1, mode=mode, num_classes=2)
    with pytest.raises(VitaeError, match='no CPU fallback'):
        Mixup(mixup_alpha=0.1, num_classes=2)(torch.zeros(2, 1, 4, 4, 4), torch.tensor([0, 1]))


def test_abi_and_dropin_know_the_evaluation_surface():
    from vit_ae_plus_plus_amd import _abi, build, dropin
    dll = ctypes.CDLL(build.build(verbose=False))
    for name, nargs in (('vitae_cls_loss', 14), ('vitae_mixup_pairs', 6), ('vitae_mixup_targets', 7)):
        assert name in _abi.PROTOS and len(_abi.PROTOS[name][1]) == nargs
        assert hasattr(dll, name)
    assert _abi.PROTOS['vitae_mixup_pairs'][1][2] == 'double'                  # lam arrives as a double
    assert _abi.CONSTS['VITAE_ABI_VERSION'] >= 50
    assert 'timm' not in dropin._ALIASES and not any(k.startswith('timm.') for k in dropin._ALIASES)
    saved = {k: sys.modules.get(k) for k in dropin._ALIASES}
    try:
        dropin.install(force=True)
        import utils.mixup as mx
        import utils.used_metrics as um
        import post_training_utils.fine_tune_epoch as fte
        from utils.custom_loss import HipCrossEntropyLoss, HipSoftCrossEntropyWithWeightsLoss  # noqa: F401
        assert um.__name__ == 'vit_ae_plus_plus_amd.utils.used_metrics' and callable(um.roc_auc)
        assert mx.__name__ == 'vit_ae_plus_plus_amd.utils.mixup' and callable(mx.Mixup)
        assert all(callable(getattr(fte, n)) for n in ('evaluate', 'select_best_model', 'evaluate_best_val_model'))
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def _cfg(gp, classes=2):
    return V.VitConfig(num_classes=classes, global_pool=gp, **ENC)


def _module(cfg):
    from vit_ae_plus_plus_amd.model.vit import VisionTransformer3D
    return VisionTransformer3D(volume_size=cfg.volume_size[0], patch_size=cfg.patch_size, in_chans=cfg.in_chans,
                               num_classes=cfg.num_classes, embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads,
                               global_pool=cfg.global_pool, precision='fp32')


def test_cpu_tensors_are_refused(x_micro):
    from vit_ae_plus_plus_amd._abi import VitaeError
    from vit_ae_plus_plus_amd.post_training_utils.fine_tune_epoch import evaluate
    from vit_ae_plus_plus_amd.utils.custom_loss import HipCrossEntropyLoss, HipSoftCrossEntropyWithWeightsLoss
    with pytest.raises(VitaeError, match='no CPU fallback'):
        HipCrossEntropyLoss(torch.tensor([1.0, 2.0]))(torch.zeros(3, 2), torch.tensor([0, 1, 1]))
    with pytest.raises(VitaeError, match='no CPU fallback'):
        HipSoftCrossEntropyWithWeightsLoss(torch.tensor([1.0, 2.0]))(torch.zeros(3, 2), torch.full((3, 2), 0.5))
    with pytest.raises(VitaeError, match='no CPU fallback'):
        evaluate([(x_micro, None, torch.tensor([0, 1, 1]))], _module(_cfg(True)), torch.device('cpu'),
                 Namespace(cross_entropy_wt=torch.tensor([1.0, 2.0])))


# ----------------------------------------------------------------------------------------------- GPU: vitae_cls_loss
def _ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def _guarded(rows, cols, dtype=torch.float32):
    """[rows + 1, cols] filled with a sentinel: the kernel gets the first `rows`, the last one is the guard."""
    return torch.full((rows + 1, cols), SENTINEL if dtype.is_floating_point else 12345, dtype=dtype, device='cuda')


def _guard_ok(t):
    return bool((t[-1] == (SENTINEL if t.dtype.is_floating_point else 12345)).all())


def _formulas(x, y, t, w, dtype):
    """(loss, dlogits for g = 1, probs) of the header's formulas under autograd, in `dtype` on the CPU.  y: labels (hard mode)
    or None; t: soft targets or None.  Labels that are neither a class nor -100 make the loss NaN and zero their row."""
    x = x.to(dtype).clone().requires_grad_(True)
    w = None if w is None else w.to(dtype)
    C = x.shape[1]
    if y is not None:
        bad = (y != -100) & ((y < 0) | (y >= C))
        loss = F.cross_entropy(x, torch.where(bad, torch.full_like(y, -100), y), weight=w)
    else:
        wv = torch.ones(C, dtype=dtype) if w is None else w
        loss = ((-(t.to(dtype) * torch.log_softmax(x, dim=-1)) * wv).sum(dim=0) / wv.sum()).mean()
    if torch.isnan(loss):
        grad = torch.zeros_like(x)
    else:
        grad, = torch.autograd.grad(loss, x)
    if y is not None and bool(bad.any()):
        loss = torch.full_like(loss, float('nan'))
    return loss.detach(), grad, torch.softmax(x.detach(), dim=-1)


def _run_cls(x, ld, y, t, w, g=1.0, confusion=None, want=('dlogits', 'probs', 'pred')):
    """One vitae_cls_loss launch on a [B, ld] copy of x (padding columns poisoned); returns the outputs on the CPU."""
    from vit_ae_plus_plus_amd._abi import lib
    B, C = x.shape
    xs = torch.full((B, ld), 1e30, device='cuda')
    xs[:, :C] = x.cuda()
    loss = _guarded(1, 1)
    dl, pr = _guarded(B, C), _guarded(B, C)
    pred = _guarded(B, 1, torch.int32)
    yd = None if y is None else y.cuda()
    td = None if t is None else t.cuda().contiguous()
    wd = None if w is None else w.cuda()
    lib.vitae_cls_loss(xs.data_ptr(), ld, None if yd is None else yd.data_ptr(), None if td is None else td.data_ptr(),
                       None if wd is None else wd.data_ptr(), g, loss.data_ptr(), dl.data_ptr() if 'dlogits' in want else None,
                       pr.data_ptr() if 'probs' in want else None, pred.data_ptr() if 'pred' in want else None,
                       None if confusion is None else confusion.data_ptr(), B, C, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert _guard_ok(loss) and _guard_ok(dl) and _guard_ok(pr) and _guard_ok(pred)
    for name, buf in (('dlogits', dl), ('probs', pr), ('pred', pred)):
        if name not in want:
            assert bool((buf == buf[-1, 0]).all()), name           # an output that was not asked for is not written
    assert bool((xs[:, C:] == 1e30).all())
    return loss[0, 0].cpu(), dl[:B].cpu(), pr[:B].cpu(), pred[:B, 0].cpu()


def _check_cls(tag, x, y, t, w, ld, ratios):
    """Runs one case and holds loss, dlogits and probs to the bounds of the module docstring; returns the kernel's outputs."""
    l64, g64, p64 = _formulas(x, y, t, w, torch.float64)
    l32, g32, p32 = _formulas(x, y, t, w, torch.float32)
    loss, dl, pr, pred = _run_cls(x, ld, y, t, w)
    if torch.isnan(l64):
        assert torch.isnan(loss), tag
    else:
        assert torch.isfinite(loss), tag
        allowed = max(3 * abs(float(l32) - float(l64)), _ulp32(float(l64)))
        err = abs(float(loss.double()) - float(l64))
        ratios['loss'] = max(ratios.get('loss', 0.0), err / allowed)
        assert err <= allowed, (tag, 'loss', float(loss), float(l64), err, allowed)
    for name, got, r64, r32 in (('dlogits', dl, g64, g32), ('probs', pr, p64, p32)):
        assert bool(torch.isfinite(got).all()), (tag, name)
        unit = r64.abs().max(dim=1).values
        allowed = torch.maximum(3 * (r32.double() - r64).abs().max(dim=1).values,
                                torch.from_numpy(np.spacing(unit.float().numpy())).double())
        err = (got.double() - r64).abs().max(dim=1).values
        worst = float((err / allowed).max())
        ratios[name] = max(ratios.get(name, 0.0), worst)
        assert worst <= 1.0, (tag, name, worst, int((err / allowed).argmax()))
    assert torch.equal(pred.long(), torch.max(x, dim=1)[1]), tag
    return loss, dl, pr, pred


def _expected_confusion(x, y):
    C = x.shape[1]
    cm = torch.zeros(C, C, dtype=torch.int32)
    for p, l in zip(torch.max(x, dim=1)[1].tolist(), y.tolist()):
        if 0 <= l < C:
            cm[p, l] += 1
    return cm.reshape(-1)


# every B of {1, 2, 7, 64, 65, 300} and every C of {1, 2, 3, 5, 64, 65, 1000}: one lane, a partial wave, exactly one wave, one
# column more, 16 columns per lane; one row, fewer rows than waves, rows that do not divide by the 4 waves, > 256 rows
CLS_SHAPES = [(1, 1), (1, 2), (2, 2), (2, 3), (7, 5), (64, 2), (64, 64), (65, 65), (300, 3), (7, 1000), (300, 64), (65, 1000)]


@pytest.mark.gpu
@pytest.mark.parametrize('B,C', CLS_SHAPES)
def test_cls_loss_kernel_against_float64(B, C):
    gen = torch.Generator().manual_seed(100 * B + C)
    ratios = {}
    for hard in (True, False):
        for weighted in (False, True):
            for ld in (C, C + 3):
                x = torch.randn(B, C, generator=gen) * 3
                w = (torch.rand(C, generator=gen) + 0.25) if weighted else None
                y = torch.randint(0, C, (B,), generator=gen) if hard else None
                t = None if hard else torch.softmax(2 * torch.randn(B, C, generator=gen), dim=-1)
                tag = f'B={B} C={C} {"hard" if hard else "soft"} weighted={weighted} ld={ld}'
                loss, dl, pr, pred = _check_cls(tag, x, y, t, w, ld, ratios)
                again = _run_cls(x, ld, y, t, w)
                assert all(torch.equal(a, b) for a, b in zip((loss, dl, pr, pred), again)), tag        # bitwise reproducible
                half = _run_cls(x, ld, y, t, w, g=0.5)
                assert torch.equal(half[1], dl * 0.5), tag                                            # linear in g, bit for bit
                assert torch.equal(half[0], loss) and torch.equal(half[2], pr)
                if hard:
                    conf = _guarded(C, C, torch.int32)
                    conf[:C] = 0
                    expected = _expected_confusion(x, y)
                    for calls in (1, 2):                                                               # added to, not overwritten
                        _run_cls(x, ld, y, t, w, confusion=conf, want=())
                        assert _guard_ok(conf) and torch.equal(conf[:C].reshape(-1).cpu(), calls * expected), tag
    print(f'vitae_cls_loss B={B} C={C}: worst observed / allowed error ' + ', '.join(f'{k} {v:.3f}' for k, v in ratios.items()))


@pytest.mark.gpu
@pytest.mark.parametrize('C', [2, 5])
def test_cls_loss_kernel_failure_modes(C):
    B = 7
    gen = torch.Generator().manual_seed(C)
    x = torch.randn(B, C, generator=gen)
    x[0] = 80.0
    x[0, 0] = -80.0                      # logits of +-80
    x[1] = -80.0
    x[1, C - 1] = 80.0
    x[2, 1] += 1e4                       # one logit 1e4 above the rest
    x[3] = 0.625                         # all equal: pred 0
    w = torch.rand(C, generator=gen) + 0.5
    w[0] = 0.0                           # a class of weight 0
    y = torch.tensor([0, C - 1, 0, 1, 1, 0, C - 1])       # rows 0 and 2 pay for the wrong class: large, finite losses
    t = torch.softmax(torch.randn(B, C, generator=gen), dim=-1)
    ratios = {}
    for ld in (C, C + 3):
        for wt in (None, w):
            loss, dl, pr, pred = _check_cls(f'C={C} extreme hard', x, y, None, wt, ld, ratios)
            assert torch.isfinite(loss) and int(pred[3]) == 0 and int(pred[2]) == 1
            loss, _, _, _ = _check_cls(f'C={C} extreme soft', x, None, t, wt, ld, ratios)
            assert torch.isfinite(loss)
            # one ignored row
            yi = y.clone()
            yi[4] = -100
            loss, dl, _, _ = _check_cls(f'C={C} one ignored', x, yi, None, wt, ld, ratios)
            assert torch.isfinite(loss) and bool((dl[4] == 0).all()) and bool((dl[6] != 0).any())
            # every row ignored: NaN, as torch, and no gradient
            loss, dl, pr, _ = _check_cls(f'C={C} all ignored', x, torch.full((B,), -100), None, wt, ld, ratios)
            assert torch.isnan(loss) and bool((dl == 0).all()) and bool(torch.isfinite(pr).all())
            # labels that are no class: NaN loss, a zero row, the other rows as if the row were ignored, nothing out of range
            for wrong in (C, -1, 2 ** 40):
                yb = y.clone()
                yb[5] = wrong
                conf = _guarded(C, C, torch.int32)
                conf[:C] = 0
                loss, dl, _, _ = _check_cls(f'C={C} label {wrong}', x, yb, None, wt, ld, ratios)
                assert torch.isnan(loss) and bool((dl[5] == 0).all()) and bool((dl[6] != 0).any())
                _run_cls(x, ld, yb, None, wt, confusion=conf, want=())
                assert _guard_ok(conf) and torch.equal(conf[:C].reshape(-1).cpu(), _expected_confusion(x, yb))
                assert int(conf[:C].sum()) == B - 1
    print(f'vitae_cls_loss failure modes C={C}: worst observed / allowed error ' + ', '.join(f'{k} {v:.3f}' for k, v in ratios.items()))


@pytest.mark.gpu
def test_cls_loss_kernel_meets_the_fixture(gold):
    w = torch.from_numpy(gold['class_weights']).float()
    for case in (str(c) for c in gold['cases']):
        x = torch.from_numpy(gold[f'{case}/logits']).float()
        y = torch.from_numpy(gold[f'{case}/labels'])
        t = torch.from_numpy(gold[f'{case}/soft_targets']).float()
        for name, yy, tt in (('ce', y, None), ('soft', None, t)):
            ref = float(gold[f'{case}/{name}'])
            l32, _, _ = _formulas(x, yy, tt, w, torch.float32)
            loss, _, _, _ = _run_cls(x, 2, yy, tt, w)
            allowed = max(3 * abs(float(l32) - ref), _ulp32(ref))
            print(f'fixture {case}/{name}: {float(loss)} against {ref}, error / allowed {abs(float(loss.double()) - ref) / allowed:.3f}')
            assert abs(float(loss.double()) - ref) <= allowed, (case, name)


@pytest.mark.gpu
def test_classify_kernels_refuse_bad_arguments():
    from vit_ae_plus_plus_amd._abi import lib
    dll = lib.load()
    buf = torch.full((64,), SENTINEL, device='cuda')
    lab = torch.zeros(8, dtype=torch.int64, device='cuda')
    p, q, l = buf.data_ptr(), buf.data_ptr() + 128, lab.data_ptr()
    cls = dll.vitae_cls_loss
    assert cls(None, 2, l, None, None, 1.0, q, None, None, None, None, 4, 2, None) == INVALID
    assert cls(p, 2, l, None, None, 1.0, None, None, None, None, None, 4, 2, None) == INVALID        # the loss is not optional
    assert cls(p, 2, None, None, None, 1.0, q, None, None, None, None, 4, 2, None) == INVALID        # neither mode
    assert cls(p, 2, l, p, None, 1.0, q, None, None, None, None, 4, 2, None) == INVALID              # both modes
    assert cls(p, 1, l, None, None, 1.0, q, None, None, None, None, 4, 2, None) == INVALID           # ld < C
    assert cls(p, 2, l, None, None, 1.0, q, None, None, None, None, 0, 2, None) == INVALID
    assert cls(p, 2, l, None, None, 1.0, q, None, None, None, None, 4, 0, None) == INVALID
    assert cls(p, 2, None, p, None, 1.0, q, None, None, None, q, 4, 2, None) == INVALID              # confusion is hard mode's
    assert cls(p + 2, 2, l, None, None, 1.0, q, None, None, None, None, 4, 2, None) == INVALID       # misaligned
    assert cls(p, 1025, l, None, None, 1.0, q, None, None, None, None, 1, 1025, None) == UNSUPPORTED
    pairs = dll.vitae_mixup_pairs
    assert pairs(None, None, 0.5, 2, 4, None) == INVALID
    assert pairs(p, None, 0.5, 0, 4, None) == INVALID
    assert pairs(p, None, 0.5, 2, 0, None) == INVALID
    assert pairs(p, None, 1.5, 2, 4, None) == INVALID
    assert pairs(p, None, float('nan'), 2, 4, None) == INVALID
    assert pairs(p, p + 16, 0.5, 2, 4, None) == INVALID                                              # partial overlap
    assert pairs(p + 1, None, 0.5, 2, 4, None) == INVALID
    tg = dll.vitae_mixup_targets
    assert tg(None, p, 0.5, 0.1, 4, 2, None) == INVALID
    assert tg(l, None, 0.5, 0.1, 4, 2, None) == INVALID
    assert tg(l, p, -0.1, 0.1, 4, 2, None) == INVALID
    assert tg(l, p, 0.5, 1.5, 4, 2, None) == INVALID
    assert tg(l, p, 0.5, 0.1, 0, 2, None) == INVALID
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())                                                             # a refusal writes nothing


# ----------------------------------------------------------------------------------------------- GPU: mixup kernels
def _beta_lam():
    return float(np.random.RandomState(5).beta(0.1, 0.1))


@pytest.mark.gpu
@pytest.mark.parametrize('B', [1, 2, 3, 4, 5])
def test_mixup_pairs_kernel(B):
    from vit_ae_plus_plus_amd._abi import lib
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator().manual_seed(B)
    worst = 0.0
    for n in (1, 3, 4, 1023, 4101):
        x0 = torch.randn(B, n, generator=gen)
        for off in (0, 1):                                   # the base pointer on / one float past a 16-byte boundary
            for lam in (0.0, 1.0, 0.3, _beta_lam()):
                def buffers():
                    a = torch.full((off + (B + 1) * n,), SENTINEL, device='cuda')      # [offset | B samples | guard sample]
                    assert a.data_ptr() % 16 == 0
                    return a, a[off:off + B * n]
                xa, xv = buffers()
                xv.copy_(x0.reshape(-1))
                lib.vitae_mixup_pairs(xv.data_ptr(), None, lam, B, n, st)                            # in place
                src_a, src = buffers()
                src.copy_(x0.reshape(-1))
                da, dv = buffers()
                lib.vitae_mixup_pairs(src.data_ptr(), dv.data_ptr(), lam, B, n, st)                  # into dst
                torch.cuda.synchronize()
                tag = f'B={B} n={n} offset={off} lam={lam}'
                for a in (xa, src_a, da):
                    assert bool((a[off + B * n:] == SENTINEL).all()) and bool((a[:off] == SENTINEL).all()), tag
                got, got_dst = xv.cpu().view(B, n), dv.cpu().view(B, n)
                assert torch.equal(src.cpu().view(B, n), x0), tag                                    # the source is left alone
                assert torch.equal(got, got_dst), tag                                                # the same, bit for bit
                a64, b64 = lam * x0.double(), (1 - lam) * x0.flip(0).double()
                bound = 4 * 2.0 ** -24 * (a64.abs() + b64.abs())
                err = (got.double() - (a64 + b64)).abs()
                assert bool((err <= bound).all()), (tag, float((err / bound.clamp_min(1e-300)).max()))
                worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
                if lam == 1.0:
                    assert torch.equal(got, x0), tag
                if B % 2:
                    assert torch.equal(got[B // 2], x0[B // 2]), tag
    print(f'vitae_mixup_pairs B={B}: worst error / bound {worst:.3f}')


@pytest.mark.gpu
def test_mixup_targets_kernel():
    from vit_ae_plus_plus_amd._abi import lib
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator().manual_seed(3)

    def run(y, lam, s, C):
        B = y.shape[0]
        out = _guarded(B, C)
        lib.vitae_mixup_targets(y.cuda().data_ptr(), out.data_ptr(), lam, s, B, C, st)
        torch.cuda.synchronize()
        assert _guard_ok(out)
        return out[:B].cpu()

    def formula(y, lam, s, C):
        off = s / C
        oh = lambda v: torch.full((v.shape[0], C), off, dtype=torch.float64).scatter_(1, v.view(-1, 1), 1.0 - s + off)
        return lam * oh(y) + (1 - lam) * oh(y.flip(0))

    for C in (2, 5):
        for B in (1, 4, 5):
            for s in (0.0, 0.1):
                for lam in (0.0, 1.0, 0.3, _beta_lam()):
                    y = torch.randint(0, C, (B,), generator=gen)
                    got, ref = run(y, lam, s, C), formula(y, lam, s, C)
                    assert float((got.double() - ref).abs().max()) <= 2.0 ** -23, (C, B, s, lam)
                    assert float((got.double().sum(dim=1) - 1).abs().max()) <= C * 2.0 ** -23, (C, B, s, lam)
    # a label that is no class: the rows that depend on it are NaN, the others right
    for B, k, nan_rows in ((5, 2, {2}), (4, 1, {1, 2}), (5, 0, {0, 4})):
        for wrong in (5, -1, 2 ** 40):
            y = torch.randint(0, 5, (B,), generator=gen)
            good = formula(y, 0.3, 0.1, 5)
            y[k] = wrong
            got = run(y, 0.3, 0.1, 5)
            for r in range(B):
                if r in nan_rows:
                    assert bool(torch.isnan(got[r]).all()), (B, k, r)
                else:
                    assert float((got[r].double() - good[r]).abs().max()) <= 2.0 ** -23, (B, k, r)


# ----------------------------------------------------------------------------------------------- GPU: end to end
def _micro(gp, classes=2):
    cfg = _cfg(gp, classes)
    m = _module(cfg).cuda().train()
    m.load_state_dict(V.init_vit_state_dict(cfg, seed=5))
    return m


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _without_key_bias(m, name, a):
    """The key third of attn.qkv.bias has no gradient in exact arithmetic (softmax ignores a shift common to all keys): what it
    holds is rounding noise that no two implementations share — test_finetune_epoch_soft_targets_accumulation has the figures."""
    D = m.embed_dim
    return np.delete(a, np.s_[D:2 * D]) if name.endswith('attn.qkv.bias') else a


def _five_samples(x_micro):
    x = torch.cat((x_micro, (x_micro.flip(0) * 0.5 + 0.1)))[:5].contiguous()
    return x, torch.tensor([0, 1, 1, 0, 1])


def _loader(x, y, bs=2):
    return [(x[i:i + bs], None, y[i:i + bs]) for i in range(0, x.shape[0], bs)]


@pytest.mark.gpu
@pytest.mark.parametrize('gp', [False, True])
def test_hip_criteria_match_torch_on_the_model(finetune_gold, x_micro, gp):
    from vit_ae_plus_plus_amd._abi import VitaeError
    from vit_ae_plus_plus_amd.utils.custom_loss import (HipCrossEntropyLoss, HipSoftCrossEntropyWithWeightsLoss,
                                                        SoftCrossEntropyWithWeightsLoss)
    w = torch.from_numpy(finetune_gold['class_weights'])
    x = x_micro.cuda()
    hard = torch.from_numpy(finetune_gold['labels']).cuda()
    soft = torch.from_numpy(finetune_gold['epoch/targets'][0]).cuda()
    pairs = ((HipCrossEntropyLoss(w).cuda(), torch.nn.CrossEntropyLoss(weight=w).cuda(), hard),
             (HipSoftCrossEntropyWithWeightsLoss(w).cuda(), SoftCrossEntropyWithWeightsLoss(w).cuda(), soft))
    for hip, ref, target in pairs:
        out = []
        for crit in (hip, ref):
            m = _micro(gp, classes=3)
            loss = crit(m(x), target)
            assert loss.shape == () and loss.dtype == torch.float32
            loss.backward()
            torch.cuda.synchronize()
            out.append((float(loss.detach()), m, {n: p.grad.detach().cpu().numpy() for n, p in m.named_parameters()}))
        (l_hip, m, g_hip), (l_ref, _, g_ref) = out
        print(f'{type(hip).__name__} {"gp" if gp else "cls"}: loss {l_hip} against torch {l_ref}')
        assert abs(l_hip - l_ref) <= 1e-6 * abs(l_ref)
        worst = max((_rel(_without_key_bias(m, n, g_hip[n]), _without_key_bias(m, n, g_ref[n])), n) for n in g_ref)
        print(f'  worst gradient relative L2 difference {worst[0]:.3e} ({worst[1]})')
        assert worst[0] <= 1e-5, worst
        # the incoming gradient scales it; a second backward is refused
        m = _micro(gp, classes=3)
        loss = hip(m(x), target)
        (loss * 0.25).backward()
        for n, p in m.named_parameters():
            assert _rel(_without_key_bias(m, n, p.grad.cpu().numpy()), _without_key_bias(m, n, 0.25 * g_hip[n])) <= 1e-5, n
        with pytest.raises(VitaeError):
            loss.backward()
        torch.cuda.synchronize()
    # without a gradient to compute, the forward alone
    with torch.no_grad():
        m = _micro(gp, classes=3)
        assert abs(float(pairs[0][0](m(x), hard)) - float(pairs[0][1](m(x), hard))) <= 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize('gp', [False, True])
def test_evaluate_five_samples_in_batches_of_two(x_micro, gp):
    from vit_ae_plus_plus_amd.post_training_utils.fine_tune_epoch import evaluate
    from vit_ae_plus_plus_amd.utils import used_metrics as U
    x, y = _five_samples(x_micro)
    w = torch.tensor([1.0, 2.5])
    args = Namespace(cross_entropy_wt=w)
    m = _micro(gp)
    marker = torch.full_like(m.head.bias, 3.0)
    m.head.bias.grad = marker.clone()
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    seen = []
    hook = m.register_forward_hook(lambda mod, inp, out: seen.append(out.detach().clone()))
    stats = evaluate(_loader(x, y), m, torch.device('cuda'), args)
    hook.remove()
    assert sorted(stats) == ['loss', 'roc_auc_score', 'sensitivity', 'specificity']
    assert [tuple(s.shape) for s in seen] == [(2, 2), (2, 2), (1, 2)]               # drop_last=False: the last batch is one sample
    assert not m.training                                                           # left in eval mode, as the reference
    with torch.no_grad():
        full = m(x.cuda()).cpu()
    logits = torch.cat(seen).cpu()
    assert float((logits - full).abs().max()) <= 1e-5 * float(full.abs().max())
    batch_losses = [float(F.cross_entropy(s.cpu().double(), yb, weight=w.double())) for s, (_, _, yb) in zip(seen, _loader(x, y))]
    print(f'evaluate {"gp" if gp else "cls"}: {stats}, batch losses {batch_losses}')
    assert abs(stats['loss'] - float(np.mean(batch_losses))) <= 1e-6 * abs(float(np.mean(batch_losses)))
    auc, spec, sens = U.roc_auc(logits, y)
    assert abs(stats['roc_auc_score'] - auc) <= 1e-12
    assert _same(stats['specificity'], spec) and _same(stats['sensitivity'], sens)
    for n, p in m.named_parameters():
        assert torch.equal(p.detach(), before[n]), n
        assert (torch.equal(p.grad, marker) if n == 'head.bias' else p.grad is None), n
    assert evaluate(_loader(x, y), m, torch.device('cuda'), args) == stats
    # no class weights, one sample per batch
    stats1 = evaluate(_loader(x, y, bs=1), m, torch.device('cuda'), Namespace(cross_entropy_wt=None))
    ref1 = float(np.mean([float(F.cross_entropy(full[i:i + 1].double(), y[i:i + 1])) for i in range(5)]))
    # cross entropy moves by at most twice the largest change of a logit, and the logits were held to 1e-5 of the largest above
    assert abs(stats1['loss'] - ref1) <= 2e-5 * float(full.abs().max()) and abs(stats1['roc_auc_score'] - auc) <= 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize('gp', [False, True])
def test_finetune_epoch_with_mixup_and_hip_criterion(x_micro, gp):
    from vit_ae_plus_plus_amd.post_training_utils.fine_tune_epoch import train_one_epoch
    from vit_ae_plus_plus_amd.utils.custom_loss import HipSoftCrossEntropyWithWeightsLoss, SoftCrossEntropyWithWeightsLoss
    from vit_ae_plus_plus_amd.utils.misc import NativeScalerWithGradNormCount
    from vit_ae_plus_plus_amd.utils.mixup import Mixup
    w = torch.tensor([1.0, 2.5])
    args = Namespace(accum_iter=2, lr=0.5, min_lr=0.0, warmup_epochs=0, epochs=4)
    batches = [(x_micro, None, torch.tensor([0, 1, 1])), ((x_micro.flip(0) * 0.5 + 0.1).contiguous(), None, torch.tensor([1, 1, 0]))]
    smoothing, classes, lams = 0.1, 2, []

    def torch_mixup(x, target):
        """timm's batch mode written out: the draws, the three-op mix, the smoothed one-hot rows."""
        lam = 1.0
        if np.random.rand() < 1.0:
            lam = float(np.random.beta(0.1, 0.1))
        lams.append(lam)
        flipped = x.flip(0).mul_(1.0 - lam)
        x.mul_(lam).add_(flipped)
        off, on = smoothing / classes, 1.0 - smoothing + smoothing / classes
        oh = lambda v: torch.full((v.shape[0], classes), off, device=v.device).scatter_(1, v.view(-1, 1), on)
        return x, oh(target) * lam + oh(target.flip(0)) * (1.0 - lam)

    def run(criterion, mix):
        np.random.seed(11)
        m = _micro(gp)
        before = {n: p.detach().cpu().clone() for n, p in m.named_parameters()}
        opt = torch.optim.SGD(m.parameters(), lr=args.lr)
        stats = train_one_epoch(m, criterion.cuda(), batches, opt, torch.device('cuda'), 0, NativeScalerWithGradNormCount(),
                                max_norm=None, args=args, mix_up_fn=mix)
        return stats, m, {n: (p.detach().cpu() - before[n]).numpy() for n, p in m.named_parameters()}

    mix = Mixup(mixup_alpha=0.1, num_classes=classes)
    s_hip, m, d_hip = run(HipSoftCrossEntropyWithWeightsLoss(w), mix)
    s_ref, _, d_ref = run(SoftCrossEntropyWithWeightsLoss(w), torch_mixup)
    assert mix.last_lam == lams[-1] and len(lams) == 2                              # the same numpy stream, the same ratios
    print(f'mixup epoch {"gp" if gp else "cls"}: lam {lams}, loss {s_hip["loss"]} against {s_ref["loss"]}')
    assert abs(s_hip['loss'] - s_ref['loss']) <= 1e-5 * abs(s_ref['loss'])
    assert s_hip['lr'] == s_ref['lr']
    worst = max((_rel(_without_key_bias(m, n, d_hip[n]), _without_key_bias(m, n, d_ref[n])), n) for n in d_ref)
    print(f'  worst parameter-delta relative L2 difference {worst[0]:.3e} ({worst[1]})')
    assert all(np.linalg.norm(d) > 0 for d in d_ref.values())
    assert worst[0] <= 1e-4, worst


@pytest.mark.gpu
def test_checkpoint_selection_round_trip(x_micro, tmp_path):
    from vit_ae_plus_plus_amd.post_training_utils.fine_tune_epoch import evaluate, evaluate_best_val_model, select_best_model
    from vit_ae_plus_plus_amd.utils.misc import NativeScalerWithGradNormCount
    x, y = _five_samples(x_micro)
    loader = _loader(x, y)
    args = Namespace(cross_entropy_wt=torch.tensor([1.0, 2.5]), output_dir=str(tmp_path), eval_model_path=str(tmp_path))
    dev = torch.device('cuda')
    m = _micro(True)
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    scaler = NativeScalerWithGradNormCount()
    saved = evaluate(loader, m, dev, args)
    best = select_best_model(args=args, epoch=0, loss_scaler=scaler, max_val=-1.0, model=m, model_without_ddp=m, optimizer=opt,
                             cur_val=saved['roc_auc_score'], model_name='best_ft_model')
    assert best == saved['roc_auc_score'] and os.path.exists(tmp_path / 'checkpoint-best_ft_model.pth')
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(-0.5)
    changed = evaluate(loader, m, dev, args)
    assert changed['loss'] != saved['loss']
    # a value that is no better saves nothing
    assert select_best_model(args=args, epoch=1, loss_scaler=scaler, max_val=best, model=m, model_without_ddp=m, optimizer=opt,
                             cur_val=best, model_name='best_ft_model') == best
    for mode in (None, 'test'):
        with torch.no_grad():
            m.head.bias.add_(1.0)
        assert evaluate_best_val_model(args, loader, list(range(5)), dev, m, model_name='best_ft_model', mode=mode) == saved['roc_auc_score']
        assert evaluate(loader, m, dev, args) == saved
