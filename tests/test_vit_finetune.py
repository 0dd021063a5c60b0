"""Fine-tuning VisionTransformer3D on the HIP kernels (reference model/vit.py:265-297 differentiated,
post_training_utils/fine_tune_epoch.py:34-100, utils/lr_decay.py:15-75).

The expectations come from tests/golden/vit_finetune.npz, written by tools/gen_finetune_golden.py from the reference's own
VisionTransformer3D.  CPU part: the oracle restatement reproduces the fixture under autograd (so GPU tests on a machine
without the reference have an independent expectation), the layer-decay groups, the ABI and the drop-in aliases.  GPU part:
the two new kernels and the training path against the fixture.

Bounds: 1e-4 (relative L2 per gradient, relative on losses) is the project's fp32 parity bound (BASELINE north star) and
holds for fp32x3 as well; bf16 gradients may lose at most twice what the reference itself loses under bf16 autocast on the
same weights (``bf16_ref_relerr`` in the fixture).  1e-6 where two runs of the same arithmetic differ only by the order of
float atomics (LayerNorm / bias column sums)."""
import os
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

from oracle import mae_ref as R
from oracle import vit_ref as V
from oracle.gen_golden import MICRO, VITB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'vit_finetune.npz')
FEAT = os.path.join(ROOT, 'tests', 'golden', 'vit_features.npz')
ENC = {k: MICRO[k] for k in ('volume_size', 'patch_size', 'in_chans', 'embed_dim', 'depth', 'num_heads')}
TAGS = {False: 'cls', True: 'gp'}


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD, allow_pickle=False)


@pytest.fixture(scope='module')
def x_micro():
    return torch.from_numpy(np.load(FEAT, allow_pickle=False)['micro/x'])


def _cfg(gp):
    return V.VitConfig(num_classes=3, global_pool=gp, **ENC)


def _module(cfg, precision='fp32', **kw):
    from vit_ae_plus_plus_amd.model.vit import VisionTransformer3D
    return VisionTransformer3D(volume_size=cfg.volume_size[0], patch_size=cfg.patch_size, in_chans=cfg.in_chans,
                               num_classes=cfg.num_classes, embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads,
                               global_pool=cfg.global_pool, precision=precision, **kw)


def _micro(gp, precision='fp32', **kw):
    cfg = _cfg(gp)
    m = _module(cfg, precision, **kw).cuda().train()
    m.load_state_dict(V.init_vit_state_dict(cfg, seed=5))
    return m


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _criterion(gold, device='cpu'):
    return torch.nn.CrossEntropyLoss(weight=torch.from_numpy(gold['class_weights']).to(device))


def _grads(m):
    return {n: (None if p.grad is None else p.grad.detach().cpu().numpy()) for n, p in m.named_parameters()}


# ----------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize('gp', [False, True])
def test_oracle_autograd_matches_reference_gradients(gold, x_micro, gp):
    tag, cfg = TAGS[gp], _cfg(gp)
    sd = {k: v.clone().requires_grad_(True) for k, v in V.init_vit_state_dict(cfg, seed=5).items()}
    logits = V.forward(sd, x_micro, cfg)
    loss = _criterion(gold)(logits, torch.from_numpy(gold['labels']))
    loss.backward()
    assert list(gold[f'{tag}/names']) == list(sd.keys())
    assert abs(float(loss.detach()) - float(gold[f"{tag}/loss"])) <= 1e-6 * abs(float(gold[f'{tag}/loss']))
    assert np.allclose(logits.detach().numpy(), gold[f'{tag}/logits'], atol=2e-6)
    for n, p in sd.items():
        ref = gold[f'{tag}/grad/{n}']
        assert np.linalg.norm(ref) > 0, n
        assert _rel(p.grad.numpy(), ref) <= 1e-6, n


def test_param_groups_lrd_table(gold):
    from vit_ae_plus_plus_amd.utils.lr_decay import get_layer_id_for_vit, param_groups_lrd
    m = _module(_cfg(True))
    wd, ld = (float(v) for v in gold['lrd/args'])
    groups = param_groups_lrd(m, wd, no_weight_decay_list=m.no_weight_decay(), layer_decay=ld)
    name_of = {id(p): n for n, p in m.named_parameters()}
    rows = [(name_of[id(p)], gi, g['lr_scale'], g['weight_decay']) for gi, g in enumerate(groups) for p in g['params']]
    assert [r[0] for r in rows] == [str(n) for n in gold['lrd/names']]
    assert [r[1] for r in rows] == [int(v) for v in gold['lrd/group']]
    assert np.array_equal(np.array([r[2] for r in rows]), gold['lrd/lr_scale'])
    assert np.array_equal(np.array([r[3] for r in rows]), gold['lrd/weight_decay'])
    assert sorted(r[0] for r in rows) == sorted(name_of.values())          # every parameter is in exactly one group
    n_layers = len(m.blocks) + 1
    assert [get_layer_id_for_vit(n, n_layers) for n in ('cls_token', 'pos_embed', 'patch_embed.proj.bias', 'blocks.1.norm1.weight',
                                                        'fc_norm.weight', 'head.bias')] == [0, 0, 0, 2, 3, 3]
    # frozen parameters are left out
    for n, p in m.named_parameters():
        p.requires_grad = n.startswith(('head.', 'blocks.1.'))
    kept = [name_of[id(p)] for g in param_groups_lrd(m, wd, m.no_weight_decay(), ld) for p in g['params']]
    assert sorted(kept) == sorted(n for n in name_of.values() if n.startswith(('head.', 'blocks.1.')))


def test_abi_and_dropin_know_the_finetune_surface():
    import ctypes
    from vit_ae_plus_plus_amd import _abi, build, dropin
    dll = ctypes.CDLL(build.build(verbose=False))
    for name, nargs in (('vitae_vit_assemble_bwd', 10), ('vitae_token_select_bwd', 7)):
        assert name in _abi.PROTOS and len(_abi.PROTOS[name][1]) == nargs
        assert hasattr(dll, name)
    assert _abi.CONSTS['VITAE_ABI_VERSION'] >= 49
    saved = {k: sys.modules.get(k) for k in dropin._ALIASES}
    try:
        dropin.install(force=True)
        import post_training_utils.fine_tune_epoch as fte
        import utils.lr_decay as lrd
        assert lrd.__name__ == 'vit_ae_plus_plus_amd.utils.lr_decay' and callable(lrd.param_groups_lrd)
        assert fte.__name__ == 'vit_ae_plus_plus_amd.post_training_utils.fine_tune_epoch' and callable(fte.train_one_epoch)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_fixture_regenerates_identically(gold, tmp_path):
    from oracle import _refharness as H
    if not H.reference_available():
        pytest.skip('the reference checkout is not on this machine')
    out = str(tmp_path / 'regen.npz')
    subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_finetune_golden.py'), '--out', out], check=True, cwd=ROOT,
                   stdout=subprocess.DEVNULL)
    new = np.load(out, allow_pickle=False)
    assert sorted(new.files) == sorted(gold.files)
    for k in gold.files:
        assert new[k].dtype == gold[k].dtype and new[k].tobytes() == gold[k].tobytes(), k


# ----------------------------------------------------------------------------------------------- GPU: kernels
SHAPES = [(3, 64, 48), (4, 216, 768), (2, 512, 1024)]


@pytest.mark.gpu
@pytest.mark.parametrize('B,L,D', SHAPES)
@pytest.mark.parametrize('accumulate', [0, 1])
def test_vit_assemble_bwd_kernel(B, L, D, accumulate):
    from vit_ae_plus_plus_amd._abi import lib
    g = torch.Generator().manual_seed(B * 1000 + L)
    dx = torch.randn(B, L + 1, D, generator=g)
    # torch autograd of the reference expression (model/vit.py:269-272)
    tok = torch.randn(B, L, D, generator=g, requires_grad=True)
    cls = torch.randn(1, 1, D, generator=g, requires_grad=True)
    pos = torch.randn(1, L + 1, D, generator=g, requires_grad=True)
    (torch.cat((cls.expand(B, -1, -1), tok), dim=1) + pos).backward(dx)
    pos0, cls0 = torch.randn(L + 1, D, generator=g), torch.randn(D, generator=g)
    st = torch.cuda.current_stream().cuda_stream

    def run():
        dtok = torch.full((B * L, D), float('nan'), device='cuda')
        dtok16 = torch.zeros(B * L, D, dtype=torch.bfloat16, device='cuda')
        dpos, dcls = pos0.cuda(), cls0.cuda()
        lib.vitae_vit_assemble_bwd(dx.cuda().data_ptr(), dtok.data_ptr(), dtok16.data_ptr(), dpos.data_ptr(), dcls.data_ptr(),
                                   B, L, D, accumulate, st)
        torch.cuda.synchronize()
        return dtok.cpu(), dtok16.cpu(), dpos.cpu(), dcls.cpu()

    dtok, dtok16, dpos, dcls = run()
    assert torch.equal(dtok.view(B, L, D), tok.grad)
    assert torch.equal(dtok16.view(B, L, D), tok.grad.to(torch.bfloat16))
    ref_pos = pos.grad[0] + (pos0 if accumulate else 0)
    ref_cls = cls.grad[0, 0] + (cls0 if accumulate else 0)
    # sums over at most 4 samples of unit-variance values: a few fp32 roundings of O(1) numbers
    assert torch.allclose(dpos, ref_pos, rtol=1e-6, atol=4e-6) and torch.allclose(dcls, ref_cls, rtol=1e-6, atol=4e-6)
    again = run()
    assert all(torch.equal(a, b) for a, b in zip((dtok, dtok16, dpos, dcls), again))      # bitwise reproducible
    # outputs are optional one by one
    dpos2 = torch.zeros(L + 1, D, device='cuda')
    lib.vitae_vit_assemble_bwd(dx.cuda().data_ptr(), None, None, dpos2.data_ptr(), None, B, L, D, 0, st)
    torch.cuda.synchronize()
    assert torch.allclose(dpos2.cpu(), pos.grad[0], rtol=1e-6, atol=4e-6)


@pytest.mark.gpu
@pytest.mark.parametrize('B,L,D', SHAPES)
@pytest.mark.parametrize('mode', [0, 1])
def test_token_select_bwd_kernel(B, L, D, mode):
    from vit_ae_plus_plus_amd._abi import lib
    N = L + 1
    g = torch.Generator().manual_seed(B * 1000 + L + mode)
    dsel = torch.randn(B, D, generator=g)
    x = torch.randn(B, N, D, generator=g, requires_grad=True)
    (x[:, 1:, :].mean(dim=1) if mode else x[:, 0]).backward(dsel)      # model/vit.py:277-282
    st = torch.cuda.current_stream().cuda_stream

    def run():
        dx = torch.full((B, N, D), float('nan'), device='cuda')          # every element must be written
        lib.vitae_token_select_bwd(dsel.cuda().data_ptr(), dx.data_ptr(), B, N, D, mode, st)
        torch.cuda.synchronize()
        return dx.cpu()

    dx = run()
    assert torch.allclose(dx, x.grad, rtol=1e-6, atol=0)
    assert torch.equal(dx, run())


@pytest.mark.gpu
def test_new_kernels_reject_bad_arguments():
    from vit_ae_plus_plus_amd._abi import CONSTS, lib
    dll = lib.load()
    INVALID, UNSUPPORTED = -1, -2
    a = torch.zeros(4 * 9 * 48, device='cuda')
    p = a.data_ptr()
    assert dll.vitae_vit_assemble_bwd(None, p, None, p, p, 2, 8, 48, 0, None) == INVALID
    assert dll.vitae_vit_assemble_bwd(p, None, None, None, None, 2, 8, 48, 0, None) == INVALID
    assert dll.vitae_vit_assemble_bwd(p, p, None, p, p, 0, 8, 48, 0, None) == INVALID
    assert dll.vitae_vit_assemble_bwd(p + 4, p, None, p, p, 2, 8, 48, 0, None) == INVALID         # misaligned
    assert dll.vitae_vit_assemble_bwd(p, p, None, p, p, 2, 8, 46, 0, None) == UNSUPPORTED
    assert dll.vitae_token_select_bwd(None, p, 2, 9, 48, 1, None) == INVALID
    assert dll.vitae_token_select_bwd(p, None, 2, 9, 48, 1, None) == INVALID
    assert dll.vitae_token_select_bwd(p, p, 2, 9, 48, 2, None) == INVALID
    assert dll.vitae_token_select_bwd(p, p, 2, 1, 48, 1, None) == INVALID                         # mean over no token
    assert dll.vitae_token_select_bwd(p, p, 2, 9, 50, 0, None) == UNSUPPORTED
    torch.cuda.synchronize()
    assert CONSTS['VITAE_ABI_VERSION'] >= 49


# ----------------------------------------------------------------------------------------------- GPU: training path
def _step(m, x, y, crit):
    m.zero_grad(set_to_none=True)
    logits = m(x)
    loss = crit(logits, y)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), logits.detach().cpu().numpy(), _grads(m)


def _check_grads(gold, tag, grads, bound, report):
    names = [str(n) for n in gold[f'{tag}/names']]
    assert sorted(names) == sorted(grads.keys())           # no parameter is left out
    worst = (0.0, None)
    for n in names:
        assert grads[n] is not None, n
        e = _rel(grads[n], gold[f'{tag}/grad/{n}'])
        worst = max(worst, (e, n))
        print(f'{report} {tag} {n}: relative L2 error {e:.3e}')
    assert worst[0] <= bound, worst


def _check_trajectory(gold, gp, precision):
    m = _micro(gp, precision)
    crit = _criterion(gold, 'cuda')
    x = torch.from_numpy(np.load(FEAT, allow_pickle=False)['micro/x']).cuda()
    y = torch.from_numpy(gold['labels']).cuda()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=0.05)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss = crit(m(x), y)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    ref = gold[f'{TAGS[gp]}/adamw_losses']
    print(f'{precision} {TAGS[gp]} AdamW losses {losses} (reference {list(ref)})')
    for a, b in zip(losses, ref):
        assert abs(a - b) <= 1e-4 * abs(b), (losses, list(ref))


@pytest.mark.gpu
@pytest.mark.parametrize('gp', [False, True])
@pytest.mark.parametrize('precision', ['fp32', 'fp32x3'])
def test_finetune_gradients_micro(gold, x_micro, gp, precision):
    tag = TAGS[gp]
    m = _micro(gp, precision)
    loss, logits, grads = _step(m, x_micro.cuda(), torch.from_numpy(gold['labels']).cuda(), _criterion(gold, 'cuda'))
    ref_y = gold[f'{tag}/logits']
    print(f'{precision} {tag}: loss {loss} (reference {float(gold[f"{tag}/loss"])})')
    assert np.abs(logits - ref_y).max() < 1e-4 * max(1.0, np.abs(ref_y).max())
    assert abs(loss - float(gold[f'{tag}/loss'])) <= 1e-4 * abs(float(gold[f'{tag}/loss']))
    _check_grads(gold, tag, grads, 1e-4, precision)
    assert m._trainer.stats['kept_bytes'] > 0


@pytest.mark.gpu
@pytest.mark.parametrize('gp', [False, True])
@pytest.mark.parametrize('precision', ['fp32', 'fp32x3'])
def test_finetune_adamw_trajectory_micro(gold, gp, precision):
    _check_trajectory(gold, gp, precision)


@pytest.mark.gpu
@pytest.mark.parametrize('gp', [False, True])
def test_finetune_gradients_micro_bf16(gold, x_micro, gp):
    """Per parameter at most twice the error the reference itself shows under bf16 autocast on the same weights."""
    tag = TAGS[gp]
    m = _micro(gp, 'bf16')
    loss, _, grads = _step(m, x_micro.cuda(), torch.from_numpy(gold['labels']).cuda(), _criterion(gold, 'cuda'))
    assert np.isfinite(loss)
    worst = (0.0, None)
    for n in (str(n) for n in gold[f'{tag}/names']):
        e, allowed = _rel(grads[n], gold[f'{tag}/grad/{n}']), float(gold[f'{tag}/bf16_ref_relerr/{n}'])
        print(f'bf16 {tag} {n}: relative L2 error {e:.3e}, reference under autocast {allowed:.3e}, ratio {e / allowed:.2f}')
        worst = max(worst, (e / allowed, n))
    assert worst[0] <= 2.0, worst


@pytest.mark.gpu
def test_finetune_epoch_soft_targets_accumulation(gold, x_micro):
    """train_one_epoch with gradient accumulation over two batches, soft targets, AdamW over layer-decay groups: loss 1e-4
    relative, every parameter delta 1e-4 relative L2 — with the key third of ``attn.qkv.bias`` compared separately (its
    gradient is zero in exact arithmetic, see below; measured as a whole parameter: 1.6e-3 / 2.6e-3)."""
    from vit_ae_plus_plus_amd.post_training_utils.fine_tune_epoch import train_one_epoch
    from vit_ae_plus_plus_amd.utils.custom_loss import SoftCrossEntropyWithWeightsLoss
    from vit_ae_plus_plus_amd.utils.lr_decay import get_layer_id_for_vit, param_groups_lrd
    from vit_ae_plus_plus_amd.utils.misc import NativeScalerWithGradNormCount
    accum_iter, lr, min_lr, warmup_epochs, epochs, epoch = (float(v) for v in gold['epoch/args'])
    args = Namespace(accum_iter=int(accum_iter), lr=lr, min_lr=min_lr, warmup_epochs=warmup_epochs, epochs=epochs)
    t0, t1 = (torch.from_numpy(t) for t in gold['epoch/targets'])
    batches = [(x_micro, None, t0), (x_micro.flip(0).contiguous(), None, t1)]
    m = _micro(True)
    before = {n: p.detach().cpu().clone() for n, p in m.named_parameters()}
    wd, ld = (float(v) for v in gold['lrd/args'])
    opt = torch.optim.AdamW(param_groups_lrd(m, wd, no_weight_decay_list=m.no_weight_decay(), layer_decay=ld), lr=lr)
    crit = SoftCrossEntropyWithWeightsLoss(torch.from_numpy(gold['class_weights'])).cuda()
    stats = train_one_epoch(m, crit, batches, opt, torch.device('cuda'), int(epoch), NativeScalerWithGradNormCount(),
                            max_norm=None, args=args)
    print('epoch stats', stats, 'reference', float(gold['epoch/loss']), float(gold['epoch/lr']))
    assert abs(stats['loss'] - float(gold['epoch/loss'])) <= 1e-4 * float(gold['epoch/loss'])
    assert abs(stats['lr'] - float(gold['epoch/lr'])) <= 1e-12 + 1e-9 * float(gold['epoch/lr'])
    worst = (0.0, None)
    D, n_layers = m.embed_dim, len(m.blocks) + 1
    for n, p in m.named_parameters():
        got, ref = (p.detach().cpu() - before[n]).numpy(), gold[f'epoch/delta/{n}']
        if n.endswith('attn.qkv.bias'):
            # The key bias has NO gradient in exact arithmetic (softmax is invariant to a shift common to all keys of a row): in
            # the reference it is rounding noise (norm 3e-10 .. 5e-10 in the fixture against 0.43 for the value bias), and
            # Adam's g / (sqrt(v) + eps) turns that noise into steps of 1e-6 .. 7e-6 that no other implementation reproduces
            # (measured: 1.6e-3 / 2.6e-3 relative L2 over the whole parameter, all of it from these 48 entries).  So the query
            # and value thirds are held to the bound, and the key third to what holds for any noise: |step| <= lr * lr_scale.
            step = lr * ld ** (n_layers - get_layer_id_for_vit(n, n_layers))
            assert np.abs(got[D:2 * D]).max() <= step * (1 + 1e-6), n
            assert np.linalg.norm(gold[f'gp/grad/{n}'][D:2 * D]) <= 1e-8 * np.linalg.norm(gold[f'gp/grad/{n}']), n
            got, ref = np.delete(got, np.s_[D:2 * D]), np.delete(ref, np.s_[D:2 * D])
        e = _rel(got, ref)
        print(f'epoch delta {n}: relative L2 error {e:.3e}')
        worst = max(worst, (e, n))
    assert worst[0] <= 1e-4, worst
    assert all(p.grad is None or float(p.grad.abs().sum()) == 0 for p in m.parameters())     # zeroed after the last step


@pytest.mark.gpu
def test_soft_target_loss_and_gradient_norms(gold, x_micro):
    from vit_ae_plus_plus_amd.utils.custom_loss import SoftCrossEntropyWithWeightsLoss
    for gp in (False, True):
        m = _micro(gp)
        crit = SoftCrossEntropyWithWeightsLoss(torch.from_numpy(gold['class_weights'])).cuda()
        loss, _, grads = _step(m, x_micro.cuda(), torch.from_numpy(gold['epoch/targets'][0]).cuda(), crit)
        ref = float(gold[f'{TAGS[gp]}/soft/loss'])
        assert abs(loss - ref) <= 1e-4 * abs(ref)
        norms = np.array([np.linalg.norm(grads[n].astype(np.float64)) for n, _ in m.named_parameters()])
        assert np.abs(norms - gold[f'{TAGS[gp]}/soft/grad_norm']).max() <= 1e-4 * np.abs(gold[f'{TAGS[gp]}/soft/grad_norm']).max()


@pytest.mark.gpu
@pytest.mark.parametrize('gp', [False, True])
def test_finetune_frozen_parameters(gold, x_micro, gp):
    tag = TAGS[gp]
    x, y, crit = x_micro.cuda(), torch.from_numpy(gold['labels']).cuda(), _criterion(gold, 'cuda')
    # head only (--fix_backbone): the inference path runs, nothing is kept, the encoder gets no gradient
    m = _micro(gp)
    for n, p in m.named_parameters():
        p.requires_grad = n.startswith('head.')
    loss, _, grads = _step(m, x, y, crit)
    assert m._trainer is None                              # the training sequence was never built, so nothing was kept
    assert abs(loss - float(gold[f'{tag}/loss'])) <= 1e-4 * abs(float(gold[f'{tag}/loss']))
    for n, g in grads.items():
        if n.startswith('head.'):
            assert _rel(g, gold[f'{tag}/grad/{n}']) <= 1e-4, n
        else:
            assert g is None, n
    # embedding and block 0 frozen: the other gradients are those of the unfrozen run
    full = _micro(gp)
    _, _, g_full = _step(full, x, y, crit)
    kept_full = full._trainer.stats['kept_bytes']
    frozen = lambda n: n.startswith(('patch_embed.', 'blocks.0.')) or n in ('pos_embed', 'cls_token')
    m = _micro(gp)
    for n, p in m.named_parameters():
        p.requires_grad = not frozen(n)
    _, _, g_part = _step(m, x, y, crit)
    assert 0 < m._trainer.stats['kept_bytes'] < kept_full          # block 0 and the patch rows are not kept
    for n in g_full:
        if frozen(n):
            assert g_part[n] is None, n
        else:
            assert _rel(g_part[n], g_full[n]) <= 1e-6, n
    # a frozen weight inside a trainable block: no gradient for it, the rest unchanged
    m = _micro(gp)
    m.blocks[1].mlp.fc1.weight.requires_grad = False
    m.blocks[0].attn.qkv.bias.requires_grad = False
    _, _, g_one = _step(m, x, y, crit)
    for n in g_full:
        if n in ('blocks.1.mlp.fc1.weight', 'blocks.0.attn.qkv.bias'):
            assert g_one[n] is None
        else:
            assert _rel(g_one[n], g_full[n]) <= 1e-6, n


@pytest.mark.gpu
def test_two_forwards_then_two_backwards(gold, x_micro):
    y, crit = torch.from_numpy(gold['labels']).cuda(), _criterion(gold, 'cuda')
    xa = x_micro.cuda()
    xb = (x_micro.flip(0) * 0.5 + 0.1).contiguous().cuda()[:2]        # another input, another batch size
    yb = y[:2]
    m = _micro(True)
    _, _, ga = _step(m, xa, y, crit)
    _, _, gb = _step(m, xb, yb, crit)
    m.zero_grad(set_to_none=True)
    la, lb = crit(m(xa), y), crit(m(xb), yb)
    with torch.no_grad():                                             # an evaluation in between keeps nothing and disturbs nothing
        m.eval()
        m(xb)
        m.train()
    la.backward()
    g1 = _grads(m)
    m.zero_grad(set_to_none=True)
    lb.backward()
    g2 = _grads(m)
    for n in ga:
        assert _rel(g1[n], ga[n]) <= 1e-6 and _rel(g2[n], gb[n]) <= 1e-6, n
    # accumulation into .grad across two backwards
    m.zero_grad(set_to_none=True)
    crit(m(xa), y).backward()
    crit(m(xb), yb).backward()
    for n, g in _grads(m).items():
        assert _rel(g, ga[n] + gb[n]) <= 1e-6, n


@pytest.mark.gpu
def test_drop_path_is_ignored_and_dropout_still_raises(gold, x_micro):
    from vit_ae_plus_plus_amd._abi import VitaeError
    x, y, crit = x_micro.cuda(), torch.from_numpy(gold['labels']).cuda(), _criterion(gold, 'cuda')
    m = _micro(True, drop_path_rate=0.1)                              # the reference ignores the argument as well
    loss, _, grads = _step(m, x, y, crit)
    assert abs(loss - float(gold['gp/loss'])) <= 1e-4 * abs(float(gold['gp/loss']))
    assert all(g is not None for g in grads.values())
    with pytest.raises(VitaeError):
        _micro(True, drop_rate=0.1)(x)
    m = _micro(True)
    m.drop_rate = 0.1
    with pytest.raises(VitaeError):
        m(x)
    with pytest.raises(VitaeError):                                   # no CPU fallback in training mode either
        _module(_cfg(True)).train()(x_micro)
    m = _micro(True).eval()                                           # eval mode stays the inference path: a detached result
    assert not m(x).requires_grad


@pytest.fixture(scope='module')
def vitb_oracle():
    """Loss and per-parameter gradient norms of ViT-B/16 on 96^3 x 4ch, batch 2, from the oracle's autograd on the CPU."""
    cfg = V.VitConfig(num_classes=2, global_pool=True, **VITB)
    sd = {k: v.clone().requires_grad_(True) for k, v in V.init_vit_state_dict(cfg, seed=7).items()}
    xb, _ = R.synthetic_views((2, 4, 96, 96, 96), seed=1234)
    y = torch.tensor([1, 0])
    loss = torch.nn.functional.cross_entropy(V.forward(sd, xb, cfg), y)
    loss.backward()
    return cfg, xb, y, float(loss.detach()), {k: float(v.grad.double().norm()) for k, v in sd.items()}


@pytest.mark.gpu
@pytest.mark.parametrize('precision', ['fp32', 'fp32x3', 'bf16'])
def test_finetune_vitb(vitb_oracle, precision):
    """The shape users run (217 tokens, D = 768: split-K and tile choices the micro configuration never reaches).
    fp32 / fp32x3: loss 1e-4, each gradient norm 2e-3 relative (the bounds of the ViT-B pins in tests/test_gpu_model.py);
    bf16: finite, figures printed."""
    cfg, xb, y, ref_loss, ref_norms = vitb_oracle
    m = _module(cfg, precision).cuda().train()
    m.load_state_dict(V.init_vit_state_dict(cfg, seed=7))
    loss, _, grads = _step(m, xb.cuda(), y.cuda(), torch.nn.CrossEntropyLoss())
    worst = (0.0, None)
    for n, refn in ref_norms.items():
        assert grads[n] is not None and np.isfinite(grads[n]).all(), n
        worst = max(worst, (abs(float(np.linalg.norm(grads[n].astype(np.float64))) - refn) / refn, n))
    print(f'ViT-B {precision}: loss {loss} (oracle {ref_loss}, relative error {abs(loss - ref_loss) / abs(ref_loss):.2e}), '
          f'worst gradient-norm error {worst[0]:.2e} ({worst[1]})')
    assert np.isfinite(loss)
    if precision != 'bf16':
        assert abs(loss - ref_loss) <= 1e-4 * abs(ref_loss)
        assert worst[0] <= 2e-3, worst


@pytest.mark.gpu
def test_backward_refuses_parameters_changed_since_the_forward(gold, x_micro):
    """The backward reads the weights again, so an in-place update between forward and backward must not go unnoticed."""
    from vit_ae_plus_plus_amd._abi import VitaeError
    m = _micro(True)
    loss = _criterion(gold, 'cuda')(m(x_micro.cuda()), torch.from_numpy(gold['labels']).cuda())
    with torch.no_grad():
        m.blocks[1].mlp.fc2.weight.mul_(1.0)
    with pytest.raises(VitaeError):
        loss.backward()
    torch.cuda.synchronize()
