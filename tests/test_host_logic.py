"""CPU: host-side logic of the drop-in surface (no kernels): schedule, meters, scaler state,
factories / state-dict keys, arena layout rules, drop-in aliases, loud failure on CPU tensors."""
import argparse
import math
import os

import numpy as np
import pytest
import torch

from oracle import mae_ref as R
from vit_ae_plus_plus_amd._abi import VitaeError
from vit_ae_plus_plus_amd.model import model_factory, vit_autoenc
from vit_ae_plus_plus_amd.model.model_utils.vit_helpers import get_3d_sincos_pos_embed
from vit_ae_plus_plus_amd.utils import lr_sched, misc


def test_lr_schedule_matches_oracle_restatement():
    from oracle.train_ref import lr_at
    args = argparse.Namespace(lr=1e-3, min_lr=1e-5, warmup_epochs=40, epochs=50)

    class Opt:
        param_groups = [{'lr': 0.0}, {'lr': 0.0, 'lr_scale': 0.5}]
    for e in (0.0, 0.5, 3.25, 39.99, 40.0, 44.4, 50.0):
        lr = lr_sched.adjust_learning_rate(Opt, e, args)
        assert lr == pytest.approx(lr_at(e, 1e-3, 1e-5, 40, 50), rel=1e-15, abs=1e-20)
        assert Opt.param_groups[0]['lr'] == lr and Opt.param_groups[1]['lr'] == lr * 0.5


def test_smoothed_value_and_logger(capsys):
    m = misc.SmoothedValue(window_size=3)
    for v in (1.0, 5.0, 3.0, 4.0):
        m.update(v)
    assert m.count == 4 and m.total == 13.0 and m.global_avg == 3.25
    assert m.median == float(torch.tensor([5.0, 3.0, 4.0]).median()) and m.max == 5.0 and m.value == 4.0
    assert abs(m.avg - 4.0) < 1e-6
    m2 = misc.SmoothedValue(window_size=4)
    for v in (1.0, 2.0, 3.0, 4.0):
        m2.update(v)
    assert m2.median == float(torch.tensor([1.0, 2.0, 3.0, 4.0]).median()) == 2.0   # lower middle
    lg = misc.MetricLogger(delimiter="  ")
    lg.add_meter('lr', misc.SmoothedValue(window_size=1, fmt='{value:.6f}'))
    seen = [x for x in lg.log_every(range(5), 2, 'Epoch: [0]')]
    assert seen == list(range(5))
    lg.update(loss=torch.tensor(2.0), lr=0.1, skipped=None)
    assert lg.loss.global_avg == 2.0 and 'skipped' not in lg.meters
    out = capsys.readouterr().out
    assert 'Epoch: [0]' in out and 'Total time' in out
    with pytest.raises(AttributeError):
        lg.nope


def test_scaler_state_dict_format():
    s = misc.NativeScalerWithGradNormCount()
    sd = s.state_dict()
    assert set(sd) == {'scale', 'growth_factor', 'backoff_factor', 'growth_interval', '_growth_tracker'}
    s.load_state_dict({'scale': 65536.0, 'growth_factor': 2.0, 'backoff_factor': 0.5, 'growth_interval': 2000,
                       '_growth_tracker': 7})
    assert s.state_dict()['scale'] == 1.0 and s.state_dict()['_growth_tracker'] == 7
    assert misc.all_reduce_mean(3.5) == 3.5 and misc.get_world_size() == 1 and misc.is_main_process()


def test_get_grad_norm_matches_reference_formula():
    ps = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(7)), torch.nn.Parameter(torch.randn(2))]
    ps[0].grad, ps[1].grad = torch.randn(5, 3), torch.randn(7)
    want = torch.norm(torch.stack([torch.norm(p.grad, 2.0) for p in ps[:2]]), 2.0)
    assert torch.allclose(misc.get_grad_norm_(ps), want)
    assert float(misc.get_grad_norm_([ps[2]])) == 0.0


def _args(**kw):
    d = dict(model='contr_mae_vit_base_patch16', volume_size=96, in_channels=4, patch_size=16, use_imagenet=False,
             perceptual_weight=0)
    d.update(kw)
    return argparse.Namespace(**d)


@pytest.mark.parametrize('name,contr', [('contr_mae_vit_tiny_patch16', True), ('mae_vit_tiny_patch16', False)])
def test_factory_state_dict_keys_match_reference_layout(name, contr):
    model = model_factory.get_models('autoenc', _args(model=name, volume_size=64, in_channels=1))
    cfg = R.RefConfig(volume_size=(64,) * 3, patch_size=16, in_chans=1, embed_dim=128, depth=2, num_heads=4,
                      decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=4, contrastive=contr)
    spec = R.state_dict_spec(cfg)   # pinned against the reference's own state dict in test_oracle_golden
    sd = model.state_dict()
    assert list(sd.keys()) == list(spec.keys())
    for k, shp in spec.items():
        assert tuple(sd[k].shape) == shp, k
    frozen = {k for k, p in model.named_parameters() if not p.requires_grad}
    assert frozen == {'pos_embed', 'decoder_pos_embed', 'sobel_filter3D.sobel_filter.weight',
                      'sobel_filter3D.sobel_filter.bias'}
    np.testing.assert_array_equal(sd['pos_embed'][0].numpy(),
                                  get_3d_sincos_pos_embed(128, 4, True).astype(np.float32))
    np.testing.assert_array_equal(sd['sobel_filter3D.sobel_filter.weight'].numpy(), R.sobel_kernels().numpy())
    # init statistics (vit_autoenc.py:65-98): LN (1,0), linear biases 0, xavier bound
    assert float(sd['blocks.0.norm1.weight'].min()) == 1.0 and float(sd['blocks.1.mlp.fc2.bias'].abs().max()) == 0.0
    w = sd['blocks.0.attn.qkv.weight']
    assert float(w.abs().max()) <= math.sqrt(6.0 / (128 + 384)) + 1e-6
    w = sd['patch_embed.proj.weight']
    assert float(w.abs().max()) <= math.sqrt(6.0 / (128 + 4096)) + 1e-6
    # reference-format state dicts (incl. the real reference's perceptual_loss.* tensors) load
    ref_sd = R.init_state_dict(cfg, seed=1)
    ref_sd['perceptual_loss.slice1.0.weight'] = torch.zeros(3)
    model.load_state_dict(ref_sd)
    assert torch.equal(model.state_dict()['decoder_pred.weight'], ref_sd['decoder_pred.weight'])


def test_vitb_parameter_count_matches_survey():
    model = vit_autoenc.contr_mae_vit_base_patch16(volume_size=96, in_chans=4, patch_size=16, args=_args())
    n_train = sum(p.numel() for p in model.parameters() if p.requires_grad)
    n_all = sum(p.numel() for p in model.parameters())   # trainable + frozen (tables, sobel)
    assert n_train == 132_841_728 and n_all == 133_119_572
    assert model.patch_embed.num_patches == 216 and model.patch_embed.patch_size == (16, 16, 16)
    assert model.patch_embed.grid_size == (6, 6, 6) and model.embed_dim == 768 and len(model.blocks) == 12


def test_patchify_roundtrip_and_kat():
    model = vit_autoenc.mae_vit_tiny_patch16(volume_size=(8, 4, 12), in_chans=3, patch_size=4, args=_args())
    v = torch.randn(2, 3, 8, 4, 12)
    assert torch.equal(model.unpatchify(model.patchify(v)), v)
    assert torch.equal(model.patchify(v), R.patchify(v, 4))


def test_cpu_forward_fails_loudly_instead_of_falling_back():
    model = model_factory.get_models('autoenc', _args(model='contr_mae_vit_tiny_patch16', volume_size=64, in_channels=1))
    x = torch.zeros(1, 1, 64, 64, 64)
    with pytest.raises(VitaeError, match='no CPU fallback'):
        model(view1=x, view2=x)
    from vit_ae_plus_plus_amd.utils.train_one_epoch import compute_contrastive_loss
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        compute_contrastive_loss(_args(contr_weight=1.0), None, torch.zeros(2, 4), torch.zeros(2, 4), torch.zeros(2, 4),
                                 torch.zeros(2, 4))


def test_unsupported_options_are_rejected():
    # a perceptual weight builds the VGG hook with the reference's keys (it was refused in round 1)
    m = vit_autoenc.mae_vit_tiny_patch16(volume_size=64, in_chans=1, patch_size=16, args=_args(perceptual_weight=1))
    assert 'perceptual_loss.slice3.14.weight' in m.state_dict()
    assert not any(k.startswith('perceptual_loss.') for k, p in m.named_parameters() if p.requires_grad)
    with pytest.raises(VitaeError):
        vit_autoenc.mae_vit_tiny_patch16(volume_size=64, in_chans=1, patch_size=16, args=_args(), norm_pix_loss=True)
    with pytest.raises(NotImplementedError):
        model_factory.get_models('nope', _args())


def test_dropin_aliases():
    import subprocess, sys, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import vit_ae_plus_plus_amd.dropin as d; d.install();"
            "from model.model_factory import get_models; from model.vit_autoenc import ContrastiveMAEViT;"
            "from utils import misc, lr_sched; from utils.train_one_epoch import train_one_stage_epoch, train_one_epoch, "
            "compute_contrastive_loss; from model.model_utils.vit_helpers import get_3d_sincos_pos_embed, interpolate_pos_embed;"
            "from model.vit import PatchEmbed3D, Mlp3D, Attention, Block; print('ok')")
    r = subprocess.run([sys.executable, '-c', code], cwd=root, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stderr


def test_fused_adamw_param_groups_follow_timm_rule():
    from vit_ae_plus_plus_amd.optim import FusedAdamW
    model = vit_autoenc.contr_mae_vit_tiny_patch16(volume_size=64, in_chans=1, patch_size=16, args=_args())
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.05)
    names = {id(p): n for n, p in model.named_parameters()}
    ref = R.param_groups(dict(model.named_parameters()), 0.05)
    assert [names[id(p)] for p in opt.param_groups[0]['params']] == ref[0]['names']
    assert [names[id(p)] for p in opt.param_groups[1]['params']] == ref[1]['names']
    assert 'cls_token' in ref[1]['names'] and 'norm.weight' in ref[0]['names']


def test_pos_embed_matches_reference_kat(golden):
    """get_3d_sincos_pos_embed against the table the reference's own function produced (tests/golden/kats.npz),
    not against itself."""
    from vit_ae_plus_plus_amd.model.model_utils.vit_helpers import get_3d_sincos_pos_embed
    g = golden('kats.npz')
    keys = [k for k in g.files if 'pos' in k.lower()]
    assert keys, g.files
    checked = 0
    for k in keys:
        ref = g[k]
        if ref.ndim != 2:
            continue
        rows, dim = ref.shape
        n = round((rows - 1) ** (1 / 3))
        if n ** 3 != rows - 1:
            continue
        got = get_3d_sincos_pos_embed(dim, n, cls_token=True)
        np.testing.assert_allclose(np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), rtol=0, atol=1e-7)
        checked += 1
    assert checked >= 1


def test_bench_rank_plumbing():
    """bench.py --gpus N: spawns N ranks when no launcher is around, refuses fewer visible GPUs, and refuses a launcher that
    provides a different number of ranks (`--gpus 8` silently ran dp1)."""
    import bench
    args = bench.parse(['--gpus', '2', '--steps', '3'])
    os.environ.pop('WORLD_SIZE', None)
    with pytest.raises(SystemExit) as e:
        bench.spawn_command(args, ['--gpus', '2'], n_visible=1, port=12345)
    assert 'only 1 GPU' in str(e.value)
    cmd = bench.spawn_command(args, ['--gpus', '2', '--steps', '3'], n_visible=2, port=12345)
    assert '--nproc-per-node=2' in cmd and '127.0.0.1' in cmd and cmd[-4:] == ['--gpus', '2', '--steps', '3']
    assert bench.spawn_command(bench.parse(['--gpus', '1']), [], n_visible=0, port=1) is None
    with pytest.raises(SystemExit):
        bench.rank_layout(args, env={'WORLD_SIZE': '1'})
    with pytest.raises(SystemExit):
        bench.rank_layout(bench.parse(['--gpus', '1']), env={'WORLD_SIZE': '8', 'RANK': '3', 'LOCAL_RANK': '3'})
    assert bench.rank_layout(args, env={'WORLD_SIZE': '2', 'RANK': '1', 'LOCAL_RANK': '1'}) == (2, 1, 1)


def test_bench_options():
    """bench.py: the secondary measurements are opt-in (--full), --dump-outputs takes a directory, and --steps counts timed steps."""
    import bench
    a = bench.parse(['--gpus', '1', '--steps', '7', '--warmup', '2'])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = bench.parse(['--full', '--dump-outputs', 'out'])
    assert a.full and a.dump_outputs == 'out'
    with pytest.raises(SystemExit):
        bench.parse(['--steps', '0'])


def test_fit_split_shrinks_to_capacity_and_caches_per_key():
    """_launch.fit_split: the planner's proposal lowered until its scratch fits (never below 1), one planner call per key, and the
    GELU rule as the engine's call sites apply it — outside the cache, so a cached split never depends on the epilogue."""
    from vit_ae_plus_plus_amd._launch import EPI_GELU, EPI_NONE, fit_split
    cache, calls = {}, []

    def pick(v):
        return lambda: (calls.append(v), v)[1]

    need = lambda s: 100 * s
    assert fit_split(cache, 'a', pick(7), need, 350) == 3 and cache == {'a': 3}
    assert fit_split({}, 'a', pick(7), need, 99) == 1            # capacity below need(1): one split, no further
    assert fit_split({}, 'a', pick(2), need, 10 ** 6) == 2       # what fits is left alone
    calls.clear()
    split = lambda key, v: cache.get(key) or fit_split(cache, key, pick(v), need, 10 ** 6)
    assert [split('b', 5), split('b', 9), split('b', 9)] == [5, 5, 5] and calls == [5]
    site = lambda epi: 1 if (epi & 15) == EPI_GELU else split('c', 5)       # (_g16_fwd, _lin_fwd)
    assert [site(EPI_NONE), site(EPI_GELU | 16), site(EPI_NONE)] == [5, 1, 5] and cache['c'] == 5
    assert [1 if (e & 15) == EPI_GELU else split('d', 5) for e in (EPI_GELU, EPI_NONE)] == [1, 5]      # GELU first: nothing cached for it


def test_environment_switches_are_the_documented_ones():
    """Every VITAE_* name the Python package reads from the environment has a row in DESIGN.md's table of Python-side switches
    (section 3d), and every row is still read: a new knob cannot arrive, and a retired one cannot linger, unseen."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    read = set()
    for d, _, files in os.walk(os.path.join(root, 'vit_ae_plus_plus_amd')):
        for f in files:
            if f.endswith('.py'):
                with open(os.path.join(d, f)) as fh:
                    read |= set(re.findall(r'''environ(?:\.get\(|\[)\s*['"](VITAE_\w+)['"]''', fh.read()))
    with open(os.path.join(root, 'DESIGN.md')) as fh:
        section = re.search(r'^### 3d\. Python-side switches\n(.*?)^###? ', fh.read(), flags=re.S | re.M).group(1)
    table = re.findall(r'^\| `(VITAE_\w+)` \|', section, flags=re.M)
    assert len(table) == len(set(table)) and len(table) >= 12
    assert set(table) == read, (sorted(read - set(table)), sorted(set(table) - read))


def test_library_environment_switches_are_the_documented_ones():
    """The same for the library: every VITAE_* string literal that csrc/ hands to getenv or to the two helpers of common.hpp (env_int,
    ENV_INT_ONCE) has a row in DESIGN.md's table of library-side switches, and every row is still read.  Matching on the call keeps
    VITAE_ERR_* and the other macros out; a name that reaches getenv any other way (a variable, a concatenation) fails the second
    assertion: the only getenv of csrc/ is the one inside env_int, on its parameter."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, 'vit_ae_plus_plus_amd', 'csrc')
    read, getenvs = set(), []
    for f in sorted(os.listdir(csrc)):
        if f.endswith(('.hip', '.hpp')):
            with open(os.path.join(csrc, f)) as fh:
                code = re.sub(r'//[^\n]*', '', fh.read())
            read |= set(re.findall(r'\b(?:getenv|env_int|ENV_INT_ONCE)\(\s*"(VITAE_\w+)"', code))
            getenvs += [(f, a) for a in re.findall(r'\bgetenv\(\s*([^)]*)\)', code)]
    assert getenvs == [('common.hpp', 'name')], getenvs
    with open(os.path.join(root, 'DESIGN.md')) as fh:
        section = re.search(r'^### 3d-lib\. Library-side switches\n(.*?)^###? ', fh.read(), flags=re.S | re.M).group(1)
    table = re.findall(r'^\| `(VITAE_\w+)` \|', section, flags=re.M)
    assert len(table) == len(set(table)) and len(table) >= 15
    assert set(table) == read, (sorted(read - set(table)), sorted(set(table) - read))
