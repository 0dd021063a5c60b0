"""Text trace of everything the host sequencing code issues: every ``lib.*`` call (ints / floats by value; pointers, streams
included, as NULL or p<k>, k = ordinal of the address's first appearance, so offsets into a buffer are distinct but reproducible
and a swapped buffer shows up) and, in sequence, every ``Stream.wait_stream`` / ``Stream.wait_event`` / ``Event.record``.  Two
steps per case (first sight, then the cache-hit paths).  Diff the output of two trees to check that a change to engine.py /
encoder.py launches the same things in the same order:

    python tools/launch_trace.py CASE [--timer]        CASE = 1 .. 8, knobs through the environment, e.g.
    VITAE_SIDE_STREAMS=all VITAE_WGRAD_GROUP_MIN=0 python tools/launch_trace.py 5
"""
import argparse, ctypes, os, re, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from oracle import mae_ref as R
from oracle.gen_golden import MICRO
from vit_ae_plus_plus_amd import _abi

ACT16 = dict(volume_size=(16, 16, 16), patch_size=4, in_chans=4, embed_dim=64, depth=2, num_heads=2,
             decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=2)       # tests/test_gpu_model.py
W256 = dict(ACT16, embed_dim=256, num_heads=8, decoder_embed_dim=256, decoder_num_heads=8)     # LayerNorm records, _ln_flush
# case -> (dimensions, precision, contrastive, batch); the knobs of cases 3 and 5 come from the environment (several are read at
# import).  Case 5 at batch 8: the grouped weight-gradient launch needs 256 padded token rows in both stacks
CASES = {1: (MICRO, 'fp32', True, 2), 2: (MICRO, 'fp32x3', True, 2), 3: (MICRO, 'fp32', True, 2), 4: (ACT16, 'bf16', True, 2),
         5: (ACT16, 'bf16', True, 8), 6: (W256, 'bf16', False, 2), 7: (ACT16, 'bf16', True, 2)}

_text = re.sub(r'/\*.*?\*/', '', open(_abi.HEADER).read(), flags=re.S)
DECLS = {m.group(1): [a.strip() for a in m.group(2).split(',')] for m in re.finditer(r'\b(vitae_\w+)\s*\(([^)]*)\)\s*;', _text)}
_ids, _alive = {'p': {}, 'e': {}}, []


def _ord(kind, key, obj=None):
    if key not in _ids[kind]:
        _ids[kind][key] = len(_ids[kind])
        _alive.append(obj)      # (an event that is freed would hand its id to the next one)
    return f'{kind}{_ids[kind][key]}'


def _p(addr):
    return _ord('p', int(addr)) if addr else 'NULL'


def _fmt(name, args):
    out, decl = [], DECLS[name]
    tables = any('* const*' in d for d in decl)      # host tables of n device pointers / ints: by content, not by host address
    for a, kind, d in zip(args, _abi.PROTOS[name][1], decl):
        addr = ctypes.cast(a, ctypes.c_void_p).value if kind == 'ptr' else None
        if kind != 'ptr':
            out.append(repr(a))
        elif addr and '* const*' in d:
            out.append('[' + ' '.join(_p(v) for v in (ctypes.c_uint64 * args[0]).from_address(addr)) + ']')
        elif addr and tables and d.startswith('const int*'):
            out.append(str(list((ctypes.c_int32 * args[0]).from_address(addr))))
        else:
            out.append(_p(addr))
    return f'{name}({", ".join(out)})'


def _patch():
    orig = _abi._Lib.__getattr__

    def traced(self, name):
        fn = orig(self, name)

        def call(*args):
            print(_fmt(name, args))
            return fn(*args)
        self.__dict__[name] = call      # (the binding caches its checked wrapper on the instance: keep ours in front of it)
        return call
    _abi._Lib.__getattr__ = traced
    S, E = torch.cuda.Stream, torch.cuda.Event
    for cls, meth, show in ((S, 'wait_stream', lambda s, o: f'{_p(s.cuda_stream)} wait_stream {_p(o.cuda_stream)}'),
                            (S, 'wait_event', lambda s, e: f'{_p(s.cuda_stream)} wait_event {_ord("e", id(e), e)}'),
                            (E, 'record', lambda e, s=None: f'record {_ord("e", id(e), e)} on '
                                                            f'{_p((torch.cuda.current_stream() if s is None else s).cuda_stream)}')):
        def logged(self, *a, _f=getattr(cls, meth), _show=show):
            print(_show(self, *a))
            return _f(self, *a)
        setattr(cls, meth, logged)


def mae_case(dims, precision, contrastive, B, timer):
    from functools import partial
    from vit_ae_plus_plus_amd.model import vit_autoenc as VA
    from vit_ae_plus_plus_amd.optim import FusedAdamW
    cfg, dev = R.RefConfig(contrastive=contrastive, **dims), torch.device('cuda', 0)
    vol = cfg.volume_size[0]
    model = (VA.ContrastiveMAEViT if contrastive else VA.MaskedAutoencoderViT)(
        volume_size=vol, patch_size=cfg.patch_size, in_chans=cfg.in_chans, embed_dim=cfg.embed_dim, depth=cfg.depth,
        num_heads=cfg.num_heads, decoder_embed_dim=cfg.decoder_embed_dim, decoder_depth=cfg.decoder_depth,
        decoder_num_heads=cfg.decoder_num_heads, mlp_ratio=cfg.mlp_ratio, norm_layer=partial(torch.nn.LayerNorm, eps=cfg.ln_eps),
        args=argparse.Namespace(use_imagenet=False, perceptual_weight=0), precision=precision)
    model.load_state_dict(R.init_state_dict(cfg, seed=9))
    model = model.to(dev).train()
    eng = model._ensure_engine(dev)
    _ = FusedAdamW(model, lr=1e-3, weight_decay=0.05, betas=(0.9, 0.95)).engine
    eng.set_loss_weights(0.01, 0.001 if contrastive else 0.0, 1, 1)
    eng.set_hparams(noise_keep=1.0)
    eng._alloc(B, 0.75)
    for step in range(2):
        v1, v2 = (v.to(dev) for v in R.synthetic_views((B, cfg.in_chans, *cfg.volume_size), seed=500 + step))
        noise = torch.cat(R.masking_noise(B, cfg.num_patches, seed=600 + step)[:2 if contrastive else 1]).to(dev)
        eng.optimizer_hparams(lr=1e-3)
        eng.gemm_timer = [] if timer else None
        print(f'--- step {step}: forked {eng.forked_branches()}')
        eng.train_step_launch(v1, v2 if contrastive else None, noise, 0.75)
        torch.cuda.synchronize()
        for rec in eng.gemm_timer or ():
            print('timer', rec[2:])
    print('losses finite:', bool(torch.isfinite(eng.losses[:6]).all()))


def encoder_case():
    from vit_ae_plus_plus_amd.encoder import HipEncoder, HipEncoderTrainer, HipEncoderTrainer16
    from vit_ae_plus_plus_amd.model.vit import VisionTransformer3D
    torch.manual_seed(0)
    m = VisionTransformer3D(volume_size=16, patch_size=4, in_chans=1, num_classes=0, embed_dim=64, depth=2, num_heads=2).cuda()
    x, dfeat = torch.randn(2, 1, 16, 16, 16, device='cuda'), torch.randn(2, 64, device='cuda')
    needs = {n: True for n, _ in m._encoder_params()}
    for prec in ('fp32', 'bf16'):
        enc = HipEncoder(m.eval(), prec)
        for step in range(2):
            print(f'--- forward_features {prec} {step}')
            enc.forward_features(x)
    for cls, prec in ((HipEncoderTrainer, 'fp32'), (HipEncoderTrainer16, 'bf16')):
        tr = cls(m.train(), prec)
        for step in range(2):
            print(f'--- {cls.__name__} {step}')
            feat, kept = tr.forward_keep(x, needs)
            grads = tr.backward(kept, dfeat)
            torch.cuda.synchronize()
        print('finite:', bool(torch.isfinite(feat).all() and all(torch.isfinite(g).all() for g in grads.values())))


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('case', type=int, choices=range(1, 9))
    ap.add_argument('--timer', action='store_true', help='set eng.gemm_timer and print (flops, tag, scope) of each record')
    a = ap.parse_args()
    torch.manual_seed(0)
    _patch()
    if a.case == 8:
        encoder_case()
    else:
        mae_case(*CASES[a.case], a.timer or a.case == 7)
