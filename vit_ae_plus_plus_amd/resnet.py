"""Launch sequences of the 3-D ResNet baseline (k_fold_training_scripts/resnet_3d.py) on the kernels of csrc/conv3d.hip and the
BasicBlock tail of csrc/norm.hip: one forward per route — inference on running statistics, training with what the backward needs
kept — and the backward in reverse order.  The counterpart of encoder.py for the convolutional baseline.

Inside the network every activation is channels-last rows ``[N D H W, C]``; operands of the convolutions are bf16, what a
BatchNorm reads (the convolution's output) and what a residual adds are fp32.  Launch order of one BasicBlock:

  forward    conv1 -> bn1 + relu -> conv2 -> [downsample conv -> bn] -> bn2 + residual + relu
  backward   bn2 tail (dx, dres) -> conv2 dW, dX -> bn1 tail -> conv1 dW -> [downsample bn -> dW -> dX] -> conv1 dX (added to the
             residual branch's gradient)

Kept per block for the backward: the bf16 input of each convolution, the fp32 output of each convolution (what BatchNorm
normalises), the fp32 outputs of the two ReLUs (their masks; the block output is also the next block's residual), mean / rstd.
Nothing here falls back to torch operators: a missing kernel is an error.

The bf16 operands of the convolutions live in a per-model ``ConvPackStore``: all stale ones are re-packed by one
``vitae_conv3d_pack_weights_multi`` launch when the first of them is asked for.  ``forward_batch_stats`` is the training arithmetic with
nothing kept (a MoCo momentum encoder).

``precision='fp32x3'`` (``ResNet(..., precision=)`` / ``set_precision``) is the parity-grade route: the same sequence on the split-operand
instances of csrc/conv3d.hip's kernels.  A convolution reads the fp32 tensor the sequence holds anyway (the BatchNorm tail's ``y``, the pooled stem, the
fp32 ``dx``) and splits it in registers; no bf16 activation copy is allocated or kept.  The weights are packed as two bf16 planes
(form ``transposed | VITAE_CONV3D_PACK_FORM_X3`` of the store).
"""
import os
import weakref

import numpy as np
import torch

from ._abi import CONSTS, VitaeError, lib

BF16, F32 = torch.bfloat16, torch.float32
PRECISIONS = ('bf16', 'fp32x3')
FORM_X3 = CONSTS['VITAE_CONV3D_PACK_FORM_X3']


def check_precision(p):
    if p not in PRECISIONS:
        raise VitaeError(f"ResNet: precision {p!r} is not built; 'bf16' and 'fp32x3' (fp32 operands split into bf16 hi + lo) are. "
                         f"An exact-fp32 convolution is not built.")
    return p


def _st(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _param(t, what):
    if not t.is_cuda or t.dtype != F32:
        raise VitaeError(f'{what} must be an fp32 tensor on the MI355X (is {t.dtype} on {t.device}); there is no CPU fallback')
    return t.detach().contiguous()


def _geo(N, vol, conv):
    return (N, *vol, conv.in_channels, conv.out_channels, *conv.kernel_size, *conv.stride, *conv.padding)


def conv_out_vol(vol, conv):
    return tuple((vol[i] + 2 * conv.padding[i] - conv.kernel_size[i]) // conv.stride[i] + 1 for i in range(3))


def pack_weight(conv, transposed, packs=None, x3=False):
    """The bf16 operand of ``conv`` (``transposed``: the input gradient's form; ``x3``: two planes per row, hi | lo).  ``packs``: the
    model's ``ConvPackStore`` — the stored operand, refreshed with every other stale one of the model in one launch; without it (or with
    ``VITAE_CONV_PACK_STORE=0``) a new buffer and one ``vitae_conv3d_pack_weight[_x3]`` launch per call.  The same bits either way."""
    if packs is not None and pack_store_enabled():
        return packs.operand(conv, transposed | (FORM_X3 if x3 else 0))
    w = _param(conv.weight, 'a convolution weight')
    elems, pack = (lib.vitae_conv3d_packed_elems_x3, lib.vitae_conv3d_pack_weight_x3) if x3 else (lib.vitae_conv3d_packed_elems, lib.vitae_conv3d_pack_weight)
    out = torch.empty(elems(conv.out_channels, conv.in_channels, *conv.kernel_size, transposed), dtype=BF16, device=w.device)
    pack(w.data_ptr(), out.data_ptr(), conv.out_channels, conv.in_channels, *conv.kernel_size, transposed, _st(w))
    return out


def pack_store_enabled():
    """``VITAE_CONV_PACK_STORE`` (default on; read at call time): 0 packs per call, for A/B runs and the equality test."""
    return os.environ.get('VITAE_CONV_PACK_STORE', '1') != '0'


class ConvPackStore:
    """Persistent bf16 operands of every convolution of one ResNet, in every form its routes use (forward and transposed; the stem,
    whose input has no gradient, forward only) — the analogue of ``shadow.ShadowStore`` for packed convolution weights.  A form is
    ``transposed | VITAE_CONV3D_PACK_FORM_X3``; the store holds the forms of ONE precision at a time: asking for a form of the other
    one (after ``set_precision``) drops what it held and enumerates anew, so the next refresh packs every operand of the new route in
    its one launch.

    An operand records the weight state it was packed from, ``(data_ptr, _version)``, and is current while that still matches.  ``operand()`` returns a current one as it is; otherwise ALL stale operands of the model are re-packed by one
    ``vitae_conv3d_pack_weights_multi`` launch.  Whatever writes a weight bumps its version: torch optimisers, ``load_state_dict`` and
    in-place edits by themselves, the raw-pointer updaters (EMA, LARS, MultiTensorAdamW) through ``increment_version``.  The table and
    its chunk list live in one pinned buffer with a device copy; both are rebuilt only when an address or the stale set changes.
    ``launches`` / ``table_builds`` count for the tests."""

    def __init__(self, model):
        self.model = weakref.ref(model)
        self.launches = 0
        self.table_builds = 0
        self.x3 = False             # the precision whose forms are held
        self._entries = None        # [dict(conv, form, geo, data, key)], the forms of one convolution next to each other
        self._index = {}            # (id(conv), form) -> entry
        self._table = None          # dict(sig, pinned, dev, n, chunks, keep)

    def __reduce__(self):           # a pickled or deep-copied model carries no store along: the copy makes its own
        return (_no_store, ())

    def _enumerate(self):
        model = self.model()
        stem = getattr(model, 'conv1', None)
        self._entries, self._index, self._table = [], {}, None
        for conv in model.modules():
            if isinstance(conv, torch.nn.Conv3d):
                for transposed in ((0,) if conv is stem else (0, 1)):
                    form = transposed | (FORM_X3 if self.x3 else 0)
                    e = dict(conv=conv, form=form, data=None, key=None, geo=(conv.out_channels, conv.in_channels, *conv.kernel_size, form))
                    self._entries.append(e)
                    self._index[(id(conv), form)] = e

    @staticmethod
    def _key(conv):
        w = conv._parameters['weight']
        return (w.data_ptr(), w._version)

    def operand(self, conv, form):
        form = int(form)
        e = self._index.get((id(conv), form))
        if e is None or e['conv'] is not conv:
            self.x3 = bool(form & FORM_X3)
            self._enumerate()
            e = self._index.get((id(conv), form))
            if e is None:
                raise VitaeError('ConvPackStore: this convolution (in this form) is not part of the model the store belongs to')
        if e['key'] != self._key(conv):
            self._refresh()
        return e['data']

    def _refresh(self):
        stale, sig, last, key = [], [], None, None
        for i, e in enumerate(self._entries):
            if e['conv'] is not last:
                last, key = e['conv'], self._key(e['conv'])
            if e['key'] != key:
                stale.append((e, key))
                sig.append((i, key[0]))
        t = self._table
        if t is None or t['sig'] != sig:       # another stale set, or a weight that moved: judge the weights again, make a new table
            t = self._table = self._build_table(stale, sig)
        with torch.cuda.device(t['dev'].device):
            lib.vitae_conv3d_pack_weights_multi(t['th'], t['td'], t['n'], t['ch'], t['cd'], t['chunks'], torch.cuda.current_stream().cuda_stream)
        self.launches += 1
        for e, key in stale:
            e['key'] = key

    def _build_table(self, stale, sig):
        weights = [_param(e['conv'].weight, 'a convolution weight') for e, _ in stale]
        device = weights[0].device
        rows = []
        for (e, _), w in zip(stale, weights):
            if w.device != device:
                raise VitaeError('ConvPackStore: the convolutions of one model must be on one device')
            if tuple(w.shape) != (*e['geo'][:2], *e['geo'][2:5]):
                raise VitaeError(f'ConvPackStore: a weight of shape {tuple(w.shape)} in a convolution of geometry {e["geo"][:5]}')
            n = (lib.vitae_conv3d_packed_elems_x3 if e['form'] & FORM_X3 else lib.vitae_conv3d_packed_elems)(*e['geo'][:5], e['form'] & 1)
            if e['data'] is None or e['data'].numel() != n or e['data'].device != device:
                e['data'] = torch.empty(n, dtype=BF16, device=device)
            rows.append((w.data_ptr(), e['data'].data_ptr(), *e['geo']))
        n, ew = len(rows), CONSTS['VITAE_CONV3D_PACK_ENTRY_WORDS']
        table = np.array(rows, dtype=np.int64).reshape(n, ew)
        chunks = int(lib.vitae_conv3d_pack_multi_chunks(table.ctypes.data, n))
        if chunks <= 0:
            raise VitaeError('vitae_conv3d_pack_weights_multi refuses this set of convolutions (geometry, alignment or total size)')
        # fresh buffers each time (a launch already enqueued may still read the old ones); [table | chunk list (int32 pairs)]
        pinned = torch.empty(n * ew + chunks, dtype=torch.int64, pin_memory=True)
        pinned.numpy()[:n * ew] = table.reshape(-1)
        th = pinned.data_ptr()
        lib.vitae_conv3d_pack_multi_chunk_list(th, n, th + 8 * n * ew, chunks)
        dev = torch.empty(n * ew + chunks, dtype=torch.int64, device=device)
        dev.copy_(pinned, non_blocking=True)
        td = dev.data_ptr()
        self.table_builds += 1
        # a weight that had to be copied to be contiguous lives in `weights` only: such a table is never found again (sig None)
        copied = any(w.data_ptr() != key[0] for (_, key), w in zip(stale, weights))
        return dict(sig=None if copied else sig, pinned=pinned, dev=dev, n=n, chunks=chunks, th=th, td=td, ch=th + 8 * n * ew, cd=td + 8 * n * ew)


def _no_store():
    return None


def pack_store_of(model):
    """The ``ConvPackStore`` of ``model`` (a ResNet), made on first use."""
    st = model.__dict__.get('_conv_packs')
    if st is None or st.model() is not model:
        st = model.__dict__['_conv_packs'] = ConvPackStore(model)
    return st


def _rows_dtype(t, x3, what):
    want = F32 if x3 else BF16
    if t.dtype != want:
        raise VitaeError(f'{what}: the {"fp32x3" if x3 else "bf16"} route reads {want} rows, got {t.dtype}')


def conv_fwd(x16, N, vol, conv, packs=None, x3=False):
    """-> fp32 [M, Cout], output volume.  ``x16``: the channels-last rows in bf16 (``x3``: in fp32, split by the kernel)"""
    _rows_dtype(x16, x3, 'conv_fwd')
    ovol = conv_out_vol(vol, conv)
    y = torch.empty(N * ovol[0] * ovol[1] * ovol[2], conv.out_channels, dtype=F32, device=x16.device)
    fn = lib.vitae_conv3d_fwd_x3 if x3 else lib.vitae_conv3d_fwd
    fn(x16.data_ptr(), pack_weight(conv, 0, packs, x3).data_ptr(), y.data_ptr(), None, *_geo(N, vol, conv), _st(x16))
    return y, ovol


def conv_bwd_input(dy16, N, vol, conv, into=None, packs=None, x3=False):
    """dx fp32 [N D H W, Cin]; `into`: the sum is added to that tensor (the residual branch's gradient) instead"""
    _rows_dtype(dy16, x3, 'conv_bwd_input')
    dx = into if into is not None else torch.empty(N * vol[0] * vol[1] * vol[2], conv.in_channels, dtype=F32, device=dy16.device)
    fn = lib.vitae_conv3d_bwd_input_x3 if x3 else lib.vitae_conv3d_bwd_input
    fn(dy16.data_ptr(), pack_weight(conv, 1, packs, x3).data_ptr(), dx.data_ptr(), None, 0 if into is None else 1, *_geo(N, vol, conv), _st(dy16))
    return dx


def conv_bwd_weight(dy16, x16, N, vol, conv, x3=False):
    _rows_dtype(dy16, x3, 'conv_bwd_weight')
    _rows_dtype(x16, x3, 'conv_bwd_weight')
    geo = _geo(N, vol, conv)
    n = lib.vitae_conv3d_wgrad_ws_floats(*geo)
    ws = torch.empty(n, dtype=F32, device=dy16.device)
    dw = torch.empty_like(conv.weight, dtype=F32, memory_format=torch.contiguous_format)
    fn = lib.vitae_conv3d_bwd_weight_x3 if x3 else lib.vitae_conv3d_bwd_weight
    fn(dy16.data_ptr(), x16.data_ptr(), dw.data_ptr(), ws.data_ptr(), n, 0, *geo, _st(dy16))
    return dw


def _bn_operands(bn):
    if bn.momentum is None or not bn.affine or not bn.track_running_stats:
        raise NotImplementedError('BatchNorm3d: only affine layers with running statistics and a fixed momentum are built')
    return _param(bn.weight, 'a BatchNorm weight'), _param(bn.bias, 'a BatchNorm bias')


def bn_tail_train(x, res, bn, relu, want16):
    """y = [relu](bn(x) [+ res]) on batch statistics; updates the running statistics -> y, y16 | None, mean, rstd"""
    R, C = x.shape
    w, b = _bn_operands(bn)
    y = torch.empty_like(x)
    y16 = torch.empty(R, C, dtype=BF16, device=x.device) if want16 else None
    mean, rstd = torch.empty(C, dtype=F32, device=x.device), torch.empty(C, dtype=F32, device=x.device)
    ws = torch.empty(lib.vitae_bn1d_split_ws_floats(R, C), dtype=F32, device=x.device)
    lib.vitae_bn_tail_fwd_split(x.data_ptr(), _p(res), w.data_ptr(), b.data_ptr(), y.data_ptr(), _p(y16), mean.data_ptr(), rstd.data_ptr(),
                                bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.num_batches_tracked.data_ptr(), R, C, bn.eps,
                                bn.momentum, relu, ws.data_ptr(), _st(x))
    return y, y16, mean, rstd


def bn_tail_eval(x, res, bn, relu, want16):
    R, C = x.shape
    w, b = _bn_operands(bn)
    y = torch.empty_like(x)
    y16 = torch.empty(R, C, dtype=BF16, device=x.device) if want16 else None
    lib.vitae_bn_tail_eval(x.data_ptr(), _p(res), w.data_ptr(), b.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(), y.data_ptr(),
                           _p(y16), R, C, bn.eps, relu, _st(x))
    return y, y16


def bn_tail_bwd(dy, x, y, bn, mean, rstd, relu, dres=None, want16=True):
    """-> dx16 (the next convolution gradient's operand; without ``want16`` the fp32 dx itself, no bf16 copy is written), dw, db;
    dres (optional) receives the masked gradient"""
    R, C = x.shape
    w, _ = _bn_operands(bn)
    dx = torch.empty_like(x)
    dx16 = torch.empty(R, C, dtype=BF16, device=x.device) if want16 else None
    dw, db = torch.zeros(C, dtype=F32, device=x.device), torch.zeros(C, dtype=F32, device=x.device)       # the kernel adds to them
    ws = torch.empty(lib.vitae_bn1d_split_ws_floats(R, C), dtype=F32, device=x.device)
    lib.vitae_bn_tail_bwd_split(dy.data_ptr(), x.data_ptr(), _p(y) if relu else None, w.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                                _p(dx16), _p(dres), dw.data_ptr(), db.data_ptr(), R, C, relu, ws.data_ptr(), _st(x))
    return (dx16 if want16 else dx), dw, db


class HipResNetRunner:
    """Sequences the kernels over a ``k_fold_training_scripts.resnet_3d.ResNet`` (its modules hold the parameters and buffers).  The
    route follows ``model.precision``.  Below, a name ending in 16 is the operand a convolution reads: the bf16 copy on the bf16
    route, the fp32 tensor itself under ``fp32x3`` (no copy exists there)."""

    def __init__(self, model):
        self.model = model
        self.packs = pack_store_of(model)
        self.x3 = check_precision(getattr(model, 'precision', 'bf16')) == 'fp32x3'

    def blocks(self):
        for li in range(1, 5):
            for bi, blk in enumerate(getattr(self.model, f'layer{li}')):
                yield f'layer{li}.{bi}', blk

    # ------------------------------------------------------------------ forward
    def _forward(self, x, train, keep=None):
        """-> features fp32 [N, C] and (keep; default: train) what the backward needs.  train: BatchNorm on batch statistics, the running
        statistics updated.  Without ``keep`` no record is collected: an activation is released as soon as the sequence has passed it."""
        m, packs, x3 = self.model, self.packs, self.x3
        keep = train if keep is None else keep
        if keep and not train:
            raise VitaeError('ResNet: the backward needs the batch statistics; the inference route keeps nothing')
        if not x.is_cuda:
            raise VitaeError(f'ResNet: input is on {x.device}; this package computes on MI355X only (no CPU fallback).')
        if x.dim() != 5 or x.shape[1] != m.conv1.in_channels:
            raise VitaeError(f'ResNet: expected [N, {m.conv1.in_channels}, D, H, W], got {tuple(x.shape)}')
        bn_route = bn_tail_train if train else (lambda x_, res, bn_, relu, want16: bn_tail_eval(x_, res, bn_, relu, want16) + (None, None))

        def bn(x_, res, bn_, relu, want16):             # -> y, the next convolution's operand (None: not wanted), mean, rstd
            y_, y16_, mean_, rstd_ = bn_route(x_, res, bn_, relu, want16 and not x3)
            return y_, (y_ if x3 and want16 else y16_), mean_, rstd_
        x = x.detach().contiguous().float()
        N, C, vol0 = x.shape[0], x.shape[1], tuple(x.shape[2:])
        st, dev = _st(x), x.device
        x16 = torch.empty(N * vol0[0] * vol0[1] * vol0[2], C, dtype=F32 if x3 else BF16, device=dev)
        (lib.vitae_to_channels_last_f32 if x3 else lib.vitae_to_channels_last_bf16)(x.data_ptr(), x16.data_ptr(), N, C, *vol0, st)
        pre, vol = conv_fwd(x16, N, vol0, m.conv1, packs=packs, x3=x3)
        y, y16, mean, rstd = bn(pre, None, m.bn1, 1, m.no_max_pool)
        stem = dict(x16=x16, vol_in=vol0, pre=pre, y=y, mean=mean, rstd=rstd, vol=vol, idx=None) if keep else None
        cur, cur16 = y, y16
        del x, x16, pre, mean, rstd
        if not m.no_max_pool:
            C0 = y.shape[1]
            pvol = tuple((v - 1) // 2 + 1 for v in vol)
            rows = N * pvol[0] * pvol[1] * pvol[2]
            cur = torch.empty(rows, C0, dtype=F32, device=dev)
            cur16 = cur if x3 else torch.empty(rows, C0, dtype=BF16, device=dev)
            idx = torch.empty(rows, C0, dtype=torch.uint8, device=dev)
            lib.vitae_maxpool3d_fwd(y.data_ptr(), cur.data_ptr(), None if x3 else cur16.data_ptr(), idx.data_ptr(), N, *vol, C0, st)
            if keep:
                stem['idx'] = idx
            vol = pvol
            del idx
        del y, y16
        recs = []
        for _, blk in self.blocks():
            pre1, ovol = conv_fwd(cur16, N, vol, blk.conv1, packs=packs, x3=x3)
            y1, y1_16, mean1, rstd1 = bn(pre1, None, blk.bn1, 1, True)
            pre2, _ = conv_fwd(y1_16, N, ovol, blk.conv2, packs=packs, x3=x3)
            rec = dict(in16=cur16, vol_in=vol, vol=ovol, pre1=pre1, y1=y1, y1_16=y1_16, mean1=mean1, rstd1=rstd1, pre2=pre2)
            del pre1, y1, y1_16
            if blk.downsample is not None:
                pred, _ = conv_fwd(cur16, N, vol, blk.downsample[0], packs=packs, x3=x3)
                res, _, meand, rstdd = bn(pred, None, blk.downsample[1], 0, False)
                rec.update(pred=pred, meand=meand, rstdd=rstdd)
                del pred
            else:
                res = cur
            cur, cur16, mean2, rstd2 = bn(pre2, res, blk.bn2, 1, True)
            rec.update(out=cur, mean2=mean2, rstd2=rstd2)
            del pre2, res
            if keep:
                recs.append(rec)
            del rec
            vol = ovol
        S, Cl = vol[0] * vol[1] * vol[2], cur.shape[1]
        feat = torch.empty(N, Cl, dtype=F32, device=dev)
        lib.vitae_rows_mean_fwd(cur.data_ptr(), feat.data_ptr(), None, N, S, Cl, st)
        return feat, (dict(N=N, S=S, stem=stem, recs=recs, x3=x3) if keep else None)

    def infer(self, x):
        return self._forward(x, False)[0]

    def forward_batch_stats(self, x):
        """The training arithmetic (batch statistics, running statistics and ``num_batches_tracked`` updated) with nothing kept: what a
        momentum encoder in ``train()`` mode under ``no_grad`` computes."""
        return self._forward(x, True, keep=False)[0]

    def forward_keep(self, x):
        return self._forward(x, True)

    # ------------------------------------------------------------------ backward
    def backward(self, kept, dfeat):
        """-> {parameter name: gradient} of everything below the head; the input volume gets none"""
        m, N, S, x3 = self.model, kept['N'], kept['S'], kept['x3']          # the route of the forward that kept the activations
        w16 = not x3
        grads = {}
        dfeat = dfeat.contiguous().float()
        Cl = dfeat.shape[1]
        dcur = torch.empty(N * S, Cl, dtype=F32, device=dfeat.device)
        lib.vitae_rows_mean_bwd(dfeat.data_ptr(), dcur.data_ptr(), None, N, S, Cl, _st(dfeat))
        for (name, blk), rec in reversed(list(zip(self.blocks(), kept['recs']))):
            vin, vout = rec['vol_in'], rec['vol']
            identity = blk.downsample is None
            dres = torch.empty_like(rec['out'])                        # identity shortcut: this IS the block input's gradient buffer
            d2_16, grads[f'{name}.bn2.weight'], grads[f'{name}.bn2.bias'] = bn_tail_bwd(dcur, rec['pre2'], rec['out'], blk.bn2, rec['mean2'],
                                                                                      rec['rstd2'], 1, dres, want16=w16)
            grads[f'{name}.conv2.weight'] = conv_bwd_weight(d2_16, rec['y1_16'], N, vout, blk.conv2, x3=x3)
            dy1 = conv_bwd_input(d2_16, N, vout, blk.conv2, packs=self.packs, x3=x3)
            d1_16, grads[f'{name}.bn1.weight'], grads[f'{name}.bn1.bias'] = bn_tail_bwd(dy1, rec['pre1'], rec['y1'], blk.bn1, rec['mean1'],
                                                                                      rec['rstd1'], 1, want16=w16)
            grads[f'{name}.conv1.weight'] = conv_bwd_weight(d1_16, rec['in16'], N, vin, blk.conv1, x3=x3)
            if identity:
                din = dres
            else:
                dd_16, grads[f'{name}.downsample.1.weight'], grads[f'{name}.downsample.1.bias'] = bn_tail_bwd(
                    dres, rec['pred'], None, blk.downsample[1], rec['meand'], rec['rstdd'], 0, want16=w16)
                grads[f'{name}.downsample.0.weight'] = conv_bwd_weight(dd_16, rec['in16'], N, vin, blk.downsample[0], x3=x3)
                din = conv_bwd_input(dd_16, N, vin, blk.downsample[0], packs=self.packs, x3=x3)
            dcur = conv_bwd_input(d1_16, N, vin, blk.conv1, into=din, packs=self.packs, x3=x3)
        stem = kept['stem']
        if stem['idx'] is not None:
            dy = torch.empty_like(stem['y'])
            lib.vitae_maxpool3d_bwd(dcur.data_ptr(), stem['idx'].data_ptr(), dy.data_ptr(), None, N, *stem['vol'], dy.shape[1], _st(dy))
            dcur = dy
        d16, grads['bn1.weight'], grads['bn1.bias'] = bn_tail_bwd(dcur, stem['pre'], stem['y'], m.bn1, stem['mean'], stem['rstd'], 1, want16=w16)
        grads['conv1.weight'] = conv_bwd_weight(d16, stem['x16'], N, stem['vol_in'], m.conv1, x3=x3)      # the input volume has no gradient
        return grads
