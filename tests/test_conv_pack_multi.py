"""``vitae_conv3d_pack_weights_multi`` (every convolution operand of a network in one launch) and ``resnet.ConvPackStore``.

Kernel: every destination must EQUAL what ``vitae_conv3d_pack_weight`` writes for the same weight, bit for bit — zero tail of each row,
NaN, infinities, -0 and denormals in the weight included.  All destinations of a table lie in one arena filled with a sentinel bit
pattern, 64 elements of it in front of and behind each: whatever the launch writes outside a destination shows.  Tables: one entry
smaller than a chunk; the 23 operands of the micro ResNet-10; entries whose boundaries fall inside a chunk (sizes 1408, 5504, 5504,
128, 64, 896, 896 elements against a chunk of 4096).  Every refusal leaves the arena untouched.

Store: operands are re-packed exactly when a weight's ``(data_ptr, _version)`` changed — counted on the store, not timed — and with
the store switched off (``VITAE_CONV_PACK_STORE=0``) a training step gives the same bits."""
import copy
from functools import partial

import numpy as np
import pytest
import torch

F32, BF16 = torch.float32, torch.bfloat16
GUARD, SENT = 64, 0x7FC1          # a NaN pattern no conversion produces from these weights
KW = dict(n_input_channels=1, widen_factor=0.0625)


def geo(cout, cin, k, transposed):
    return (cout, cin, *((k,) * 3 if isinstance(k, int) else k), transposed)


SMALL = [geo(4, 4, 1, 0)]                                            # 4 rows x 16 = 64 elements
BOUNDARIES = [geo(4, 1, 7, 0),                                       # K = 343, Kpad 352
              geo(4, 4, 7, 0), geo(4, 4, 7, 1),                      # K = 1372, Kpad 1376: crosses the first chunk edge
              geo(8, 4, 1, 0), geo(8, 4, 1, 1),                      # K = 4: 12 zeros per row / K = 8
              geo(8, 4, 3, 0), geo(8, 4, 3, 1)]                      # Cout != Cin: K = 108 -> 112 / K = 216 -> 224; holds the second edge


def micro_geos():
    from vit_ae_plus_plus_amd.k_fold_training_scripts.resnet_3d import generate_model
    m = generate_model(10, n_classes=2, **KW)
    out = []
    for c in m.modules():
        if isinstance(c, torch.nn.Conv3d):
            for t in ((0,) if c is m.conv1 else (0, 1)):
                out.append((c.out_channels, c.in_channels, *c.kernel_size, t))
    return out


# ---------------------------------------------------------------------------- CPU
def test_prototypes_constants_and_host_helpers():
    from vit_ae_plus_plus_amd import _abi
    assert _abi.CONSTS['VITAE_ABI_VERSION'] == 57
    for name, nargs in (('vitae_conv3d_pack_weights_multi', 7), ('vitae_conv3d_pack_multi_chunks', 2), ('vitae_conv3d_pack_multi_chunk_list', 4)):
        assert name in _abi.PROTOS and len(_abi.PROTOS[name][1]) == nargs
    assert _abi.PROTOS['vitae_conv3d_pack_weights_multi'][1] == ['ptr', 'ptr', 'long', 'ptr', 'ptr', 'long', 'ptr']
    C = _abi.CONSTS
    assert C['VITAE_CONV3D_PACK_ENTRY_WORDS'] == 8 and C['VITAE_CONV3D_PACK_CHUNK'] % 16 == 0 and C['VITAE_CONV3D_PACK_MAX_ELEMS'] == 1 << 33
    assert len(micro_geos()) == 23
    # the host side alone (no device is touched): chunk count and chunk list of a table, refusals by a count of 0
    lib, chunk = _abi.lib, C['VITAE_CONV3D_PACK_CHUNK']
    table = np.array([(4096, 8192 + 16 * i, *g) for i, g in enumerate(BOUNDARIES)], dtype=np.int64)
    sizes = [int(lib.vitae_conv3d_packed_elems(*g)) for g in BOUNDARIES]
    assert sizes == [1408, 5504, 5504, 128, 64, 896, 896]
    n = int(lib.vitae_conv3d_pack_multi_chunks(table.ctypes.data, len(table)))
    assert n == -(-sum(sizes) // chunk) == 4
    chunks = np.full((n, 2), -1, dtype=np.int32)
    lib.vitae_conv3d_pack_multi_chunk_list(table.ctypes.data, len(table), chunks.ctypes.data, n)
    starts = np.cumsum([0] + sizes)
    for c in range(n):
        e = int(np.searchsorted(starts, c * chunk, side='right')) - 1
        assert chunks[c].tolist() == [e, (c * chunk - starts[e]) // 8], c
    with pytest.raises(_abi.VitaeError):
        lib.vitae_conv3d_pack_multi_chunk_list(table.ctypes.data, len(table), chunks.ctypes.data, n + 1)
    for bad in (dict(n=0), dict(col=0, val=0), dict(col=1, val=0), dict(col=1, val=8200), dict(col=2, val=6), dict(col=3, val=0),
                dict(col=4, val=8), dict(col=7, val=2), dict(col=2, val=1 << 22, col2=3, val2=1 << 12)):
        t = table.copy()
        if 'col' in bad:
            t[1, bad['col']] = bad['val']
        if 'col2' in bad:
            t[1, bad['col2']] = bad['val2']
        assert lib.vitae_conv3d_pack_multi_chunks(t.ctypes.data, bad.get('n', len(t))) == 0, bad


# ---------------------------------------------------------------------------- GPU: the kernel
def weights_for(geos, seed):
    g = torch.Generator().manual_seed(seed)
    ws = []
    for i, (cout, cin, kd, kh, kw, _) in enumerate(geos):
        w = torch.randn(cout, cin, kd, kh, kw, generator=g)
        flat = w.view(-1)
        special = [float('nan'), float('inf'), -float('inf'), -0.0, 1e-40, 1.00390625, 1.01171875]      # the last two: ties of the rounding
        for j, v in enumerate(special):
            flat[(7 * i + 3 * j) % flat.numel()] = v
        ws.append(w.cuda())
    return ws


class Arena:
    """All destinations of one table in one bf16 buffer of sentinels, GUARD elements around each (offsets 16-byte aligned)."""

    def __init__(self, sizes):
        self.offsets, pos = [], GUARD
        for n in sizes:
            self.offsets.append(pos)
            pos += n + GUARD
            pos = -(-pos // 8) * 8
        self.sizes = sizes
        self.buf = torch.full((pos,), SENT, dtype=torch.int16, device='cuda')
        self.mask = torch.ones(pos, dtype=torch.bool, device='cuda')
        for o, n in zip(self.offsets, sizes):
            self.mask[o:o + n] = False

    def ptr(self, i):
        return self.buf.data_ptr() + 2 * self.offsets[i]

    def dest(self, i):
        return self.buf[self.offsets[i]:self.offsets[i] + self.sizes[i]]

    def guards_intact(self):
        return bool((self.buf[self.mask] == SENT).all())

    def untouched(self):
        return bool((self.buf == SENT).all())


def launch_multi(lib, table, chunks=None, n_entries=None, n_chunks=None):
    """table: int64 [n, 8] -> runs the entry point with host and device copies of table and chunk list"""
    n = len(table) if n_entries is None else n_entries
    if chunks is None:
        nc = int(lib.vitae_conv3d_pack_multi_chunks(table.ctypes.data, len(table)))
        assert nc > 0
        chunks = np.zeros((nc, 2), dtype=np.int32)
        lib.vitae_conv3d_pack_multi_chunk_list(table.ctypes.data, len(table), chunks.ctypes.data, nc)
    td = torch.from_numpy(table.copy()).cuda()
    cd = torch.from_numpy(chunks.copy()).cuda()
    lib.vitae_conv3d_pack_weights_multi(table.ctypes.data, td.data_ptr(), n, chunks.ctypes.data, cd.data_ptr(),
                                        len(chunks) if n_chunks is None else n_chunks, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return chunks


def single_pack(lib, w, g):
    n = int(lib.vitae_conv3d_packed_elems(*g))
    out = torch.full((n + GUARD,), SENT, dtype=torch.int16, device='cuda')
    lib.vitae_conv3d_pack_weight(w.data_ptr(), out.data_ptr(), *g, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((out[n:] == SENT).all())
    return out[:n]


def make_table(lib, geos, seed):
    ws = weights_for(geos, seed)
    arena = Arena([int(lib.vitae_conv3d_packed_elems(*g)) for g in geos])
    table = np.array([(w.data_ptr(), arena.ptr(i), *g) for i, (w, g) in enumerate(zip(ws, geos))], dtype=np.int64)
    return ws, arena, table


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['small', 'micro_resnet10', 'boundaries'])
def test_multi_equals_the_single_pack_bit_for_bit(name):
    from vit_ae_plus_plus_amd._abi import CONSTS, lib
    geos = {'small': SMALL, 'micro_resnet10': micro_geos(), 'boundaries': BOUNDARIES}[name]
    ws, arena, table = make_table(lib, geos, 5)
    chunks = launch_multi(lib, table)
    total = sum(arena.sizes)
    assert len(chunks) == -(-total // CONSTS['VITAE_CONV3D_PACK_CHUNK'])
    if name == 'small':
        assert total < CONSTS['VITAE_CONV3D_PACK_CHUNK'] and len(chunks) == 1
    else:
        assert len(chunks) > 1 and any(int(o) != 0 for _, o in chunks[1:])          # a chunk begins inside an entry
    assert arena.guards_intact()
    for i, (w, g) in enumerate(zip(ws, geos)):
        want = single_pack(lib, w, g)
        got = arena.dest(i)
        assert torch.equal(got, want), (name, i, g, int((got != want).sum()))
        rows = g[1] if g[5] else g[0]
        K = g[2] * g[3] * g[4] * (g[0] if g[5] else g[1])
        tail = got.view(rows, -1)[:, K:]
        assert bool((tail == 0).all()), (name, i)                                   # +0.0 in every tail element
    launch_multi(lib, table)                                                        # repeats are bit-equal
    assert all(torch.equal(arena.dest(i), single_pack(lib, w, g)) for i, (w, g) in enumerate(zip(ws, geos)))


@pytest.mark.gpu
def test_refusals_write_nothing():
    from vit_ae_plus_plus_amd._abi import VitaeError, lib
    ws, arena, table = make_table(lib, BOUNDARIES, 6)
    nc = int(lib.vitae_conv3d_pack_multi_chunks(table.ctypes.data, len(table)))
    good = np.zeros((nc, 2), dtype=np.int32)
    lib.vitae_conv3d_pack_multi_chunk_list(table.ctypes.data, len(table), good.ctypes.data, nc)

    def edited(col, val, row=2, col2=None, val2=None):
        t = table.copy()
        t[row, col] = val
        if col2 is not None:
            t[row, col2] = val2
        return t

    cases = {
        'n = 0': dict(table=table, n_entries=0, err='INVALID_ARG'),
        'n < 0': dict(table=table, n_entries=-3, err='INVALID_ARG'),
        'null source': dict(table=edited(0, 0), err='INVALID_ARG'),
        'null destination': dict(table=edited(1, 0), err='INVALID_ARG'),
        'destination not 16-byte aligned': dict(table=edited(1, int(table[2, 1]) + 8), err='UNSUPPORTED_SHAPE'),
        'kernel extent 8': dict(table=edited(4, 8), err='UNSUPPORTED_SHAPE'),
        'kernel extent 0': dict(table=edited(6, 0), err='UNSUPPORTED_SHAPE'),
        'Cout % 4': dict(table=edited(2, 6), err='UNSUPPORTED_SHAPE'),
        'Cin = 0': dict(table=edited(3, 0), err='INVALID_ARG'),
        'transposed = 2': dict(table=edited(7, 2), err='INVALID_ARG'),
        'total beyond the index type': dict(table=edited(2, 1 << 22, col2=3, val2=1 << 12), err='UNSUPPORTED_SHAPE'),
        'one chunk too few': dict(table=table, n_chunks=nc - 1, err='INVALID_ARG'),
        'one chunk too many': dict(table=table, chunks=np.concatenate([good, good[-1:]]), err='INVALID_ARG'),
        'a chunk that begins elsewhere': dict(table=table, chunks=np.concatenate([good[:1], good[1:] + np.array([[0, 1]], dtype=np.int32)]),
                                              err='INVALID_ARG'),
    }
    for what, c in cases.items():
        with pytest.raises(VitaeError, match=c['err']):
            launch_multi(lib, c['table'], chunks=c.get('chunks', good), n_entries=c.get('n_entries'), n_chunks=c.get('n_chunks'))
        torch.cuda.synchronize()
        assert arena.untouched(), what
    st = torch.cuda.current_stream().cuda_stream
    td, cd = torch.from_numpy(table.copy()).cuda(), torch.from_numpy(good.copy()).cuda()
    for args in ((None, td.data_ptr(), len(table), good.ctypes.data, cd.data_ptr(), nc, st),
                 (table.ctypes.data, None, len(table), good.ctypes.data, cd.data_ptr(), nc, st),
                 (table.ctypes.data, td.data_ptr(), len(table), None, cd.data_ptr(), nc, st),
                 (table.ctypes.data, td.data_ptr(), len(table), good.ctypes.data, None, nc, st)):
        with pytest.raises(VitaeError, match='INVALID_ARG'):
            lib.vitae_conv3d_pack_weights_multi(*args)
    torch.cuda.synchronize()
    assert arena.untouched()
    launch_multi(lib, table, chunks=good)                                           # and the accepted call does write
    assert arena.guards_intact() and not arena.untouched()


# ---------------------------------------------------------------------------- GPU: the store
def micro_resnet():
    from vit_ae_plus_plus_amd.k_fold_training_scripts.resnet_3d import generate_model
    torch.manual_seed(3)
    return generate_model(10, n_classes=2, **KW).cuda().train()


def check_operands(model, store):
    """every stored operand equals a fresh single pack of the weight as it is now"""
    from vit_ae_plus_plus_amd import resnet as R
    n = 0
    for conv in model.modules():
        if isinstance(conv, torch.nn.Conv3d):
            for t in ((0,) if conv is model.conv1 else (0, 1)):
                got = store.operand(conv, t)
                assert torch.equal(got.view(torch.int16), R.pack_weight(conv, t).view(torch.int16)), (t, tuple(conv.weight.shape))
                n += 1
    return n


@pytest.mark.gpu
def test_store_repacks_exactly_when_a_weight_changed():
    from vit_ae_plus_plus_amd import resnet as R
    from vit_ae_plus_plus_amd.other_baselines.mocov3.moco.optimizer import LARS
    m = micro_resnet()
    store = R.pack_store_of(m)
    assert R.pack_store_of(m) is store and R.HipResNetRunner(m).packs is store
    x = torch.randn(2, 1, 16, 16, 16, device='cuda')
    y = torch.tensor([0, 1], device='cuda')

    def step():
        m.zero_grad()
        torch.nn.functional.cross_entropy(m(x), y).backward()

    step()
    assert (store.launches, store.table_builds) == (1, 1)                           # all 23 operands, both forms, in the first launch
    assert check_operands(m, store) == 23 and store.launches == 1
    step()
    with torch.no_grad():
        m.eval()(x)
        m.train()
    assert (store.launches, store.table_builds) == (1, 1)                           # nothing changed: nothing packed
    for what, write in (('Adam', lambda: torch.optim.Adam(m.parameters(), lr=1e-2).step()),
                        ('LARS', lambda: LARS(m.parameters(), lr=0.1, weight_decay=1e-6).step()),
                        ('load_state_dict', lambda: m.load_state_dict({k: v * 1.5 if v.is_floating_point() else v
                                                                       for k, v in m.state_dict().items()}))):
        before = (store.launches, store.table_builds)
        step()                                                                      # gradients for the optimisers; packs are current
        assert (store.launches, store.table_builds) == before, what
        write()
        step()
        assert (store.launches, store.table_builds) == (before[0] + 1, before[1]), what      # one launch, the same table
        check_operands(m, store)
        assert store.launches == before[0] + 1, what
    # one weight edited in place: one launch, of a table with two entries (its two forms)
    before = (store.launches, store.table_builds)
    with torch.no_grad():
        m.layer2[0].conv2.weight.mul_(0.5)
    step()
    assert (store.launches, store.table_builds) == (before[0] + 1, before[1] + 1)
    check_operands(m, store)
    # a parameter that moved: new addresses, a new table
    before = (store.launches, store.table_builds)
    m.conv1.weight.data = m.conv1.weight.data.clone()
    step()
    assert (store.launches, store.table_builds) == (before[0] + 1, before[1] + 1)
    check_operands(m, store)
    # a copy of the model gets a store of its own
    m2 = copy.deepcopy(m)
    assert R.pack_store_of(m2) is not store and R.pack_store_of(m2).launches == 0


@pytest.mark.gpu
def test_store_follows_the_momentum_update():
    from vit_ae_plus_plus_amd import resnet as R
    from vit_ae_plus_plus_amd.other_baselines.mocov3.moco import builder, resent3d_base
    torch.manual_seed(4)
    model = builder.MoCo_ResNet(partial(resent3d_base.generate_model, model_depth=10, **KW), 16, 64, 1.0).cuda().train()
    x1, x2 = torch.randn(4, 1, 16, 16, 16, device='cuda'), torch.randn(4, 1, 16, 16, 16, device='cuda')
    with torch.no_grad():
        for p in model.base_encoder.parameters():                                   # so that the update changes the momentum encoder
            p.add_(0.01)
    sb, sm = R.pack_store_of(model.base_encoder), R.pack_store_of(model.momentum_encoder)
    model(x1, x2, 0.9).backward()
    assert (sb.launches, sm.launches) == (1, 1)                                     # two views, one pack per encoder
    check_operands(model.momentum_encoder, sm)
    model(x1, x2, 0.9).backward()
    assert (sb.launches, sm.launches) == (1, 2) and sm.table_builds == 1            # the update bumped the versions; the base is unchanged
    check_operands(model.momentum_encoder, sm)
    check_operands(model.base_encoder, sb)
    assert (sb.launches, sm.launches) == (1, 2)


@pytest.mark.gpu
def test_same_bits_with_the_store_off(monkeypatch):
    from vit_ae_plus_plus_amd import resnet as R
    from vit_ae_plus_plus_amd.other_baselines.mocov3.moco import builder, resent3d_base
    x = torch.randn(4, 1, 16, 16, 16, device='cuda')
    x2 = x + 0.3 * torch.randn_like(x)
    y = torch.tensor([0, 1, 1, 0], device='cuda')
    m0 = micro_resnet()
    torch.manual_seed(4)
    moco0 = builder.MoCo_ResNet(partial(resent3d_base.generate_model, model_depth=10, **KW), 16, 64, 0.2).cuda().train()
    results = {}
    for flag in ('0', '1'):
        monkeypatch.setenv('VITAE_CONV_PACK_STORE', flag)
        assert R.pack_store_enabled() == (flag == '1')
        m, moco = copy.deepcopy(m0), copy.deepcopy(moco0)
        logits = m(x)
        torch.nn.functional.cross_entropy(logits, y).backward()
        loss = moco(x, x2, 0.99)
        loss.backward()
        torch.cuda.synchronize()
        assert R.pack_store_of(m).launches == (1 if flag == '1' else 0)
        results[flag] = (logits.detach(), loss.detach(), [p.grad for p in m.parameters()],
                         [p.grad for p in moco.parameters() if p.requires_grad], [b.clone() for b in moco.buffers()])
    a, b = results['0'], results['1']
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for i in (2, 3, 4):
        assert len(a[i]) == len(b[i]) and all(torch.equal(u, v) for u, v in zip(a[i], b[i]))
