"""One SHA-256 per output of the convolution family, on fixed operands: do two builds of the library write the same bytes?

    VITAE_HIP_LIB=/path/to/one/libvitae_hip.so   python tools/conv_bits.py > one.txt
    VITAE_HIP_LIB=/path/to/other/libvitae_hip.so python tools/conv_bits.py > other.txt        then: diff one.txt other.txt

The kernels are deterministic (ordered sums, no float atomics), so a change that leaves them alone leaves every line alone.  The
shapes are the case tables of tests/test_resnet3d_kernels.py and tests/test_resnet3d_x3_kernels.py and the several-chunk weight
gradient of each; every case runs on both routes (bf16, fp32x3): packing (single launch and table launch, both orientations),
channels-last, forward, input gradient without and with accumulate, weight gradient without and with accumulate."""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import test_resnet3d_kernels as TB  # noqa: E402
import test_resnet3d_x3_kernels as TX  # noqa: E402
from vit_ae_plus_plus_amd import _abi  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32
lib = _abi.lib


def sha(t: torch.Tensor) -> str:
    torch.cuda.synchronize()
    t = t.contiguous().cpu()
    return hashlib.sha256(t.view(torch.int16 if t.dtype == BF16 else torch.int32).numpy().tobytes()).hexdigest()


def run(label: str, c: dict, seed: int, x3: bool, only_dw: bool = False) -> None:
    g = torch.Generator().manual_seed(seed)
    st = torch.cuda.current_stream().cuda_stream
    N, Cin, Cout, vol, ovol = c['N'], c['Cin'], c['Cout'], c['vol'], TB.out_vol(c)
    geo = TB.geo_args(c)
    M, V = N * int(np.prod(ovol)), N * int(np.prod(vol))
    sfx, src_dt = ('_x3', F32) if x3 else ('', BF16)
    fn = lambda name: getattr(lib, name + sfx)        # noqa: E731
    say = lambda what, t: print(f'{label} {"fp32x3" if x3 else "bf16"} {what} {sha(t)}')      # noqa: E731
    x = torch.randn(N, Cin, *vol, generator=g).cuda()
    w = (torch.randn(Cout, Cin, *c['k'], generator=g) * 0.1).cuda()
    dy = TB.cl(torch.randn(N, Cout, *ovol, generator=g)).to(src_dt).cuda()
    xs = torch.empty(V, Cin, dtype=src_dt, device='cuda')
    (lib.vitae_to_channels_last_f32 if x3 else lib.vitae_to_channels_last_bf16)(x.data_ptr(), xs.data_ptr(), N, Cin, *vol, st)
    if not only_dw:
        say('channels_last', xs)
        wgeo = (Cout, Cin, *c['k'])
        packed = [torch.empty(fn('vitae_conv3d_packed_elems')(*wgeo, tr), dtype=BF16, device='cuda') for tr in (0, 1)]
        multi = [torch.empty_like(p) for p in packed]
        for tr in (0, 1):
            fn('vitae_conv3d_pack_weight')(w.data_ptr(), packed[tr].data_ptr(), *wgeo, tr, st)
            say(f'pack{tr}', packed[tr])
        table = np.array([(w.data_ptr(), multi[tr].data_ptr(), *wgeo, tr | (4 if x3 else 0)) for tr in (0, 1)], dtype=np.int64)
        nc = int(lib.vitae_conv3d_pack_multi_chunks(table.ctypes.data, 2))
        chunks = np.zeros((nc, 2), dtype=np.int32)
        lib.vitae_conv3d_pack_multi_chunk_list(table.ctypes.data, 2, chunks.ctypes.data, nc)
        td, cd = torch.from_numpy(table.copy()).cuda(), torch.from_numpy(chunks.copy()).cuda()
        lib.vitae_conv3d_pack_weights_multi(table.ctypes.data, td.data_ptr(), 2, chunks.ctypes.data, cd.data_ptr(), nc, st)
        for tr in (0, 1):
            say(f'pack_multi{tr}', multi[tr])
        y, y16 = torch.empty(M, Cout, device='cuda'), torch.empty(M, Cout, dtype=BF16, device='cuda')
        fn('vitae_conv3d_fwd')(xs.data_ptr(), packed[0].data_ptr(), y.data_ptr(), y16.data_ptr(), *geo, st)
        say('fwd', y)
        say('fwd_bf16', y16)
        dx, dx16 = torch.empty(V, Cin, device='cuda'), torch.empty(V, Cin, dtype=BF16, device='cuda')
        for acc in (0, 1):          # the second call adds to what the first wrote
            fn('vitae_conv3d_bwd_input')(dy.data_ptr(), packed[1].data_ptr(), dx.data_ptr(), dx16.data_ptr(), acc, *geo, st)
            say(f'dx_acc{acc}', dx)
            say(f'dx_acc{acc}_bf16', dx16)
    n = lib.vitae_conv3d_wgrad_ws_floats(*geo)
    ws, dw = torch.empty(n, device='cuda'), torch.empty(Cout, Cin, *c['k'], device='cuda')
    for acc in (0, 1):
        fn('vitae_conv3d_bwd_weight')(dy.data_ptr(), xs.data_ptr(), dw.data_ptr(), ws.data_ptr(), n, acc, *geo, st)
        say(f'dw_acc{acc}', dw)


def main() -> None:
    assert torch.cuda.is_available(), 'conv_bits needs the GPU'
    chunk = _abi.CONSTS['VITAE_CONV3D_WGRAD_CHUNK']
    three_chunks = TB.conv_case(1, (2 * chunk // 64 + 3, 8, 8), 4, 8, 3, (1, 1, 1), 1)      # test_wgrad_three_chunks_with_a_partial_last
    seed = 100
    for x3 in (False, True):
        for table, cases in (('bf16_table', TB.CASES), ('x3_table', TX.CASES)):
            for name, c in cases.items():
                seed += 1
                run(f'{table}/{name}', c, seed, x3)
        for name, c in (('three_chunks', three_chunks), ('two_chunks', TX.BIG_WGRAD)):
            seed += 1
            run(f'wgrad/{name}', c, seed, x3, only_dw=True)


if __name__ == '__main__':
    main()
