"""Headline benchmark: pre-training volumes/sec of the ViT-B/16^3 (contrastive) MAE step on MI355X.

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]
                                                             (N > 1 without a launcher: spawns N ranks itself)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A "step" = one full optimisation step of BASELINE config 2 (ViT-B/16^3 autoenc as the reference
scripts train it, i.e. ``contr_mae_vit_base_patch16``; synthetic BraTS-shape 96^3 x 4ch volumes,
batch 4 per GPU, mask 0.75): forward (both views) + loss chain + backward + global grad norm +
AdamW, with the gradient all-reduce over RCCL at N > 1.  Inputs are resident in HBM before the timed
region.  Weights come from the product's own ``initialize_weights`` (seed 0).  Rank 0 prints ONE JSON
line (contract in the task statement).

A plain run sets up, warms up, times the K steps and prints the line; ``--dump-outputs DIR`` then runs
the timed path once more on the batch of the last timed step, from the seeded state of set-up, and
writes what it computed (``step_outputs``) as ``DIR/<name>.npy``: the same on every run up to float
round-off.  ``--full`` adds everything else to the line: ``roofline`` (the GEMM kernel the
step spends most time in, timed with HIP events on the launch stream in instrumented steps right after
the timed region; plus ``encoder_attn_mlp_b8``, the north-star sub-total at batch 8), the secondary data
points under ``config.also_*``, the exchange diagnostics at N > 1 and, at N = 1, ``cpu_baseline`` and
``parity`` (the same state dict handed to the CPU oracle, the only place ``oracle/`` is imported).
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# Plumbing check only (never a reported number): VITAE_BENCH_ONE_GPU=1 lets N ranks share cuda:0 and exchange over gloo, so the
# whole N > 1 flow (rank spawn, per-phase graphs, bucketed exchange, barriers, max-over-ranks clock, rank-0 instrumentation)
# can be run on a one-GPU box.  The printed line says so in config.parallelism.
ONE_GPU = os.environ.get('VITAE_BENCH_ONE_GPU') == '1'
VOL, CH, PATCH = 96, 4, 16
PEAK_TFLOPS = {'bf16': 2500.0, 'fp32': 157.3, 'fp32x3': 2500.0 / 3}   # dense MFMA peaks, MI355X_MICROARCH.md (fp32x3: three bf16 MFMAs per product)
ALGO_GFLOP_PER_VOL = {'contr': 136.3, 'mae': 90.8}   # BASELINE.md §4 (fwd+bwd, reference formulation)
ENC_ATTN_MLP_GFLOP_PER_VOL = 9.45 * 3                # encoder blocks fwd+bwd, one view per volume
P8_GFLOP_PER_VOL = 941.4                             # the reference's shipped shape (patch 8), contrastive ViT-B, fwd+bwd
KNAMES = {'glds_pair': 'gemm_glds_pair_kernel<64,64,64,64> (csrc/gemm_glds.hip: dgrad + wgrad of one Linear per launch)',
          'glds': 'gemm_glds_kernel<64,64,..> (csrc/gemm_glds.hip)',
          'glds_wide': 'gemm_glds_kernel<64,128,..> (csrc/gemm_glds.hip)',
          'glds_pair_wide': 'gemm_glds_pair_kernel<..,64,128> (csrc/gemm_glds.hip)',
          'glds_dgrad': 'gemm_glds_kernel<64,64,true,false> (csrc/gemm_glds.hip: dgrad of one Linear)',
          'bt256': 'gemm_bt_kernel<256,256,2,4,..> (csrc/gemm_bt.hip: 8 staggered waves)',
          'bt128': 'gemm_bt_kernel<128,128,2,2,..> (csrc/gemm_bt.hip: 4 waves, two workgroups per CU, in-launch split-K)',
          'bt_bwd': 'backward of one Linear as two launches (dgrad, wgrad), at least one on a csrc/gemm_bt.hip tile',
          'ws64_pair': 'gemm_ws64_pair_kernel (csrc/gemm_bt.hip: dgrad + wgrad of one Linear as wave-specialised 64x64 workgroups of one launch)',
          'ws64': 'gemm_ws64_kernel (csrc/gemm_bt.hip: wave-specialised 64x64 tile, 4 MFMA waves + 4 LDS-DMA waves)',
          'ws128': 'gemm_ws_kernel (csrc/gemm_bt.hip: wave-specialised 128x128 tile)',
          'bt_group': 'gemm_bt_wgrad_group_kernel (csrc/gemm_bt.hip: the four weight gradients of a transformer block in one launch of 128x128 tiles)',
          'attn': 'attn_fwd_mfma_kernel / attn_bwd_fused_kernel (csrc/attention_mfma.hip)'}
BT_NOTE = ('GEMM launches are served by csrc/gemm_bt.hip (wave-specialised 64x64 / 128x128 workgroups: 4 MFMA waves + 4 LDS-DMA producer waves; '
           '256x256 / 128x128 ping-pong tiles; in-launch split-K) or csrc/gemm_glds.hip (64-row tiles) as the cost model of vitae_gemm_glds picks per problem')


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--batch', type=int, default=4, help='volumes per GPU per step (BASELINE config 2: 4)')
    ap.add_argument('--precision', default='bf16', choices=['bf16', 'fp32', 'fp32x3'])
    ap.add_argument('--patch', type=int, default=PATCH, help='patch size (BASELINE configs: 16; the reference\'s config.ini default: 8) — not the headline workload when changed')
    ap.add_argument('--model', default='contr', choices=['contr', 'mae'])
    ap.add_argument('--no-graph', action='store_true')
    ap.add_argument('--grad-comm', default=None, choices=['fp32', 'bf16'],
                    help='wire dtype of the gradient all-reduce at >1 GPU (default: the compute precision)')
    ap.add_argument('--full', action='store_true',
                    help='also run everything beyond the headline figure: roofline, secondary data points, CPU baseline + parity, '
                         'exchange diagnostics at N > 1 (a plain run sets up, warms up, times the steps and prints the line)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, run the timed path once more on the last timed batch from the seeded state of '
                         'set-up and write what it computed (losses, seeded samples of the updated parameters and of the gradients) '
                         'to DIR/<name>.npy')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: skip the CPU baseline and parity legs')
    ap.add_argument('--no-extra', action='store_true', help='with --full: skip the secondary data points (plain MAE, batch 8 / 32, fp32 mode)')
    ap.add_argument('--cpu-steps', type=int, default=3)
    ap.add_argument('--profile-steps', type=int, default=3, help='with --full: instrumented steps for the roofline block')
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error('--steps must be at least 1')
    return args


# ----------------------------------------------------------------------------- ranks
def spawn_command(args, argv, n_visible, port):
    """The torch.distributed.run command `python bench.py --gpus N` re-executes itself under when no launcher is around it
    (one process per GPU over RCCL), or None when this process is already a rank / N == 1.  Raises SystemExit when fewer
    than N GPUs are visible: a dp-N number from fewer ranks would be a lie."""
    if args.gpus <= 1 or 'WORLD_SIZE' in os.environ:
        return None
    if n_visible < args.gpus and not ONE_GPU:
        raise SystemExit(f'bench.py --gpus {args.gpus}: only {n_visible} GPU(s) visible on this node; refusing to report a '
                         f'{args.gpus}-GPU number from fewer ranks')
    return [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={args.gpus}',
            '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + list(argv)


def rank_layout(args, env=None):
    """-> (world, rank, local).  The number of ranks RCCL will see must be the number asked for."""
    env = os.environ if env is None else env
    world = int(env.get('WORLD_SIZE', '1'))
    rank = int(env.get('RANK', '0'))
    local = int(env.get('LOCAL_RANK', '0'))
    if world != args.gpus:
        raise SystemExit(f'bench.py --gpus {args.gpus} but WORLD_SIZE={world}: launch one rank per GPU '
                         f'(torch.distributed.run --nproc-per-node {args.gpus}) or drop the launcher')
    return world, rank, local


def free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


# ----------------------------------------------------------------------------- data / model
def synthetic_batches(batch, rank, n_batches=4):
    """view2 ~ N(0,1), view1 = z-score(view2 + 0.1 N(0,1)); CPU generator 1234+rank."""
    out = []
    for i in range(n_batches):
        g = torch.Generator(device='cpu').manual_seed(1234 + rank + 1000 * i)
        v2 = torch.randn(batch, CH, VOL, VOL, VOL, generator=g)
        v1 = v2 + 0.1 * torch.randn(batch, CH, VOL, VOL, VOL, generator=g)
        dims = (2, 3, 4)
        v1 = (v1 - v1.mean(dim=dims, keepdim=True)) / v1.std(dim=dims, keepdim=True)
        out.append((v1.contiguous(), v2.contiguous()))
    return out


def masking_noise(batch, num_patches, seed):
    """two independent U[0,1) [B, L] noises from a CPU generator (the torch.rand of vit_autoenc.py:139, one per view)"""
    g = torch.Generator(device='cpu').manual_seed(seed)
    return [torch.rand(batch, num_patches, generator=g) for _ in range(2)]


def build_model(kind, precision, dev, seed=0, patch=None, fused_opt=True):
    """The product's own constructor + initialize_weights under a fixed seed; returns (model, cpu state dict, engine)."""
    from vit_ae_plus_plus_amd.model import vit_autoenc as VA
    from vit_ae_plus_plus_amd.optim import FusedAdamW
    torch.manual_seed(seed)
    margs = argparse.Namespace(use_imagenet=False, perceptual_weight=0)
    ctor = VA.contr_mae_vit_base_patch16 if kind == 'contr' else VA.mae_vit_base_patch16
    model = ctor(volume_size=VOL, in_chans=CH, patch_size=patch or PATCH, args=margs, precision=precision)
    sd_cpu = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(dev).train()
    eng = model._ensure_engine(dev)
    if fused_opt:
        opt = FusedAdamW(model, lr=1e-4, weight_decay=0.05, betas=(0.9, 0.95))
        _ = opt.engine
    return model, sd_cpu, eng


def device_batches(batch, dev, n=2, seed=77):
    g = torch.Generator(device=dev).manual_seed(seed)
    out = []
    for _ in range(n):
        v2 = torch.randn(batch, CH, VOL, VOL, VOL, generator=g, device=dev)
        v1 = v2 + 0.1 * torch.randn(batch, CH, VOL, VOL, VOL, generator=g, device=dev)
        v1 = (v1 - v1.mean(dim=(2, 3, 4), keepdim=True)) / v1.std(dim=(2, 3, 4), keepdim=True)
        out.append((v1.contiguous(), v2))
    return out


DUMP_SAMPLE = 1 << 21      # elements of the parameter / gradient samples written by --dump-outputs (8 MB each in float32)


def step_outputs(model, eng):
    """What a caller of the timed step receives after it: the loss terms + global gradient norm, the updated parameters and the
    step's gradients.  Parameters and gradients are sampled at DUMP_SAMPLE fixed positions (seeded) of their concatenation in
    ``named_parameters`` order, so the sample does not depend on the engine's arena layout.  -> {name: float32 / float64 array}"""
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    params = torch.cat([eng.p[n].reshape(-1) for n in names])
    grads = torch.cat([eng.g[n].reshape(-1) for n in names])
    n = params.numel()
    if n > DUMP_SAMPLE:
        idx = torch.randint(n, (DUMP_SAMPLE,), generator=torch.Generator(device='cpu').manual_seed(0)).sort().values.to(params.device)
        params, grads = params[idx], grads[idx]
    return {'losses': eng.losses[:6].double().cpu().numpy(),      # [loss, raw_edge, recon, percep, contr, grad_norm]
            'params_sample': params.float().cpu().numpy(), 'grads_sample': grads.float().cpu().numpy()}


def state_snapshot(eng):
    """Copies of everything a fused step reads and updates (the set ``_StepRunner._capture`` saves around its warm-up launch:
    parameters, gradients, AdamW moments, predictor BatchNorm statistics, the device block with the applied-step count) and the
    host's step count."""
    keep = [eng.params, eng.grads] + ([eng.opt_state['exp_avg'], eng.opt_state['exp_avg_sq']] if eng.opt_state else [])
    keep += [t for k, t in eng.buffers.items() if k.startswith('predictor.1.')]
    keep.append(eng.hp)
    return keep, [t.clone() for t in keep], eng.opt_step


def restore_state(eng, snap):
    keep, saved, opt_step = snap
    for t, s in zip(keep, saved):
        t.copy_(s)
    eng.opt_step = opt_step
    eng.refresh_shadow(force=True)     # the bf16 / two-plane weight copies follow the restored fp32 arena


def write_outputs(outdir, outs):
    import numpy as np
    os.makedirs(outdir, exist_ok=True)
    for name, a in outs.items():
        np.save(os.path.join(outdir, f'{name}.npy'), a)


def run_steps(model, eng, batches, contr, batch, graph, warm, steps):
    runner = model._step_runner(batch, 0.75, True, False, graph)
    t0 = 0.0
    for i in range(warm + steps):
        if i == warm:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        v1, v2 = batches[i % len(batches)]
        runner.load(v1, v2 if contr else None)
        eng.optimizer_hparams(lr=1e-4)
        runner.run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


# ----------------------------------------------------------------------------- instrumentation
def instrumented_steps(model, eng, batches, contr, batch, n_steps, dev, phases_only=False):
    """Eager steps with HIP events (torch.cuda.Event on the launch stream = torch's current stream) around every GEMM /
    attention launch.  A spin kernel is queued first so the host enqueues the whole step while the GPU is still busy: the
    event deltas then contain no host-launch gaps.  -> ([(ms, flops, tag, scope, raw ms)], event-pair overhead in ms)"""
    from vit_ae_plus_plus_amd._abi import lib as _lib
    eager = model._step_runner(batch, 0.75, True, False, False)
    recs = []
    for i in range(n_steps):
        v1, v2 = batches[i % len(batches)]
        eager.load(v1, v2 if contr else None)
        eng.optimizer_hparams(lr=1e-4)
        torch.cuda._sleep(200_000_000)
        eng.gemm_timer = []
        if phases_only:   # N > 1: keep collectives matched — other ranks idle here, so time the phases locally only
            for k in range(eng.N_PHASES - 1):
                eager._phase(k)
        else:
            eager.run()
        torch.cuda.synchronize()
        recs += eng.gemm_timer
        eng.gemm_timer = None
    # calibration of the event pair itself: the same record / tiny kernel / record pattern behind a spin kernel.  A
    # 16-byte fill runs for ~2 us (rocprofv3: the launch floor of this box); whatever the events report beyond that is
    # command-processor time around the kernel, not kernel time, and is removed.
    scratch = torch.zeros(64, device=dev)
    torch.cuda._sleep(50_000_000)
    cal = []
    for _ in range(64):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.vitae_memset_zero(scratch.data_ptr(), 16, torch.cuda.current_stream(dev).cuda_stream)
        b.record()
        cal.append((a, b))
    torch.cuda.synchronize()
    null_ms = sorted(x.elapsed_time(y) for x, y in cal)[len(cal) // 2]
    overhead = max(0.0, null_ms - 0.002)
    out = []
    for a, b, f, tag, scope in recs:
        raw = a.elapsed_time(b)
        out.append((max(raw - overhead, 0.25 * raw), f, tag, scope, raw))
    return out, overhead


def roofline_block(args, recs, overhead_ms, ms_step, world):
    fam = {}
    for ms, f, tag, scope, raw in recs:
        if tag == 'attn':
            continue
        d = fam.setdefault(tag, [0.0, 0.0, 0, 0.0])
        d[0] += ms; d[1] += f; d[2] += 1; d[3] += raw
    n = args.profile_steps
    tot_ms = sum(d[0] for d in fam.values())
    tot_fl = sum(d[1] for d in fam.values())
    dom = max(fam, key=lambda k: fam[k][0])          # the kernel the step spends most GEMM time in
    d_ms, d_fl, d_n, d_raw = fam[dom]
    ach = d_fl / (d_ms * 1e-3) / 1e12
    peak = PEAK_TFLOPS[args.precision]
    traffic, tnote, rp_us, mfma_busy = None, None, None, None   # PMC counters cannot be read in-process: last committed rocprofv3 --pmc result
    for name in ('round6_gemm_traffic.json', 'round5_gemm_traffic.json', 'round4_gemm_traffic.json', 'round3_gemm_traffic.json', 'round2_gemm_traffic.json', 'round1_gemm_traffic.json'):
        tfile = os.path.join(ROOT, 'profiles', name)
        if args.precision == 'bf16' and args.batch == 4 and os.path.exists(tfile):
            tj = json.load(open(tfile))
            traffic = tj.get('bytes_per_launch', {}).get(dom)
            rp_us = tj.get('rocprof_avg_launch_us', {}).get(dom)    # the committed rocprofv3 mean of the same kernel (graph replays)
            mfma_busy = tj.get('mfma_busy_frac', {}).get(dom)       # SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x duration x 2.4 GHz), same file
            tnote = f'HBM-side bytes per launch of that kernel (2*FETCH_SIZE + WRITE_SIZE, profiles/{name})'
            if traffic is not None:
                break
    exe_gflop = tot_fl / n / 1e9        # GEMM flops the step actually executes (masked patches are not embedded)
    ref_gflop = world * args.batch * ALGO_GFLOP_PER_VOL[args.model]
    sec = ms_step * 1e-3
    return {'bound': 'mfma', 'kernel': KNAMES.get(dom, dom), 'achieved': round(ach, 2), 'peak': peak, 'unit': 'TFLOP/s',
            'frac': round(ach / peak, 4), 'traffic': traffic, 'traffic_unit': tnote,
            # (NOT measured by this run: PMC counters cannot be read in-process — the value of the last committed rocprofv3 --pmc pass)
            'mfma_busy_frac_committed_profile': mfma_busy, 'mfma_busy_note': 'matrix-pipe busy cycles of that kernel (rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES, committed pass) / (1024 SIMDs x its duration x 2.4 GHz)',
            'launches_per_step': d_n / n, 'gflop_per_launch': round(d_fl / d_n / 1e9, 3), 'avg_launch_us': round(d_ms * 1e3 / d_n, 2),
            'avg_launch_us_events_raw': round(d_raw * 1e3 / d_n, 2), 'event_pair_overhead_us': round(overhead_ms * 1e3, 2),
            # the same kernel's mean in the committed rocprofv3 profile and the fraction it gives (graph replays: launches beside an
            # AdamW bucket run slower than in the instrumented eager steps above)
            'avg_launch_us_rocprof_committed': rp_us,
            'frac_at_rocprof_duration': round(d_fl / d_n / (rp_us * 1e-6) / 1e12 / peak, 4) if rp_us else None,
            'gemm_family': {'launches_per_step': sum(d[2] for d in fam.values()) / n, 'gflop_per_step': round(exe_gflop, 2),
                            'ms_per_step': round(tot_ms / n, 3), 'tflops': round(tot_fl / (tot_ms * 1e-3) / 1e12, 2),
                            'by_kernel_ms_per_step': {k: round(v[0] / n, 3) for k, v in fam.items()}},
            # whole step against the MFMA peak, on the FLOPs it executes and on the reference formulation (which embeds
            # the masked patches too: 136.3 vs 106.1 GFLOP per volume for the contrastive model)
            'step_frac_of_peak_executed': round(exe_gflop * 1e9 / sec / 1e12 / peak, 4),
            'step_frac_of_peak_reference_formulation': round(ref_gflop * 1e9 / sec / 1e12 / (peak * world), 4)}


def _committed_b8_mfma_busy():
    """MFMA-busy share of the GEMM + attention kernels of a batch-8 step from the committed counter pass (profiles/round5_pmc_sq_b8.json,
    tools/probes/refresh_profiles_r5.sh): sum of busy cycles / (1024 SIMDs x sum of durations x 2.4 GHz).  None when the file is absent."""
    f = next((q for q in (os.path.join(ROOT, 'profiles', n) for n in ('round6_pmc_sq_b8.json', 'round5_pmc_sq_b8.json')) if os.path.exists(q)), None)
    if f is None:
        return None
    try:
        return json.load(open(f)).get('gemm_attn_mfma_busy_frac')
    except Exception:
        return None


def encoder_attn_mlp_point(args, dev, model, eng, contr, batch=8):
    """North-star sub-total: the encoder's attention + MLP kernels (qkv / proj / fc1 / fc2 GEMMs forward and backward and
    the attention kernels of the 12 encoder blocks) at batch 8: executed FLOPs / sum of their HIP-event durations."""
    batches = device_batches(batch, dev)
    dt = run_steps(model, eng, batches, contr, batch, not args.no_graph, 2 * len(batches) + 2, 10)
    recs, ov = instrumented_steps(model, eng, batches, contr, batch, 2, dev)
    enc = [r for r in recs if r[3] == 'enc']
    ms = sum(r[0] for r in enc) / 2
    fl = sum(r[1] for r in enc) / 2
    peak = PEAK_TFLOPS[args.precision]
    views = 2 if contr else 1
    return ({'batch': batch, 'value': round(batch / dt, 2), 'unit': 'volumes/s', 'ms_per_step': round(dt * 1e3, 3), 'steps': 10},
            {'batch': batch, 'kernels': 'encoder blocks: qkv/proj/fc1/fc2 GEMMs fwd + dgrad/wgrad, attention fwd + bwd',
             'launches_per_step': len(enc) / 2, 'gflop_executed': round(fl / 1e9, 1),
             'gflop_reference_formulation_one_view': round(batch * ENC_ATTN_MLP_GFLOP_PER_VOL, 1), 'views': views,
             'sum_kernel_ms': round(ms, 3), 'achieved': round(fl / (ms * 1e-3) / 1e12, 1), 'peak': peak, 'unit': 'TFLOP/s',
             'frac': round(fl / (ms * 1e-3) / 1e12 / peak, 4), 'target_frac': 0.40,
             'mfma_busy_frac_committed_profile': _committed_b8_mfma_busy(),
             'event_pair_overhead_us': round(ov * 1e3, 2)})


def cpu_baseline(args, batches, sd_cpu, noises):
    """The oracle (CPU restatement of the reference, validated against it in tests) timed on this
    host: full training steps of the same workload.  Also returns the first-step losses."""
    from oracle import mae_ref as R
    from oracle import train_ref as T
    cfg = R.vit_base_cfg(volume_size=(VOL,) * 3, patch_size=PATCH, in_chans=CH, contrastive=args.model == 'contr')
    cores = torch.get_num_threads()
    tr = T.RefTrainer(cfg, sd_cpu, lr=1e-4, weight_decay=0.05)
    first = None
    times = []
    for i in range(args.cpu_steps + 1):
        v1, v2 = batches[i % len(batches)]
        n1, n2 = noises[i % len(noises)]
        t0 = time.perf_counter()
        terms, _, _ = tr.step(v1, v2, n1, n2, lr=1e-4, mask_ratio=0.75, edge_map_weight=0.01, contr_weight=0.001)
        dt = time.perf_counter() - t0
        if i == 0:
            first = terms
        else:
            times.append(dt)
    sec = sum(times) / len(times)
    return {'value': args.batch / sec, 'unit': 'volumes/s', 'cores': cores, 'kind': 'port',
            'sample': f'{args.cpu_steps} timed full steps (fwd+loss+bwd+AdamW) of the same workload, batch {args.batch}, '
                      f'fp32, torch {torch.__version__} CPU, after 1 warm-up step; {sec:.2f} s/step'}, first


def secondary_model_point(args, dev, kind, precision, batches, label):
    """Another model / precision through the same step machinery (own instance, own graphs)."""
    model, _, eng = build_model(kind, precision, dev)
    eng.set_loss_weights(0.01, 0.001 if kind == 'contr' else 0.0, 1, 1)
    dt = run_steps(model, eng, batches, kind == 'contr', args.batch, not args.no_graph, 2 * len(batches) + 2, 15)
    return {'model': label, 'precision': precision, 'value': round(args.batch / dt, 2), 'unit': 'volumes/s',
            'ms_per_step': round(dt * 1e3, 3), 'steps': 15}


def patch8_point(args, dev):
    """The reference's SHIPPED shape (config.ini:33 patch_size = 8 through read_configs.py:38 into model_factory.py:12): contrastive
    ViT-B on 96^3 x 4ch = 1728 patches, 433 encoder / 1729 decoder tokens, 941 GFLOP per volume in the reference formulation —
    the one configuration of this model that is compute-bound.  Full optimisation step at the bench's batch; MFMA fraction on the
    reference formulation and on the GEMM + attention FLOPs the step executes (HIP events around those launches)."""
    model, _, eng = build_model('contr', args.precision, dev, patch=8)
    eng.set_loss_weights(0.01, 0.001, 1, 1)
    batches = device_batches(args.batch, dev)
    dt = run_steps(model, eng, batches, True, args.batch, not args.no_graph, 2 * len(batches) + 2, 10)
    recs, ov = instrumented_steps(model, eng, batches, True, args.batch, 1, dev)
    peak = PEAK_TFLOPS[args.precision]
    fam = {}
    for ms, f, tag, scope, raw in recs:
        d = fam.setdefault(tag, [0.0, 0.0, 0])
        d[0] += ms; d[1] += f; d[2] += 1
    k_ms, k_fl = sum(d[0] for d in fam.values()), sum(d[1] for d in fam.values())
    return {'model': 'contr_mae_vit_base_patch16(patch_size=8): the reference\'s config.ini default', 'batch': args.batch,
            'tokens': {'patches': eng.cfg.num_patches, 'encoder': eng.cfg.len_keep(0.75) + 1 if hasattr(eng.cfg, 'len_keep') else 433,
                       'decoder': eng.cfg.num_patches + 1},
            'value': round(args.batch / dt, 2), 'unit': 'volumes/s', 'ms_per_step': round(dt * 1e3, 3), 'steps': 10,
            'gflop_per_volume_reference_formulation': P8_GFLOP_PER_VOL,
            'step_frac_of_peak_reference_formulation': round(P8_GFLOP_PER_VOL * args.batch / dt / 1e3 / peak, 4),
            'gemm_attn_gflop_executed_per_step': round(k_fl / 1e9, 1), 'gemm_attn_kernel_ms_per_step': round(k_ms, 3),
            'gemm_attn_frac_of_peak': round(k_fl / (k_ms * 1e-3) / 1e12 / peak, 4),
            'by_kernel': {k: {'ms': round(v[0], 3), 'tflops': round(v[1] / (v[0] * 1e-3) / 1e12, 1), 'launches': v[2]} for k, v in fam.items()}}


def other_config_point(args, dev, which):
    """BASELINE configs 4 and 5 through the same fused step / graph replay (parity cases elsewhere: tests/test_gpu_model.py
    ::test_config4_vit_large_128, ::test_config5_anisotropic_egd_shape): config 4 = mae_vit_large_patch16 on 128^3 x 4ch
    (model/vit_autoenc.py:288-293: 513 decoder tokens, 129 kept), config 5 = mae_vit_base_patch16 on EGD-shape 192 x 192 x 32 x 1ch
    volumes (the non-cubic patch grid 12 x 12 x 2).  GFLOP per volume of the reference formulation: BASELINE.md section 4."""
    from vit_ae_plus_plus_amd.model import vit_autoenc as VA
    from vit_ae_plus_plus_amd.optim import FusedAdamW
    c = {4: dict(ctor='mae_vit_large_patch16', vol=(128, 128, 128), ch=4, gflop=406.8, batch=4,
                 label='BASELINE config 4: ViT-L/16 MAE, 128^3 x 4ch'),
         5: dict(ctor='mae_vit_base_patch16', vol=(192, 192, 32), ch=1, gflop=94.8, batch=4,
                 label='BASELINE config 5: ViT-B/16 MAE, EGD-shape 192 x 192 x 32 x 1ch (per-rank workload)')}[which]
    model = getattr(VA, c['ctor'])(volume_size=c['vol'][0] if which == 4 else c['vol'], in_chans=c['ch'], patch_size=16,
                                   args=argparse.Namespace(use_imagenet=False, perceptual_weight=0), precision=args.precision).to(dev).train()
    eng = model._ensure_engine(dev)
    opt = FusedAdamW(model, lr=1e-4, weight_decay=0.05, betas=(0.9, 0.95)); _ = opt.engine
    eng.set_loss_weights(0.01, 0.0, 1, 1)
    B = c['batch']
    g = torch.Generator(device=dev).manual_seed(1)
    vols = [torch.randn(B, c['ch'], *c['vol'], device=dev, generator=g) for _ in range(3)]
    runner = model._step_runner(B, 0.75, True, False, not args.no_graph)
    warm, steps = 2 * len(vols) + 2, 10
    for i in range(warm + steps):
        if i == warm:
            torch.cuda.synchronize(); t0 = time.perf_counter()
        runner.load(vols[i % 3], None); eng.optimizer_hparams(lr=1e-4); runner.run()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    out = {'model': c['label'], 'batch': B, 'params_m': round(sum(q.numel() for q in model.parameters() if q.requires_grad) / 1e6, 1),
           'value': round(B / dt, 2), 'unit': 'volumes/s', 'ms_per_step': round(dt * 1e3, 3), 'steps': steps,
           'gflop_per_volume_reference_formulation': c['gflop'],
           'step_frac_of_peak_reference_formulation': round(c['gflop'] * B / dt / 1e3 / PEAK_TFLOPS[args.precision], 4),
           'final_losses': [round(x, 5) for x in eng.losses.cpu().tolist()[:3]]}
    del model, eng, opt, runner, vols
    torch.cuda.empty_cache()
    return out


def epoch_loop_point(args, dev, bare_ms):
    """The entry point the reference's scripts call (utils/train_one_epoch.py:21-110 train_one_stage_epoch) over >= 100
    device-resident iterations: a plain torch.optim.AdamW with timm's decay groups (the reference's optimiser,
    k_fold_cross_valid_combined_brats.py:168-169), adopted by the loop onto the fused step.  One short epoch first (graph capture)."""
    import contextlib
    import io
    from vit_ae_plus_plus_amd.utils import misc
    from vit_ae_plus_plus_amd.utils.train_one_epoch import train_one_stage_epoch
    model, _, eng = build_model(args.model, args.precision, dev, fused_opt=False)
    named = [(n, q) for n, q in model.named_parameters() if q.requires_grad]
    decay = [q for n, q in named if not (q.ndim <= 1 or n.endswith('.bias'))]
    no_decay = [q for n, q in named if (q.ndim <= 1 or n.endswith('.bias'))]
    opt = torch.optim.AdamW([{'params': no_decay, 'weight_decay': 0.0}, {'params': decay, 'weight_decay': 0.05}], lr=1e-4, betas=(0.9, 0.95))
    largs = argparse.Namespace(accum_iter=1, mask_ratio=0.75, contr_weight=0.001, lr=1e-4, min_lr=0.0, warmup_epochs=40, epochs=50,
                               hip_graph=not args.no_graph, no_fused_step=False)
    resident = device_batches(args.batch, dev, n=4)
    lab = torch.zeros(args.batch)
    iters = 120

    def epoch(n, ep):
        loader = [(resident[i % len(resident)][0], resident[i % len(resident)][1], lab) for i in range(n)]
        with contextlib.redirect_stdout(io.StringIO()):
            return train_one_stage_epoch(model, loader, opt, dev, ep, misc.NativeScalerWithGradNormCount(), log_writer=None, args=largs,
                                         edge_map_weight=0.01)
    epoch(3 * len(resident), 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stats = epoch(iters, 1)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / iters
    return {'entry_point': 'utils.train_one_epoch.train_one_stage_epoch (fused graph route, torch.optim.AdamW adopted)', 'iterations': iters,
            'value': round(args.batch / dt, 2), 'unit': 'volumes/s', 'ms_per_iteration': round(dt * 1e3, 3),
            'bare_step_ms': round(bare_ms, 3), 'over_bare_step': round(dt * 1e3 / bare_ms - 1.0, 4),
            'fused_route': bool(getattr(opt, 'engine', None) is not None), 'epoch_mean_loss': round(float(stats['loss']), 6)}


def pinned_trajectory_parity(args, dev):
    """Part of the checker leg (the only other place oracle/ is imported): the benchmarked route — batch 4, fused graph, the
    bench's precision — on the pinned batches of tests/golden/vitb_b4.npz (first step + three AdamW steps taken by the REFERENCE
    model, oracle/gen_golden.py gen_vitb_b4): worst relative error per loss term over the four steps."""
    import numpy as np
    from oracle import mae_ref as R
    from vit_ae_plus_plus_amd.model import vit_autoenc as VA
    from vit_ae_plus_plus_amd.optim import FusedAdamW
    path = os.path.join(ROOT, 'tests', 'golden', 'vitb_b4.npz')
    if not os.path.exists(path) or args.model != 'contr':
        return None
    g = np.load(path, allow_pickle=False)
    B, steps, lr, wd, mask_ratio, edge_w, contr_w = [float(v) for v in g['hp']]
    B, steps = int(B), int(steps)
    cfg = R.vit_base_cfg(volume_size=(VOL,) * 3, patch_size=PATCH, in_chans=CH, contrastive=True)
    model = VA.contr_mae_vit_base_patch16(volume_size=VOL, in_chans=CH, patch_size=PATCH,
                                          args=argparse.Namespace(use_imagenet=False, perceptual_weight=0), precision=args.precision)
    model.load_state_dict(R.init_state_dict(cfg, seed=0))
    model = model.to(dev).train()
    opt = FusedAdamW(model, lr=lr, weight_decay=wd, betas=(0.9, 0.95))
    eng = model._ensure_engine(dev)
    _ = opt.engine
    eng.set_loss_weights(edge_w, contr_w, 1)
    runner = model._step_runner(B, mask_ratio, True, False, not args.no_graph)
    worst = {'total': 0.0, 'raw_edge': 0.0, 'recon': 0.0, 'contr': 0.0}
    per_step_total = []
    for it in range(steps + 1):
        v1, v2 = R.synthetic_views((B, CH, VOL, VOL, VOL), seed=1234 + it)
        n1, n2 = R.masking_noise(B, cfg.num_patches, seed=4321 + it)
        model.set_masking_noise(n1, n2)
        runner.load(v1.to(dev), v2.to(dev))
        eng.optimizer_hparams(lr=lr)
        runner.run()
        got, want = eng.losses.cpu().tolist(), g['losses'][it]       # [loss, raw edge, recon, percep, contr]
        rel = lambda i: abs(got[i] - want[i]) / (abs(want[i]) + 1e-30)
        for key, i in (('total', 0), ('raw_edge', 1), ('recon', 2), ('contr', 4)):
            worst[key] = max(worst[key], rel(i))
        per_step_total.append(rel(0))
    return {'fixture': 'tests/golden/vitb_b4.npz (reference model: first step + 3 AdamW steps, lr 1e-4)', 'steps': steps + 1,
            'worst_total_loss_rel_err': worst['total'], 'worst_recon_loss_rel_err': worst['recon'],
            'worst_raw_edge_rel_err': worst['raw_edge'], 'worst_contr_rel_err': worst['contr'],
            'total_loss_rel_err_per_step': per_step_total}


def main():
    global PATCH
    args = parse()
    PATCH = args.patch
    cmd = spawn_command(args, sys.argv[1:], torch.cuda.device_count(), free_port())
    if cmd is not None:
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
        raise SystemExit(subprocess.call(cmd, env=env))
    world, rank, local = rank_layout(args)
    if rank != 0:   # only rank 0 talks on stdout (the contract is ONE JSON line)
        sys.stdout = open(os.devnull, 'w')
    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs an MI355X (the HIP path has no CPU fallback)')
    if ONE_GPU:
        local = 0
    if torch.cuda.device_count() <= local:
        raise SystemExit(f'rank {rank}: no GPU {local} on this node ({torch.cuda.device_count()} visible)')
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    force_ddp = os.environ.get('VITAE_FORCE_DDP') == '1' and world == 1   # single-GPU check of the N>1 machinery
    if world > 1 or force_ddp:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29533')
        os.environ.setdefault('RANK', '0')
        os.environ.setdefault('WORLD_SIZE', '1')
        if ONE_GPU:
            dist.init_process_group('gloo')
        else:
            dist.init_process_group('nccl', device_id=dev)
        assert dist.get_world_size() == args.gpus, (dist.get_world_size(), args.gpus)

    contr = args.model == 'contr'
    model, sd_cpu, eng = build_model(args.model, args.precision, dev)
    grad_comm = args.grad_comm or args.precision
    comm_dtype = torch.bfloat16 if grad_comm == 'bf16' else None
    ddp_on = world > 1 or force_ddp

    cpu_batches = synthetic_batches(args.batch, rank)
    batches = [(a.to(dev), b.to(dev)) for a, b in cpu_batches]
    L = eng.cfg.num_patches
    noises = [masking_noise(args.batch, L, seed=4321 + rank + i) for i in range(len(batches))]
    snap = state_snapshot(eng) if args.dump_outputs else None     # the seeded state of set-up, for the step --dump-outputs writes

    def timed_leg(native):
        """W warm-up + K timed steps of the headline workload through one gradient-exchange route; -> (seconds, first-step
        losses, last losses, description of the exchange)."""
        model.enable_data_parallel(dev, force=force_ddp, comm_dtype=comm_dtype, native=native)
        eng.set_loss_weights(0.01, 0.001 if contr else 0.0, 1, world)
        runner = model._step_runner(args.batch, 0.75, True, False, not args.no_graph)

        def step(i):
            v1, v2 = batches[i % len(batches)]
            runner.load(v1, v2 if contr else None, ready=True)     # device-resident batch (static since set-up): staged once, read in place when it comes back
            eng.optimizer_hparams(lr=1e-4)
            runner.run()

        # first step with the CPU-generated noise of step 0 for the parity report
        model.set_masking_noise(*(noises[0] if contr else noises[0][:1]))
        step(0)
        torch.cuda.synchronize()
        first = eng.losses.cpu().tolist()
        # graph priming (setup, like a compile step): a device batch is staged on first sight and gets a graph on its own
        # addresses on second sight, so every batch is shown twice before the W warm-up steps and the clock
        for i in range(1, 2 * len(batches)):
            step(i)
        for i in range(max(args.warmup, 1)):
            step(i)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            step(i)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        if world > 1:
            tmax = torch.tensor([el], dtype=torch.float64, device=dev)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            el = float(tmax)
        red = model._reducer
        desc = None
        diag = None
        if args.full and red is not None and red.active:
            # VERDICT r3 item 7 — make the one hardware run say WHY: per-bucket all-reduce time on the communication stream
            # (host-issued route: events around every collective), and the same step with the exchange switched off on the same
            # ranks (replicas drift apart: measurement only, nothing after this leg uses them without a fresh broadcast)
            diag = {}
            try:
                if not native:
                    red.timing = []
                    for i in range(10):
                        step(i)
                    torch.cuda.synchronize()
                    rep = red.timing_report()
                    red.timing = None
                    diag['allreduce_ms_per_bucket'] = [round(rep.get(b, 0.0), 3) for b in range(len(red.ranges))]
                    diag['allreduce_ms_per_step'] = round(sum(rep.values()), 3)
                red.paused = True
                for i in range(2 * len(batches) + 2):          # graphs of the exchange-free route: staged on first, direct on second sight
                    step(i)
                torch.cuda.synchronize()
                # (no collective anywhere in this block: with the exchange off the ranks run independently, and a rank that fails
                # here must not leave its peers waiting in a barrier — the figure is this rank's own)
                t1 = time.perf_counter()
                for i in range(10):
                    step(i)
                torch.cuda.synchronize()
                off = (time.perf_counter() - t1) / 10
                diag['ms_per_step_exchange_off'] = round(off * 1e3, 3)
                diag['exposed_exchange_ms_per_step'] = round((el / args.steps - off) * 1e3, 3)
            except Exception as e:   # diagnostics must never cost the line
                diag['error'] = repr(e)[:200]
            finally:
                red.paused = False
                red.timing = None
        if red is not None:
            from vit_ae_plus_plus_amd._abi import lib as _lib
            sizes = [sum(e - b for b, e in parts) for parts in red.ranges]
            desc = {'route': 'native: RCCL through the C ABI (vitae_ddp_*), collectives captured inside the one step graph' if native
                             else 'host-issued: torch.distributed (RCCL process group) between per-phase graphs, on a stream of its own',
                    'wire_dtype': grad_comm, 'buckets': len(red.ranges), 'bucket_mbytes': [round(n * (2 if grad_comm == 'bf16' else 4) / 2**20, 1) for n in sizes],
                    'ms_per_step': round(el / args.steps * 1e3, 3), 'value': round(world * args.batch * args.steps / el, 2)}
            if diag:
                desc['diagnostics'] = diag
            if native:
                desc['vitae_ddp_world_size'] = int(_lib.vitae_ddp_world_size())
                assert desc['vitae_ddp_world_size'] == world, (desc['vitae_ddp_world_size'], world)
        last = eng.losses.cpu().tolist()
        outs = None
        if snap is not None:
            # --dump-outputs: the timed path (same runner, same graph) on the batch of the last timed step, started from the
            # seeded state of set-up with seeded masking noise.  The steps before it are not replayed into what is written: the
            # kernels sum some gradients with float atomics, and a few dozen AdamW steps grow those last-bit differences well
            # past round-off, while one step from a fixed state reproduces to round-off run after run.
            restore_state(eng, snap)
            n1, n2 = noises[(args.steps - 1) % len(noises)]
            model.set_masking_noise(*((n1, n2) if contr else (n1,)))
            step(args.steps - 1)
            torch.cuda.synchronize()
            outs = step_outputs(model, eng) if rank == 0 else None
        return el, first, last, desc, outs

    # N > 1 (the driver's one scaling run): BOTH exchange routes in the same invocation — host-issued collectives between
    # per-phase graphs (default) and RCCL inside the step graph (vitae_ddp_*); the faster is the reported value, the other sits in
    # config.also_exchange.  (The plumbing mode shares one GPU over gloo: RCCL refuses two ranks on a device, so no native leg.)
    # The host-issued route goes first and the line is ASSEMBLED from it (instrumentation included) before the native route is
    # tried under a watchdog (below): RCCL through the C ABI has only ever met a world of one rank on this pool, and a second
    # route that hangs or throws on some rank must never cost the line.
    t_leg0 = time.perf_counter()
    legs = [timed_leg(False)]
    t_leg0 = time.perf_counter() - t_leg0
    also_exchange = None
    if ddp_on and ONE_GPU:
        also_exchange = {'skipped': 'native RCCL leg needs one GPU per rank (plumbing mode: all ranks on one GPU over gloo)'}
    elapsed, first_gpu, last, exchange, outs = legs[0]
    if outs is not None:
        write_outputs(args.dump_outputs, outs)
    forked = eng.forked_branches()      # (of the timed workload: the extra points below rebind the workspace)
    ms = elapsed / args.steps * 1e3
    value = world * args.batch * args.steps / elapsed

    # ---- roofline of the dominant kernel (the MFMA GEMM kernels of csrc/gemm_glds.hip / gemm_bf16.hip / gemm.hip)
    roof = None
    if args.full and rank == 0 and args.profile_steps > 0:
        recs, overhead = instrumented_steps(model, eng, batches, contr, args.batch, args.profile_steps, dev,
                                            phases_only=world > 1)
        roof = roofline_block(args, recs, overhead, ms, world)
    if world > 1:
        dist.barrier()

    extra = {}
    single = args.full and rank == 0 and world == 1 and not force_ddp and not args.no_extra
    if single and args.batch != 8 and args.precision == 'bf16':
        try:
            extra['also_batch8'], enc = encoder_attn_mlp_point(args, dev, model, eng, contr)
            if roof is not None:
                roof['encoder_attn_mlp_b8'] = enc
        except Exception as e:   # a secondary point must never cost the headline line
            extra['also_batch8'] = {'error': repr(e)[:200]}
    if single and args.batch < 32:
        try:
            b32 = device_batches(32, dev)
            dt = run_steps(model, eng, b32, contr, 32, not args.no_graph, 2 * len(b32) + 2, 10)
            extra['also_batch32'] = {'batch': 32, 'value': round(32 / dt, 2), 'unit': 'volumes/s', 'ms_per_step': round(dt * 1e3, 3),
                                     'steps': 10, 'step_tflops': round(ALGO_GFLOP_PER_VOL[args.model] * 32 / dt / 1e3, 1)}
            del b32
        except Exception as e:
            extra['also_batch32'] = {'error': repr(e)[:200]}
    if single and contr:
        try:
            extra['also'] = secondary_model_point(args, dev, 'mae', args.precision, batches,
                                                  'mae_vit_base_patch16 (plain MAE, one view per volume)')
        except Exception as e:
            extra['also'] = {'error': repr(e)[:200]}
    if single and args.precision == 'bf16':
        try:
            extra['also_fp32'] = secondary_model_point(args, dev, args.model, 'fp32', batches,
                                                       'the headline model in fp32 mode (exact-fp32 MFMA: the parity mode)')
        except Exception as e:
            extra['also_fp32'] = {'error': repr(e)[:200]}
        try:   # the reference's arithmetic is fp32 — the fast mode that still holds its losses to 1e-4
            extra['also_fp32x3'] = secondary_model_point(args, dev, args.model, 'fp32x3', batches,
                                                         'the headline model in fp32x3 mode (fp32 operands split into bf16 hi + lo while '
                                                         'staged, hi.hi + hi.lo + lo.hi on the bf16 MFMA, fp32 accumulate; fp32 attention, '
                                                         'norms, losses, optimiser): fp32-grade parity — tests/test_gpu_model.py holds it to the '
                                                         'fp32 mode\'s bounds against the reference pins')
        except Exception as e:
            extra['also_fp32x3'] = {'error': repr(e)[:200]}
    if single:
        try:
            extra['also_epoch_loop'] = epoch_loop_point(args, dev, ms)
        except Exception as e:
            extra['also_epoch_loop'] = {'error': repr(e)[:200]}
    if single and contr:
        try:
            extra['also_p8'] = patch8_point(args, dev)
        except Exception as e:
            extra['also_p8'] = {'error': repr(e)[:200]}
    if single and args.patch == 16:
        for which in (4, 5):      # the two BASELINE configs that had no throughput figure
            try:
                extra[f'also_cfg{which}'] = other_config_point(args, dev, which)
            except Exception as e:
                extra[f'also_cfg{which}'] = {'error': repr(e)[:200]}

    cpu, parity = None, None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu, first_cpu = cpu_baseline(args, cpu_batches, sd_cpu, noises)
        ref_total, ref_recon = first_cpu['loss'], first_cpu['reconstruction_loss']
        got_total, got_recon = first_gpu[0] + (first_gpu[4] if contr else 0.0), first_gpu[2]
        parity = {'recon_loss_gpu': got_recon, 'recon_loss_cpu_oracle': ref_recon,
                  'recon_rel_err': abs(got_recon - ref_recon) / abs(ref_recon),
                  'total_rel_err': abs(got_total - ref_total) / abs(ref_total), 'precision': args.precision,
                  'note': 'first step (the prediction is ~0 there: the losses barely depend on the model); the trained-model figures '
                          'are in pinned_trajectory. North-star tolerance: reconstruction loss within 1e-4 relative.'}
        try:
            parity['pinned_trajectory'] = pt = pinned_trajectory_parity(args, dev)
            # the terms the headline dtype does NOT hold to 1e-4 once the model has moved, at the top level
            parity['worst_total_loss_rel_err'] = pt.get('worst_total_loss_rel_err')
            parity['worst_raw_edge_rel_err'] = pt.get('worst_raw_edge_rel_err')
            parity['worst_contr_rel_err'] = pt.get('worst_contr_rel_err')
        except Exception as e:
            parity['pinned_trajectory'] = {'error': repr(e)[:200]}
        if args.precision == 'bf16' and args.model == 'contr' and args.patch == 16 and not args.no_extra:
            # the option that holds EVERY loss term of the bf16 route to 1e-4 (two-plane weights for the whole decoder + the encoder's attention
            # projection: tests/test_gpu_model.py::test_bf16_with_the_decoder_on_two_plane_weights_holds_every_loss_term) and what it costs
            prev = os.environ.get('VITAE_W2')
            os.environ['VITAE_W2'] = 'decoder,enc.proj'
            try:
                pt2 = pinned_trajectory_parity(args, dev)
                pnt = secondary_model_point(args, dev, args.model, 'bf16', batches, 'VITAE_W2=decoder,enc.proj')
                parity['option_w2_decoder'] = {'env': 'VITAE_W2=decoder,enc.proj', 'worst_total_loss_rel_err': pt2['worst_total_loss_rel_err'],
                                               'worst_raw_edge_rel_err': pt2['worst_raw_edge_rel_err'], 'worst_recon_loss_rel_err': pt2['worst_recon_loss_rel_err'],
                                               'worst_contr_rel_err': pt2['worst_contr_rel_err'], 'value': pnt['value'], 'unit': 'volumes/s',
                                               'ms_per_step': pnt['ms_per_step']}
            except Exception as e:
                parity['option_w2_decoder'] = {'error': repr(e)[:200]}
            finally:
                if prev is None:
                    os.environ.pop('VITAE_W2', None)
                else:
                    os.environ['VITAE_W2'] = prev
        parity['parity_note'] = ('cubic volumes (configs 1, 2, 4 and patch 8): pinned to the reference itself (tests/golden); '
                                 'non-cubic (config 5, 192x192x32): oracle only (the reference cannot construct it)')

    if rank == 0:
        out = {'metric': 'pretrain volumes/sec (96^3x4ch, mask 0.75) at 1/2/4/8 MI355X + recon-loss parity',
               'value': round(value, 2), 'unit': 'volumes/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
               'ms_per_step': round(ms, 3), 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
               'dtype': args.precision, 'data': 'synthetic',
               'config': {'workload': f'ViT-B/16^3 {"contrastive " if contr else ""}MAE full optimisation step '
                                      f'(fwd+loss+bwd+grad-norm+AdamW), synthetic BraTS-shape 96^3x4ch, ' + (f'PATCH {PATCH} (not the headline workload), ' if PATCH != 16 else '') + 'batch '
                                      f'{args.batch}/GPU, mask 0.75 (BASELINE config 2{" / 3" if world > 1 else ""})',
                          'global_batch': world * args.batch,
                          'parallelism': f'dp{world}' + (' (PLUMBING CHECK: all ranks on ONE GPU, gloo transport)' if ONE_GPU else ''),
                          'rccl_ranks': dist.get_world_size() if (world > 1 or force_ddp) else 1,
                          'hip_graph': not args.no_graph, 'weights': 'product initialize_weights, seed 0',
                          # which branch streams the step forks (engine._branch): none = the captured step is ONE chain on one hardware queue
                          'step_branches_forked': forked,
                          'grad_allreduce': (f'{grad_comm}, {len(model._reducer.ranges)} buckets' if model._reducer is not None else None),
                          'exchange': exchange, 'also_exchange': also_exchange, 'gemm_dispatch': BT_NOTE,
                          'ddp_streams_on_own_hw_queues': (getattr(model, '_stream_report', None) or {}).get('ok'),
                          'final_losses': [round(x, 6) for x in last[:6]]},
               'roofline': roof, 'cpu_baseline': cpu}
        out['config'].update(extra)
        if parity:
            out['parity'] = parity
    def emit():
        if rank == 0:
            # RCCL writes its version banner through C stdio: drain that first so the JSON line is the LAST line
            import ctypes
            try:
                ctypes.CDLL(None).fflush(None)
            except Exception:
                pass
            print(json.dumps(out), flush=True)

    clean = True
    if ddp_on and not ONE_GPU:
        import threading
        limit = 3.0 * t_leg0 + 90.0

        def bail():        # every rank runs the same timer: rank 0 prints the host-issued line, everybody leaves
            if rank == 0:
                out['config']['also_exchange'] = {'error': f'native route (vitae_ddp_*) did not finish within {limit:.0f} s; abandoned'}
            emit()
            os._exit(0)

        dog = threading.Timer(limit, bail)
        dog.daemon = True
        dog.start()
        try:
            leg = timed_leg(True)
            dog.cancel()
            if rank == 0:
                if leg[0] < elapsed:      # the faster route is the reported one, the other goes to also_exchange
                    out['config']['also_exchange'], out['config']['exchange'] = out['config']['exchange'], leg[3]
                    out['value'] = round(world * args.batch * args.steps / leg[0], 2)
                    out['ms_per_step'] = round(leg[0] / args.steps * 1e3, 3)
                    out['config']['final_losses'] = [round(x, 6) for x in leg[2][:6]]
                    if leg[4] is not None:
                        write_outputs(args.dump_outputs, leg[4])
                else:
                    out['config']['also_exchange'] = leg[3]
        except Exception as e:
            dog.cancel()
            clean = False
            if rank == 0:
                out['config']['also_exchange'] = {'error': repr(e)[:300]}
    if (world > 1 or force_ddp) and clean:
        dist.destroy_process_group()
    emit()
    if not clean:
        os._exit(0)        # a rank that threw inside the native route may have left its peers in a collective


if __name__ == '__main__':
    main()
