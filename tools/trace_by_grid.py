"""Per-(kernel, grid size) durations inside the step from a rocprofv3 --kernel-trace run of bench.py:
    python tools/trace_by_grid.py <kernel_trace.csv[.gz]> [name filter] [first step] [last step]
One kernel symbol may serve several shapes (gemm_ws64_pair_kernel is ONE image for every pair launch of a step: the tile rows of
either half are launch arguments): the grid size tells them apart.  Workgroups = grid / workgroup size.  The batch-4 step's pairs
(rows x out x in; input-gradient blocks x split + weight-gradient blocks):
    480 > 840 enc fc2 (192 + 288, 128 / 128 rows)   840 enc fc1 (88 x 3 + 576)    232 enc proj (88 + 144)   696 enc qkv (88 x 3 + 432)
    480 > 592 dec fc2 (224 + 256, 128 / 64 rows)    592 dec fc1 (112 x 3 + 256)   176 dec proj (112 + 64)   416 dec qkv (112 x 2 + 192)
The two fc2 pairs have 480 workgroups each: a pair launch is therefore keyed by the workgroups of the launch that FOLLOWS it as
well (fc2's is its block's fc1 pair), printed as "480 > 840".
Steps are cut at random_masking launches; the default window skips the first five."""
import collections, csv, gzip, re, sys

f = sys.argv[1]
flt = sys.argv[2] if len(sys.argv) > 2 else ''
rows = list(csv.DictReader(gzip.open(f, 'rt') if f.endswith('.gz') else open(f)))
rows.sort(key=lambda r: int(r['Start_Timestamp']))
idx = [i for i, r in enumerate(rows) if 'random_masking' in r['Kernel_Name']]
lo = int(sys.argv[3]) if len(sys.argv) > 3 else 5
hi = int(sys.argv[4]) if len(sys.argv) > 4 else len(idx) - 1
seg, steps = rows[idx[lo]:idx[hi]], hi - lo


def short(n):
    n = re.sub(r'\(anonymous namespace\)::', '', n)
    return re.sub(r'^void ', '', n).replace('vglds::', '').split('(')[0][:56]


wgs = lambda r: int(r['Grid_Size_X']) // max(int(r['Workgroup_Size_X']), 1)
agg = collections.defaultdict(list)
for i, r in enumerate(seg):
    n = short(r['Kernel_Name'])
    if flt in n:
        g = f'{wgs(r)} > {wgs(seg[i + 1])}' if 'pair_kernel' in n and i + 1 < len(seg) else str(wgs(r))
        agg[(n, g)].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
print(f'steps {steps} (of {len(idx)}); per (kernel, workgroups): launches per step, mean / min / max us per launch, us per step')
tot = 0.0
for (n, g), v in sorted(agg.items(), key=lambda kv: -sum(kv[1])):
    tot += sum(v) / steps
    print(f'{n:56s} wgs {g:>11s}  n {len(v) / steps:5.1f}  mean {sum(v) / len(v):7.2f}  min {min(v):7.2f}  max {max(v):7.2f}  per step {sum(v) / steps:8.1f}')
print(f'total {tot:.1f} us per step')
