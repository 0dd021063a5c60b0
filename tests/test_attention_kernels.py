"""The attention kernels of csrc/attention.hip and csrc/attention_mfma.hip: bit for bit on routed, tied and uniform operands, and per
element against float64 — with NaN around every input and sentinels around every output.

One harness (``fwd_call`` / ``bwd_call``, one branch per entry point): qkv (fp32 or bf16), o, dO and lse live inside larger
allocations whose surroundings are NaN (one guard row before and after, 64 elements behind); every output (o, o16, lse, dqkv, dqkv16,
the delta workspace, the column sums) lives in a buffer of the sentinel SENT = 7.25 (test_gemm_kernels.Buf), starts as NaN inside
(the column sums: as nonzero integers, which the kernel must add to) and must leave every sentinel unchanged.  All pointers are
16-byte aligned (the unaligned fallback is not a product path).  Wherever both forms are written o16 == bf16(o) and
dqkv16 == bf16(dqkv) bitwise.  The delta workspace must stay NaN on the one-launch backward and equal rowsum(o dO) after the two
streaming kernels.  A refused call (head_dim 48 / 16 on the MFMA entry points, H hd % 8 on the bf16-input ones, delta_ws == NULL
where the two-kernel route needs it) returns its VITAE_ERR_* code and writes nothing; these are host-side checks.

Paths: 'f32' vitae_sdpa_fwd / _bwd; 'mfma' vitae_sdpa_mfma_fwd / _bwd (fp32 qkv, rounded to bf16 while staged); 'bf16in'
vitae_sdpa_mfma_fwd_bf16in / _bwd_bf16in.  The bf16 paths work in base 2: q' = bf16(fp32(q) fp32(scale log2 e)), scores q' . bf16(k),
lse = (m + log2 l) LN2, dQ = scale sum dS k, dK = LN2 sum dS q' (LN2, LOG2E, scale = 1 / sqrtf(hd): the kernels' own fp32 constants).

Family 1 — exact operands, ``torch.equal``, no tolerance.  Attention as a gather: key j is g code(j), code the +-1 binary expansion
of j over the head dimension (distinct for N <= 2^hd), g = 32; query i is a copy of key pi(i), pi a seeded many-to-one draw of its
own for every (b, h).  The best score g^2 c hd (c = bf16(scale log2 e)) beats the runner-up (one bit flipped) by 2 g^2 c >= 160 in
base 2 (asserted; 524 at hd 32, 370 at hd 64; the fp32 kernels: 2 g^2 scale log2 e), so every other probability is exactly zero in
fp32 and P is exactly 1.0.  All scores are small integers times g^2 c: exact in fp32 in any order, also minus the reference point
that rides in the MFMA C operand.  V and dO are integers of [-4, 4].  Expected, bitwise: o == V[pi]; dV[j] == the integer sum of
the dO rows routed to j (zero rows where none are); dQ == dK == 0 (dP - delta is an exact integer zero on the routed key, P is exactly
zero elsewhere); delta workspace == rowsum(o dO); column sums == old + the integer sums.  lse is held to family 2's bound.
  `tie`: keys 2 m and 2 m + 1 are the same vector (the code of m over the first hd - 2 coordinates, g in the two reserved ones) with
different V: P = 1/2, 1/2, o == (Va + Vb) / 2 bitwise, dK != 0.  `tie-split`: key 2 m has (g, 0) in the reserved coordinates, key
2 m + 1 (0, g), the queries (0, 0): the scores are still exactly equal and dQ is nonzero in the reserved coordinates.  V in
[-2, 2], dO in [-1, 1]: dS = (dO . (Va - Vb)) / 4 has |numerator| <= 256 and is exact in bf16.  On the bf16 paths the backward's
P = exp2(s - lse LOG2E) is within 1.5e-3 of 1 (1/2) and ROUNDS to exactly 1.0 (0.5) in bf16 for dV, and dS = bf16(P (dP - delta))
rounds to the exact value (half a bf16 spacing is >= 2^-9 = 1.95e-3 relative) — both asserted on the CPU in the rounding model.  So
dV == sum P dO, dQ == scale (x) sum dS k and dK == LN2 (x) sum dS q' bitwise, (x) one fp32 multiplication by the kernel's constant of
an exact sum.  What provably cannot be exact and goes to family 2's bound: (1) the column sums of dQ and dK under ties — they add the
ROUNDED products scale (x) . and LN2 (x) . in an order the atomics choose; (2) the backward of the fp32 kernels under ties — their
p = expf(s - lse) with lse = m + logf(2) is not exactly 1/2; (3) the fp32 kernels' routed backward gets the forward kernel's OWN lse
(asserted against the reference first): at hd 32 and 128 the scale is no power of two and s rounds, but forward, dQ and dK/dV run
the same fma chain over d, so s - lse is exactly zero and p exactly 1 — with any other lse p would be 1 +- 1e-3.
  `uniform`: q = 0, V integers: every valid key has p = 1, l = N exactly, o = sum(V) (1 / l): within 2 ulp of the float64 mean
(1 ulp for 1 / l, should it be the hardware reciprocal, half for the multiplication, rounded up), lse within 2 ulp of ln N (exactly 0
at N = 1).  A padded key counted into a row, or a valid one masked out, moves the divisor by 1 / N >= 1 / 641 >> 2^-22.

Family 2 — rounding quality per element against float64.  Reference: float64 attention and its analytic gradients (CPU-tested against
torch.autograd) on the operand values the path uses — f32: the fp32 inputs and the fp32 scale; bf16 paths: q', bf16 of k, v and dO.
Metric: the worst element of |x - x64| / den, den the sum of the absolute addends: o: sum_j p |v|; dV: sum_i p |dO|; dQ: scale sum_j
w |k| with w_ij = p_ij (A_ij + sum_j' p_ij' A_ij'), A_ij = sum_d |dO_id| |v_jd|; dK: LN2 (scale) sum_i w |q'|; lse: absolute error
over max_j sum_d |q_id| |k_jd| times the score factor; column sums: against the sum of the per-element denominators plus |old|.
Bound: e <= max(FACTOR e_model, FLOOR) (tests/test_norm_kernels.py), e_model the same metric on the same inputs of the plain CPU
statement of the path — f32: the fp32 torch statement (the larger of the matmul and the d-ordered running sum for the scores); bf16
paths: fp32 arithmetic with the kernels' rounding points: P rounded to bf16 for P V and for dV, dS = bf16(P (dP - delta)), the
normaliser from unrounded P, delta from the fp32 o and the fp32 dO.  The backward gets o and lse of the float64 reference rounded to
fp32, as does the model.  Sanity caps: e_model <= 2^-8 on the bf16 paths (lse: E32_SANE), E32_SANE on f32 (CPU-tested).
Input families (``family``; properties CPU-tested from the q' scores): plain N(0, 1) — peaked: q times 8 — offset: +6 on q and k
(lse in the hundreds) — all-negative: +6 on q, -6 on k: lse near -200, so exp2(0 - lse LOG2E) of a zero-filled padded key is +inf
and the backward's tail masks alone keep inf (0 - delta) out of dS and NaN out of dQ — ascending: the base-2 score grows by 6.5 per 64 keys, so a step's maximum exceeds the running reference by
less than SM_THR = 8 on one step (rescale skipped, P up to 2^7) and by more on a later one — ascending-steep: a staircase of +48 every
other step: the rescale is taken and skipped in turn — descending: the maximum is in the first tile — late: the dominant key is
the last valid row of the ragged final tile — negative-first: every score of the first step is near -50.

Which shape reaches which kernel (restated from the launchers; no environment knob is set — VITAE_ATTN_FWD, _RB, _BWD_FUSED, _BWD_G,
_F32_MFMA and _FWD_CHK64 are read once per process):
  bf16 forward    N <= 64: attn_fwd_mfma_kernel<hd, 1, 1, 64> (one 64-key chunk): N = 1, 31, 32, 33, 63, 64.
                  64 < N < 512: <hd, 1, 1, 128>, 128-key chunks, 32-key steps: N = 65, 127, 128, 129, 160, 257 (third chunk: the
                  double buffer wraps), 385 (fourth).  hd 32, N > 128 and B H >= 512: <32, 2, 2, 128> (two query blocks per wave,
                  64-key steps): B = 32, H = 16, N = 129, 161, 257: the wave's second query block empty, partial, full.
                  N >= 512: hd 32 <32, 2, 2, 128>: 512, 513 (the last step: one valid key and a whole padded tile), 577; hd 64
                  <64, 1, 2, 128>: 512, 545.
  bf16 backward   vitae_sdpa_bwd_fused_fits(N, hd) (asserted per N: 8 NP (hd + 8) + 8 NP + 12 hd <= 150 KiB, NP = ceil32(N)): N <= 448
                  at hd 32, <= 256 at hd 64 -> attn_bwd_fused_kernel, 2 NP / 32 items over ``fused_groups`` workgroups per head:
                  ceil(items / 4) capped by ceil(512 / (B H)).  B H = 6 and 1: N = 33, 65, 129, 300, 448 give 1, 2, 3, 5, 7
                  workgroups (items / 4 with a remainder); B H = 512: one workgroup walks all items (N = 1, 129, 161, 257).
                  Beyond: attn_bwd_dq_mfma_kernel<hd, 1> + attn_bwd_dkv_mfma_kernel<hd, 1> and the delta workspace: hd 32:
                  N = 449, 513, 641; hd 64: 257, 385; from fp32 and from bf16 qkv.
  fp32            hd 32, 64: attn_*_f32mfma_kernel (128 rows per workgroup, 32-row tiles): N = 1, 31, 32, 33, 127, 128, 129, 161.
                  hd 16: attn_*_kernel<16, 1> (128 rows per block): N = 1, 127, 129; hd 128: <128, 4> (32 rows per block, 4
                  lanes per row): N = 1, 31, 33, 65.
Out of scope — only the knobs reach them: attn_fwd_mfma_kernel<64, 2, 1, 128> (VITAE_ATTN_FWD=2 at hd 64), <hd, 1, 2, 128> below
N = 512 and <hd, 1, 1, 128> at N <= 64 (VITAE_ATTN_FWD, _FWD_CHK64), the two-block backward kernels attn_bwd_dq_mfma_kernel<hd, 2> /
attn_bwd_dkv_mfma_kernel<32, 2> (VITAE_ATTN_RB=2), the two-kernel backward below the LDS limit (VITAE_ATTN_BWD_FUSED=0), other
workgroup counts (VITAE_ATTN_BWD_G), and the VALU kernels attn_*_kernel<32, 1> / <64, 2> (VITAE_ATTN_F32_MFMA=0 or unaligned pointers).
B = 2, H = 3 (odd: the head strides differ from the defaults) unless stated.  Every GPU case of family 2 prints ``RATIO`` lines
(run with -s); LABNOTES.md keeps the table, the mutants, and the findings these cases made: the bf16 forward's step maximum was the
lower half wave's alone, and a routed key held by the upper half (rows 4-7, 12-15, .. of a tile) overflowed exp2; and a first step
whose maximum lay below -128 in base 2 (all-negative) rescaled the empty accumulators by exp2(+..) = inf: 0 inf = NaN."""
import math
import types

import pytest
import torch

from test_gemm_kernels import E32_SANE, GUARD, NAN, SENT, Buf, _ratio
from test_norm_kernels import FACTOR, FLOOR

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
gpu = pytest.mark.gpu
SM_THR = 8.0
E16_SANE = 2.0 ** -8
UNDER = 2.0 ** -100                                   # where every addend's probability is below fp32's exp2 range the result is a flushed zero
G = 32.0                                              # the routing gain: a power of two
f32 = lambda x: torch.tensor(x, dtype=F32)
LOG2E32, LN2_32 = f32(1.44269504088896340736), f32(0.69314718055994530942)
PATHS = ('f32', 'mfma', 'bf16in')
FAMILIES = ['plain', 'peaked', 'offset', 'all-negative', 'ascending', 'ascending-steep', 'descending', 'late', 'negative-first']
MODES = ['route', 'tie', 'tie-split', 'uniform']


def rne(x):
    return x.to(BF16).float()


def scale32(hd):
    return f32(1.0) / torch.sqrt(f32(float(hd)))     # 1.0f / sqrtf((float)hd)


def c32(hd):
    return scale32(hd) * LOG2E32                      # scale * LOG2E in fp32: what q is multiplied by before its rounding


# =========================================================================== the dispatch, restated from the launchers
def fits(N, hd):
    NP = (N + 31) // 32 * 32
    return int(hd in (32, 64) and 4 * NP * (hd + 8) * 2 + 2 * NP * 4 + 3 * hd * 4 <= 150 * 1024)


def fused_groups(N, B, H):
    items = 2 * ((N + 31) // 32)
    return max(1, min((items + 3) // 4, (512 + B * H - 1) // (B * H)))


def fwd_kernel(N, hd, B, H):
    """-> (query blocks per wave, key tiles per step, chunk rows) of the bf16 forward"""
    var = (2 if hd == 32 else 1) if N >= 512 else (2 if hd == 32 and N > 128 and B * H >= 512 else 0)
    if var == 0:
        return (1, 1, 64 if N <= 64 else 128)
    return (2, 2, 128) if var == 2 else (1, 2, 128)


# =========================================================================== operands: [B, H, N, hd] per tensor, packed as the kernels want
def pack(q, k, v):
    B, H, N, hd = q.shape
    return torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(B * N, 3 * H * hd).contiguous()


def unpack(x, B, H, N, hd):
    return x.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)


def rows(x):                                          # [B, H, N, hd] -> [B N, H hd]
    B, H, N, hd = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * N, H * hd).contiguous()


def heads(x, B, H, N, hd):                            # [B N, H hd] -> [B, H, N, hd]
    return x.reshape(B, N, H, hd).permute(0, 2, 1, 3)


def path_operands(path, q, k, v, do):
    """The operand values a path uses -> qe, k, v, dO (fp32 tensors), the factor that makes qe . k a natural-log score, scale."""
    hd = q.shape[-1]
    if path == 'f32':
        return q, k, v, do, float(scale32(hd)), float(scale32(hd))
    return rne(q * c32(hd)), rne(k), rne(v), rne(do), math.log(2.0), float(scale32(hd))


def code(N, hd, bits=None):
    """the +-1 binary expansion of the row index over `bits` coordinates, the rest +1"""
    bits = hd if bits is None else bits
    sh = torch.arange(hd).clamp_max(40)
    b = (torch.arange(N)[:, None] >> sh[None, :]) & 1
    b[:, bits:] = 1
    return (2 * b - 1).float()


def exact_inputs(mode, B, H, N, hd, seed):
    """-> q, k, v, dO [B, H, N, hd] and the route (tgt [B, H, N] | None, grp [N]): query i attends the keys j with grp[j] == tgt[i]
    (None: all of them) in equal parts — ``route_P`` makes the exact P of it"""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lim, *s: torch.randint(-lim, lim + 1, s, generator=g).float()
    if mode == 'uniform':
        k = G * code(N, hd).expand(B, H, N, hd).clone()
        v = torch.randint(1, 9, (B, H, N, hd), generator=g).float()      # positive: no mean is zero, |mean| is the sum of the |addends|
        return torch.zeros(B, H, N, hd), k, v, ri(4, B, H, N, hd), (None, torch.zeros(N, dtype=torch.long))
    if mode == 'route':
        grp = torch.arange(N)
        k1 = G * code(N, hd)
        qsrc = k1
        v, do = ri(4, B, H, N, hd), ri(4, B, H, N, hd)
    else:
        grp = torch.arange(N) // 2
        base = G * code((N + 1) // 2, hd, hd - 2)
        k1, qsrc = base[grp].clone(), base.clone()
        if mode == 'tie-split':
            k1[0::2, hd - 1] = 0
            k1[1::2, hd - 2] = 0
            qsrc[:, hd - 2:] = 0
        v, do = ri(2, B, H, N, hd), ri(1, B, H, N, hd)
    ng = int(grp.max()) + 1
    tgt = torch.randint(0, ng, (B, H, N), generator=g)                   # many-to-one: some groups get several queries, some none
    q = qsrc[tgt]
    k = k1.expand(B, H, N, hd).clone()
    return q, k, v, do, (tgt, grp)


def route_P(route, b=None):
    """the exact P [B, H, N, N] (of batch b: [H, N, N]) in float64: 1, 1/2 or 1/N on the keys a query is routed to"""
    tgt, grp = route
    if tgt is None:
        return torch.full((len(grp), len(grp)), 1.0 / len(grp), dtype=F64)
    tgt = tgt if b is None else tgt[b]
    hit = (tgt[..., :, None] == grp).double()
    return hit / hit.sum(-1, keepdim=True)


def family(fam, B, H, N, hd, seed, step=32):
    """family 2's inputs -> q, k, v, dO [B, H, N, hd] fp32; `step`: the keys a forward step covers (32 KT)"""
    g = torch.Generator().manual_seed(seed)
    q, k, v, do = (torch.randn(B, H, N, hd, generator=g) for _ in range(4))
    if fam == 'peaked':
        q = q * 8
    elif fam == 'offset':
        q, k = q + 6, k + 6
    elif fam == 'all-negative':
        q, k = q + 6, k - 6
    elif fam != 'plain':
        qa, u = 8.0, torch.full((hd,), hd ** -0.5)
        j = torch.arange(N).float()
        t = {'ascending': (6.5 / 64) * j, 'descending': -(6.5 / 64) * j,
             'ascending-steep': 48.0 * torch.div(torch.div(j, step, rounding_mode='floor') + 1, 2, rounding_mode='floor'),
             'late': 30.0 * (j == N - 1).float(), 'negative-first': -50.0 * (j < step).float()}[fam]       # the base-2 score a key aims at
        q = qa * u + 0.3 * q
        k = (t / (qa * float(c32(hd))))[:, None] * u + 0.3 * k
    return q.contiguous(), k.contiguous(), v, do


# =========================================================================== float64 reference, the CPU statements, the metric
def attn64(qe, k, v, do, factor, scale):
    """float64 attention and its analytic gradients on the given operand values, scores factor qe . k, with the denominators of the
    metric -> (values, denominators): o, lse, delta, dq, dk, dv [B, H, N, .]"""
    val, den = {}, {}

    def put(d, **kw):
        for n, t in kw.items():
            d.setdefault(n, []).append(t)

    for b in range(qe.shape[0]):                      # batch after batch: B H N^2 float64 matrices would not fit at B H = 512
        Q, K, V, G_ = (t[b].double() for t in (qe, k, v, do))
        S = factor * Q @ K.transpose(-1, -2)
        lse = torch.logsumexp(S, -1)
        P = torch.exp(S - lse[..., None])
        o = P @ V
        delta = (o * G_).sum(-1)
        dS = P * (G_ @ V.transpose(-1, -2) - delta[..., None])
        A = G_.abs() @ V.abs().transpose(-1, -2)
        w = P * (A + (P * A).sum(-1, keepdim=True))
        put(val, o=o, lse=lse, delta=delta, dq=scale * dS @ K, dk=factor * dS.transpose(-1, -2) @ Q, dv=P.transpose(-1, -2) @ G_)
        put(den, o=P @ V.abs(), lse=factor * (Q.abs() @ K.abs().transpose(-1, -2)).amax(-1), delta=(o.abs() * G_.abs()).sum(-1),
            dq=scale * w @ K.abs(), dk=factor * w.transpose(-1, -2) @ Q.abs(), dv=P.transpose(-1, -2) @ G_.abs())
    return {n: torch.stack(t) for n, t in val.items()}, {n: torch.stack(t) for n, t in den.items()}


def running_scores(a, b):
    """s += a_d b_d in fp32, d after d"""
    s = torch.zeros(*a.shape[:-1], b.shape[-2])
    for d in range(a.shape[-1]):
        s = s + a[..., :, d:d + 1] * b[..., None, :, d]
    return s


def model_f32(q, k, v, do, o_in, lse_in, running=False):
    """the plain fp32 statement of vitae_sdpa_fwd / _bwd (the backward from the o and lse it is given)"""
    sc = scale32(q.shape[-1])
    qs = q * sc
    S = running_scores(qs, k) if running else qs @ k.transpose(-1, -2)
    lse = torch.logsumexp(S, -1)
    o = torch.softmax(S, -1) @ v
    P = torch.exp(S - lse_in[..., None])
    delta = (o_in * do).sum(-1)
    dS = P * (do @ v.transpose(-1, -2) - delta[..., None])
    return dict(o=o, lse=lse, delta=delta, dq=(dS @ k) * sc, dk=dS.transpose(-1, -2) @ qs, dv=P.transpose(-1, -2) @ do)


def model_bf16(qe, k16, v16, do, o_in, lse_in):
    """fp32 arithmetic with the bf16 kernels' rounding points; qe = q', k16, v16 bf16 values, dO fp32 as given to the kernel"""
    sc = scale32(qe.shape[-1])
    S2 = qe @ k16.transpose(-1, -2)
    m = S2.amax(-1, keepdim=True)
    E = torch.exp2(S2 - m)
    l = E.sum(-1, keepdim=True)
    o = (rne(E) @ v16) / l
    lse = (m + torch.log2(l))[..., 0] * LN2_32
    P = torch.exp2(S2 - (lse_in * LOG2E32)[..., None])
    g16 = rne(do)
    delta = (o_in * do).sum(-1)
    dS = rne(P * (g16 @ v16.transpose(-1, -2) - delta[..., None]))
    return dict(o=o, lse=lse, delta=delta, dq=(dS @ k16) * sc, dk=(dS.transpose(-1, -2) @ qe) * LN2_32,
                dv=rne(P).transpose(-1, -2) @ g16, P=P, dS=dS)


def models(path, q, k, v, do, o_in, lse_in):
    """the CPU statement(s) of a path on the kernel's own inputs -> a list of result dicts"""
    if path == 'f32':
        return [model_f32(q, k, v, do, o_in, lse_in, r) for r in (False, True)]
    qe, k16, v16, _, _, _ = path_operands(path, q, k, v, do)
    return [model_bf16(qe, k16, v16, do, o_in, lse_in)]


def elem_err(x, x64, den):
    return float(_ratio((x.double() - x64).abs(), den + UNDER).max())


def seq_colsum(x, old):
    """acc += row in fp32, row after row, on top of the old content"""
    acc = old.clone().float()
    for r in x.reshape(-1, x.shape[-1]).float():
        acc = acc + r
    return acc


def colsum_parts(d):
    """dq | dk | dv [B, H, N, hd] -> [B N, 3 H hd] in the layout of dqkv"""
    return pack(d['dq'], d['dk'], d['dv'])


def within(label, e, e_model):
    r = e / e_model if e_model > 0 else (0.0 if e == 0 else float('inf'))
    print(f'RATIO {label}: e={e:.3e} e_model={e_model:.3e} ratio={r:.2f}')
    assert e <= max(FACTOR * e_model, FLOOR), (label, e, e_model)
    return r


QUANT = ('o', 'lse', 'dq', 'dk', 'dv')


def model_cap(path, name, q, k):
    """What e_model may be at most, so that a broken model cannot loosen the bound.  bf16 paths: 2^-8, the half spacing of bf16 just
    above a power of two (a row with ONE dominant probability has no more than its rounding), E32_SANE for lse, which is not
    rounded to bf16.  f32: E32_SANE (1 + max |s|), max |s| the largest |q . k| scale of the case itself: an fp32 score carries
    2^-24 |s| per rounding and exp turns that absolute error into a relative one of p — scores in the hundreds (offset,
    all-negative) cannot keep 2e-6; where |s| stays below 1 the cap is E32_SANE to a factor 2."""
    if path != 'f32':
        return E32_SANE if name == 'lse' else E16_SANE
    smax = float((q.double() @ k.double().transpose(-1, -2)).abs().max()) * float(scale32(q.shape[-1]))
    return E32_SANE * (1.0 + smax)


def model_errors(path, q, k, v, do, old_cs=None):
    """-> val64, den64, o32, lse32 (what the backward is given) and e_model per quantity (and of the column sums)"""
    qe, kk, vv, gg, factor, scale = path_operands(path, q, k, v, do)
    val, den = attn64(qe, kk, vv, gg, factor, scale)
    o_in, lse_in = val['o'].float(), val['lse'].float()
    ms = models(path, q, k, v, do, o_in, lse_in)
    em = {n: max(elem_err(m[n], val[n], den[n]) for m in ms) for n in QUANT}
    if old_cs is not None:
        cs64 = old_cs.double() + colsum_parts(val).sum(0)
        csden = old_cs.double().abs() + colsum_parts(den).sum(0)
        em['colsum'] = max(elem_err(seq_colsum(colsum_parts(m), old_cs), cs64, csden) for m in ms)
        val['colsum'], den['colsum'] = cs64, csden
    return val, den, o_in, lse_in, em


def reference_moves(S2, step, wave_rows=32):
    """The deferred rescale of attn_fwd_mfma_kernel on base-2 scores S2 [Nq, N]: per step -> (the excess tm of every query over its
    reference point, which queries' reference moved).  A wave (wave_rows queries) moves all its references when any excess is
    above SM_THR; the first step always sets it."""
    nq, N = S2.shape
    m, log = torch.zeros(nq), []
    for s0 in range(0, N, step):
        tm = S2[:, s0:s0 + step].amax(-1) - m
        if s0 == 0:
            need, delta = torch.ones(nq, dtype=torch.bool), tm
        else:
            need = torch.cat([(w > SM_THR).any().expand(len(w)) for w in tm.split(wave_rows)])
            delta = torch.where(need, tm.clamp_min(0), torch.zeros(nq))
        m = m + delta
        log.append((tm, need))
    return log


# =========================================================================== CPU tests of the constructions above
def test_dispatch_restated():
    assert [fits(n, 32) for n in (1, 448, 449)] == [1, 1, 0] and [fits(n, 64) for n in (256, 257)] == [1, 0] and fits(33, 16) == 0
    assert [fused_groups(n, 2, 3) for n in (1, 33, 65, 129, 300, 448)] == [1, 1, 2, 3, 5, 7]
    assert [fused_groups(n, 1, 1) for n in (33, 65, 448)] == [1, 2, 7] and fused_groups(257, 32, 16) == 1 and fused_groups(448, 8, 16) == 4
    assert fwd_kernel(64, 32, 2, 3) == (1, 1, 64) and fwd_kernel(65, 64, 2, 3) == (1, 1, 128) and fwd_kernel(257, 32, 2, 3) == (1, 1, 128)
    assert fwd_kernel(129, 32, 32, 16) == (2, 2, 128) and fwd_kernel(128, 32, 32, 16) == (1, 1, 128) and fwd_kernel(257, 64, 32, 16) == (1, 1, 128)
    assert fwd_kernel(512, 32, 2, 3) == (2, 2, 128) and fwd_kernel(512, 64, 2, 3) == (1, 2, 128)
    assert torch.equal(rne(f32(SENT)), f32(SENT))


@pytest.mark.parametrize('hd', [16, 32, 64, 128])
@pytest.mark.parametrize('mode', ['route', 'tie', 'tie-split'])
def test_routing_margins(hd, mode):
    """the runner-up is >= 160 below the best score in base 2, on the q' scores and on the fp32 kernels' scaled ones; keys distinct"""
    B, H, N = 2, 3, 300
    q, k, v, do, route = exact_inputs(mode, B, H, N, hd, 5)
    P = route_P(route)
    assert len(torch.unique(k[0, 0], dim=0)) == (N if mode == 'route' else (N if mode == 'tie-split' else (N + 1) // 2))
    cnt = (P[0, 0] > 0).sum(0)
    assert int((cnt == 0).sum()) > 0 and int((cnt > 1).sum()) > 0                  # some keys get no query, some several
    assert not torch.equal(P[0, 0], P[0, 1]) and not torch.equal(P[0, 0], P[1, 0])  # every (b, h) its own pi
    on, margins = P > 0, []
    for S2 in (rne(q * c32(hd)) @ rne(k).transpose(-1, -2), ((q * scale32(hd)) @ k.transpose(-1, -2)) * LOG2E32):
        best = S2.amax(-1, keepdim=True)
        assert bool(((best - S2)[on].abs() <= 2e-6 * best.abs().max()).all())      # the routed keys share the best score
        margins.append(float((best - S2)[~on].min()))
        assert margins[-1] >= 160, (hd, mode, margins)
    if mode == 'route' and hd in (32, 64):
        assert abs(margins[0] - 2 * G * G * float(rne(c32(hd)))) < 1e-3 and round(margins[0]) == {32: 524, 64: 370}[hd]
    S2 = rne(q * c32(hd)) @ rne(k).transpose(-1, -2)                                 # the q' scores are exact: the routed keys are EQUAL
    assert bool((S2[P > 0] == S2.amax(-1, keepdim=True).expand_as(S2)[P > 0]).all())
    assert float(torch.exp2(f32(-150.0))) == 0.0 and float(f32(2.0) ** -160) == 0.0


def exact_expected(path, q, k, v, do, route, keep_dS=False):
    """the exact results of family 1 from the exact P, in float64 (every value a small dyadic number), then the one fp32
    multiplication by the kernel's constant where there is one -> o, delta, dq, dk, dv (fp32), lse and its denominator (float64)"""
    qe, kk, vv, gg, factor, scale = path_operands(path, q, k, v, do)
    hd = q.shape[-1]
    kmul = scale32(hd) if path == 'f32' else LN2_32
    out = {}
    for b in range(q.shape[0]):                       # batch after batch, as attn64
        P = route_P(route, b)
        Q, K, V, G_ = qe[b].double(), kk[b].double(), vv[b].double(), gg[b].double()
        o = P @ V
        delta = (o * G_).sum(-1)
        dS = P * (G_ @ V.transpose(-1, -2) - delta[..., None])
        dq, dk = (dS @ K).float(), (dS.transpose(-1, -2) @ Q).float()
        assert torch.equal(dq.double(), dS @ K) and torch.equal(dk.double(), dS.transpose(-1, -2) @ Q)      # exact sums
        r = dict(o=o.float(), delta=delta.float(), dq=dq * scale32(hd), dk=dk * kmul, dv=(P.transpose(-1, -2) @ G_).float(),
                 lse=(factor * Q @ K.transpose(-1, -2)).amax(-1) + torch.log((P > 0).sum(-1).double()),
                 lse_den=factor * (Q.abs() @ K.abs().transpose(-1, -2)).amax(-1))
        if keep_dS:
            r['dS'] = dS
        for n, t in r.items():
            out.setdefault(n, []).append(t)
    return {n: torch.stack(t) for n, t in out.items()}


@pytest.mark.parametrize('hd', [32, 64])
@pytest.mark.parametrize('mode', ['route', 'tie', 'tie-split'])
def test_exact_families_in_the_rounding_model(hd, mode):
    """family 1 on the CPU statement of the bf16 paths: the recomputed backward P rounds to exactly 1.0 (0.5) in bf16, dS is the exact
    value, and every result is bitwise the expected one"""
    B, H, N = 2, 3, 300
    q, k, v, do, route = exact_inputs(mode, B, H, N, hd, 6)
    P = route_P(route)
    qe, k16, v16, g16, _, _ = path_operands('mfma', q, k, v, do)
    assert torch.equal(k16, k) and torch.equal(v16, v) and torch.equal(g16, do) and torch.equal(qe, q * rne(c32(hd)))
    want = exact_expected('mfma', q, k, v, do, route, keep_dS=True)
    lse64 = want['lse']
    fwd = model_bf16(qe, k16, v16, do, want['o'], torch.zeros(B, H, N))
    assert torch.equal(fwd['o'], want['o'])
    m = model_bf16(qe, k16, v16, do, fwd['o'], fwd['lse'])
    assert torch.equal(rne(m['P']), P.float()), float((m['P'] - P.float()).abs().max())
    assert float((m['P'].double() / P.clamp_min(1e-300) - 1)[P > 0].abs().max()) < 2.0 ** -9
    assert torch.equal(m['dS'].double(), want['dS'])
    for n in ('delta', 'dq', 'dk', 'dv'):
        assert torch.equal(m[n], want[n]), n
    assert float((m['lse'].double() - lse64).abs().max()) <= 2.0 ** -22 * float(lse64.abs().max())
    if mode == 'route':
        assert not m['dq'].any() and not m['dk'].any() and torch.equal(want['o'], torch.gather(v, 2, P.argmax(-1)[..., None].expand_as(v)))
        assert bool((m['dv'][(P > 0).sum(-2) == 0] == 0).all())
    else:
        assert bool(m['dk'].any())
        assert bool(m['dq'][..., hd - 2:].any()) == (mode == 'tie-split') and not m['dq'][..., :hd - 2].any()
    cs = colsum_parts(m).double().sum(0)
    if mode == 'route':
        assert float(cs.abs().max()) + 8 < 2 ** 24 and torch.equal(cs, cs.round())


def test_uniform_in_the_models():
    B, H, N, hd = 2, 3, 300, 32
    q, k, v, do, _ = exact_inputs('uniform', B, H, N, hd, 7)
    for path in ('mfma', 'bf16in'):                   # (torch's fp32 softmax normalises BEFORE the sum: N roundings, not the kernels' statement)
        o = models(path, q, k, v, do, torch.zeros(B, H, N, hd), torch.zeros(B, H, N))[0]
        mean = v.double().mean(-2, keepdim=True).expand(B, H, N, hd)
        assert float(_ratio((o['o'].double() - mean).abs(), mean.abs()).max()) <= 2 * 2.0 ** -23
        assert float((o['lse'].double() - math.log(N)).abs().max()) <= 2 * 2.0 ** -23 * math.log(N)
    wrong = v.double().sum(-2) / (N + 1)                              # a padded key counted in
    assert float(_ratio((wrong - v.double().mean(-2)).abs(), v.double().mean(-2).abs()).min()) > 100 * 2.0 ** -22


def test_reference_against_autograd():
    B, H, N, hd = 2, 3, 37, 32
    q, k, v, do = family('plain', B, H, N, hd, 8)
    for path in ('f32', 'mfma'):
        qe, kk, vv, gg, factor, scale = path_operands(path, q, k, v, do)
        Q, K, V = (t.double().clone().requires_grad_(True) for t in (qe, kk, vv))
        S = factor * Q @ K.transpose(-1, -2)
        o = torch.softmax(S, -1) @ V
        o.backward(gg.double())
        val, den = attn64(qe, kk, vv, gg, factor, scale)
        chk = dict(o=o.detach(), lse=torch.logsumexp(S, -1).detach(), dq=Q.grad * (scale / factor), dk=K.grad, dv=V.grad,
                   delta=(o.detach() * gg.double()).sum(-1))
        for n, t in chk.items():
            assert float((val[n] - t).abs().max()) < 1e-12, (path, n)
            assert bool((den[n] >= val[n].abs() - 1e-12).all()) or n == 'lse', n
    # the same through the packed layout and plain softmax attention with the true scale
    x = pack(q, k, v).double().requires_grad_(True)
    qq, kk, vv = unpack(x, B, H, N, hd)
    out = torch.softmax(qq @ kk.transpose(-1, -2) * hd ** -0.5, -1) @ vv
    out.backward(do.double())
    val, _ = attn64(q, k, v, do, hd ** -0.5, hd ** -0.5)
    assert float((colsum_parts(val) - x.grad).abs().max()) < 1e-12 and float((rows(val['o']) - rows(out.detach())).abs().max()) < 1e-12
    assert torch.equal(heads(rows(q), B, H, N, hd), q)


@pytest.mark.parametrize('hd,N,step', [(32, 257, 32), (32, 513, 64), (64, 129, 32), (64, 545, 64), (32, 33, 32)])
@pytest.mark.parametrize('fam', FAMILIES)
def test_input_families_have_their_properties(fam, hd, N, step):
    B, H = 1, 2
    qblocks, ktiles, _ = fwd_kernel(N, hd, B, H)
    assert step == 32 * ktiles
    q, k, v, do = family(fam, B, H, N, hd, 9, step)
    S2 = (rne(q * c32(hd)) @ rne(k).transpose(-1, -2))[0, 0]
    log = reference_moves(S2, step, 32 * qblocks)                # <64, 1, 2, 128>: 64-key steps, but 32 queries per wave
    later = log[1:]
    moved = [bool(n.any()) for _, n in later]
    val, den = attn64(*path_operands('mfma', q, k, v, do))
    pmax = torch.softmax(S2.double() * math.log(2), -1).amax(-1)
    if fam == 'plain':
        assert float(pmax.median()) < 0.5 and 0.9 < float(q.std()) < 1.1
    if fam == 'peaked':
        assert float(pmax.median()) > 0.5
    if fam == 'offset':
        assert float(val['lse'].min()) > 100
    if fam == 'all-negative':                                    # a padded key's unmasked exp2(0 - lse LOG2E) is +inf for EVERY query
        assert float(val['lse'].max()) < -100 and bool(torch.isinf(torch.exp2(-val['lse'].float() * LOG2E32)).all())
        assert float(S2.max()) < -100
    if fam == 'ascending' and N > 2 * step:
        skipped = [float(tm.max()) for (tm, n) in later if not n.any()]
        assert any(moved) and skipped and max(skipped) > 4 and max(skipped) <= SM_THR       # P up to 2^(4..8) above the reference
        assert all(float(tm.min()) > 0 for tm, _ in later[:-1])                              # every full step raises the maximum
    if fam == 'ascending-steep' and N > 2 * step:
        assert moved == [i % 2 == 0 for i in range(len(later))], moved                       # taken, skipped, taken, ..
        assert all(float(tm.min()) > 30 for (tm, n) in later if n.any())
    if fam == 'descending':
        assert not any(moved) and bool((S2.argmax(-1) < step).all())
    if fam == 'late':
        assert bool((S2.argmax(-1) == N - 1).all()) and (moved[-1] if later else True) and float(pmax.min()) > 0.99
    if fam == 'negative-first':
        assert float(log[0][0].max()) < -30 and (moved[0] if later else True)
    for path in PATHS:                                           # the models are sane on every family
        _, _, _, _, em = model_errors(path, q, k, v, do, torch.ones(3 * H * hd))
        for n, e in em.items():
            assert e <= model_cap(path, n, q, k), (fam, path, n, e)


def test_new_metric_sees_what_the_old_one_missed():
    """A zero-filled tail key counted into every row's sum, and one row that lost its last valid key: under max|a - b| / max|b|
    both pass the old 2e-2; per element each is outside the bound (the tail key narrowly on N(0, 1) — on q = 0, below, by three orders of
    magnitude)."""
    B, H, N, hd = 1, 2, 217, 32
    q, k, v, do = family('plain', B, H, N, hd, 10)
    val, den, o_in, lse_in, em = model_errors('mfma', q, k, v, do)
    honest = models('mfma', q, k, v, do, o_in, lse_in)[0]['o']
    bound = max(FACTOR * em['o'], FLOOR)
    tail = honest * (N / (N + 1.0))                           # one padded key (v = 0, p = mean p) in every divisor
    qe, _, v16, _, _, _ = path_operands('mfma', q, k, v, do)
    p = torch.softmax((qe[0, 0, 100] @ rne(k[0, 0]).T).double() * math.log(2), -1)
    p[N - 1] = 0                                              # the last valid key masked out of row 100 of head 0
    onerow = honest.clone()
    onerow[0, 0, 100] = ((p / p.sum()) @ v16[0, 0].double()).float()
    for name, got in (('tail key', tail), ('one wrong row', onerow)):
        old = float((got.double() - val['o']).abs().max() / val['o'].abs().max())
        e = elem_err(got, val['o'], den['o'])
        assert old < 2e-2 and e > bound, (name, old, e, bound)
    qu, ku, vu, _, _ = exact_inputs('uniform', 1, 1, 217, 32, 11)
    o = models('mfma', qu, ku, vu, vu, vu, torch.zeros(1, 1, 217))[0]['o']
    mean = vu.double().mean(-2, keepdim=True).expand_as(o)
    assert float(_ratio((o.double() * (N / (N + 1.0)) - mean).abs(), mean.abs()).max()) > 1000 * 2.0 ** -22


# =========================================================================== the GPU harness
@pytest.fixture(scope='module')
def lib():
    from vit_ae_plus_plus_amd._abi import lib as L
    L.load()
    return L


def st():
    return torch.cuda.current_stream().cuda_stream


def _p(b):
    return None if b is None else b.ptr


def _in(t, dtype=F32):
    """an input inside NaN: one guard row before and after, GUARD elements behind"""
    t = t.reshape(1, -1) if t.dim() == 1 else t
    return Buf(t.shape[0], t.shape[1], None, dtype, NAN, t)


def _out(rows, width, dtype=F32, refused=False, data=None):
    return Buf(rows, width, None, dtype, SENT, None if refused else data, SENT if refused else NAN)


def _guards(outs, refused, what):
    for name, o in outs.items():
        if o is not None:
            assert o.untouched() if refused else o.clean(), f'{what}: the guards of {name} were written'


def fwd_call(lib, path, q, k, v, o16=True, expect=0):
    """one forward of a path on q, k, v [B, H, N, hd] (CPU fp32; 'bf16in' stores them as bf16) -> o [B, H, N, hd], lse [B, H, N]"""
    dll = lib.load()
    B, H, N, hd = q.shape
    D, refused = H * hd, expect != 0
    X = _in(pack(q, k, v), BF16 if path == 'bf16in' else F32)
    O, L = _out(B * N, D, refused=refused), _out(1, B * H * N, refused=refused)
    O16 = _out(B * N, D, BF16, refused) if o16 and path != 'f32' else None
    if path == 'f32':
        rc = dll.vitae_sdpa_fwd(X.ptr, O.ptr, L.ptr, B, N, H, hd, st())
    else:
        fn = dll.vitae_sdpa_mfma_fwd if path == 'mfma' else dll.vitae_sdpa_mfma_fwd_bf16in
        rc = fn(X.ptr, O.ptr, _p(O16), L.ptr, B, N, H, hd, st())
    torch.cuda.synchronize()
    assert rc == expect, (path, rc, expect)
    _guards(dict(o=O, lse=L, o16=O16), refused, f'{path} forward N={N}')
    if refused:
        return None, None
    o = O.cpu()
    if O16 is not None:
        assert torch.equal(O16.cpu(), o.to(BF16)), 'o16 != bf16(o)'
    return heads(o, B, H, N, hd), L.cpu().view(B, H, N)


def bwd_call(lib, path, q, k, v, o, do, lse, want32=True, want16=True, old_cs=None, delta=True, expect=0):
    """one backward of a path -> dq, dk, dv [B, H, N, hd] (from dqkv, or from dqkv16 when dqkv == NULL), cs [3 H hd] | None,
    delta [B, H, N] | None (None too where the one-launch backward left the workspace untouched: asserted)"""
    dll = lib.load()
    B, H, N, hd = q.shape
    D, refused = H * hd, expect != 0
    X = _in(pack(q, k, v), BF16 if path == 'bf16in' else F32)
    O, G_, L = _in(rows(o)), _in(rows(do)), _in(lse.reshape(-1))
    DQ = _out(B * N, 3 * D, refused=refused) if want32 else None
    DQ16 = _out(B * N, 3 * D, BF16, refused) if want16 and path != 'f32' else None
    CS = _out(1, 3 * D, refused=refused, data=old_cs) if old_cs is not None and path != 'f32' else None
    DW = _out(1, B * H * N, refused=refused) if delta else None
    if path == 'f32':
        rc = dll.vitae_sdpa_bwd(X.ptr, O.ptr, G_.ptr, L.ptr, _p(DQ), _p(DW), B, N, H, hd, st())
    else:
        fn = dll.vitae_sdpa_mfma_bwd if path == 'mfma' else dll.vitae_sdpa_mfma_bwd_bf16in
        rc = fn(X.ptr, O.ptr, G_.ptr, L.ptr, _p(DQ), _p(DQ16), _p(CS), _p(DW), B, N, H, hd, st())
    torch.cuda.synchronize()
    assert rc == expect, (path, rc, expect)
    _guards(dict(dqkv=DQ, dqkv16=DQ16, colsum=CS, delta=DW), refused, f'{path} backward N={N}')
    if refused:
        return None
    if DQ is not None and DQ16 is not None:
        assert torch.equal(DQ16.cpu(), DQ.cpu().to(BF16)), 'dqkv16 != bf16(dqkv)'
    dq, dk, dv = unpack((DQ if DQ is not None else DQ16).cpu().float(), B, H, N, hd)
    dl = None
    if DW is not None:
        if path != 'f32' and fits(N, hd):
            assert bool(DW.view.isnan().all()), 'the one-launch backward wrote the delta workspace'
        else:
            dl = DW.cpu().view(B, H, N)
    return types.SimpleNamespace(dq=dq, dk=dk, dv=dv, cs=None if CS is None else CS.cpu().view(-1), delta=dl)


def old_colsum(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(1, 9, (n,), generator=g).float() * (1 - 2 * torch.randint(0, 2, (n,), generator=g)).float()


def model_lse(path, q, k):
    """the lse of the CPU statements alone (batch after batch)"""
    hd = q.shape[-1]
    outs = []
    for b in range(q.shape[0]):
        if path == 'f32':
            qs = q[b] * scale32(hd)
            outs.append([torch.logsumexp(S, -1) for S in (qs @ k[b].transpose(-1, -2), running_scores(qs, k[b]))])
        else:
            S2 = rne(q[b] * c32(hd)) @ rne(k[b]).transpose(-1, -2)
            m = S2.amax(-1, keepdim=True)
            outs.append([((m + torch.log2(torch.exp2(S2 - m).sum(-1, keepdim=True)))[..., 0] * LN2_32)])
    return [torch.stack(t) for t in zip(*outs)]


def check_colsum(label, cs, old, parts64, parts_den, parts_model, exact_cols=None):
    """column sums: bitwise on `exact_cols` (a mask over 3 H hd), family 2's bound on the rest"""
    cs64 = old.double() + parts64.double().sum(0)
    if exact_cols is not None:
        assert torch.equal(cs[exact_cols], cs64.float()[exact_cols]), label + ': exact column sums'
        if bool(exact_cols.all()):
            return
    den = old.double().abs() + parts_den.double().sum(0)
    within(label + ' colsum', elem_err(cs, cs64, den), elem_err(seq_colsum(parts_model, old), cs64, den))


def exact_case(lib, path, mode, B, N, H, hd, seed):
    """family 1 for one path, mode and shape: forward, backward, the optional-output forms"""
    q, k, v, do, route = exact_inputs(mode, B, H, N, hd, seed)
    label = f'{path}/{mode}/hd{hd}/N{N}/BH{B * H}'
    if path != 'f32':
        assert lib.load().vitae_sdpa_bwd_fused_fits(N, hd) == fits(N, hd)
    o, lse = fwd_call(lib, path, q, k, v)
    if mode == 'uniform':
        mean = v.double().mean(-2, keepdim=True).expand(B, H, N, hd)
        assert float(_ratio((o.double() - mean).abs(), mean).max()) <= 2 * 2.0 ** -23, label
        assert float((lse.double() - math.log(N)).abs().max()) <= 2 * 2.0 ** -23 * math.log(N), label
        return
    want = exact_expected(path, q, k, v, do, route)
    assert torch.equal(o, want['o']), label + ': o'
    lm = model_lse(path, q, k)
    within(label + ' lse', elem_err(lse, want['lse'], want['lse_den']), max(elem_err(m, want['lse'], want['lse_den']) for m in lm))
    if path == 'f32' and mode != 'route':
        quality_case(lib, path, q, k, v, do, label, fwd=False)          # p = expf(s - m - logf(2)) is not exactly 1/2
        return
    old = old_colsum(3 * H * hd, seed + 1)
    r = bwd_call(lib, path, q, k, v, want['o'], do, lse if path == 'f32' else lm[0], old_cs=old)
    for n in ('dq', 'dk', 'dv'):
        assert torch.equal(getattr(r, n), want[n]), f'{label}: {n}'
    if mode == 'route':
        assert not want['dq'].any() and not want['dk'].any()
    if r.delta is not None:
        assert torch.equal(r.delta, want['delta']), label + ': delta'
    if r.cs is not None:
        D = H * hd
        exact_cols = torch.ones(3 * D, dtype=torch.bool)
        if mode != 'route':
            exact_cols[:2 * D] = False                                   # rounded products added in an order the atomics choose
        check_colsum(label, r.cs, old, colsum_parts(want), colsum_parts({n: want[n].abs() for n in ('dq', 'dk', 'dv')}),
                     colsum_parts(want), exact_cols)
    if path != 'f32' and mode == 'route' and fits(N, hd):
        # dqkv == NULL and dbias == NULL (and, from bf16 qkv, no delta workspace): the bf16 gradient alone
        r = bwd_call(lib, path, q, k, v, want['o'], do, lm[0], want32=False, delta=path == 'mfma')
        for n in ('dq', 'dk', 'dv'):
            assert torch.equal(getattr(r, n), rne(want[n])), f'{label}: {n} (bf16 only)'


def quality_case(lib, path, q, k, v, do, label, fwd=True):
    """family 2 for one path on given inputs: every output per element against float64"""
    B, H, N, hd = q.shape
    if path == 'bf16in':
        q, k, v = rne(q), rne(k), rne(v)
    old = old_colsum(3 * H * hd, N + hd) if path != 'f32' else None
    val, den, o_in, lse_in, em = model_errors(path, q, k, v, do, old)
    for n, e in em.items():
        assert e <= model_cap(path, n, q, k), (label, 'model', n, e)
    if fwd:
        o, lse = fwd_call(lib, path, q, k, v)
        within(f'{label} o', elem_err(o, val['o'], den['o']), em['o'])
        within(f'{label} lse', elem_err(lse, val['lse'], den['lse']), em['lse'])
    r = bwd_call(lib, path, q, k, v, o_in, do, lse_in, old_cs=old)
    for n in ('dq', 'dk', 'dv'):
        within(f'{label} {n}', elem_err(getattr(r, n), val[n], den[n]), em[n])
    if r.cs is not None:
        within(f'{label} colsum', elem_err(r.cs, val['colsum'], den['colsum']), em['colsum'])
    if r.delta is not None:                                              # rowsum(o dO) of the fp32 o and the fp32 dO it was given
        d64, dden = (o_in.double() * do.double()).sum(-1), (o_in.double() * do.double()).abs().sum(-1)
        within(f'{label} delta', elem_err(r.delta, d64, dden), elem_err((o_in * do).sum(-1), d64, dden))


# =========================================================================== family 1 on every shape of the dispatch table
BF16_SHAPES = ([(32, n, 2, 3) for n in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 160, 257, 300, 385, 448, 449, 512, 513, 577, 641)] +
               [(64, n, 2, 3) for n in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 160, 256, 257, 385, 512, 545)] +
               [(32, n, 1, 1) for n in (1, 33, 65, 129, 300, 448)] + [(64, n, 1, 1) for n in (1, 33, 65, 256)] +
               [(32, 1, 32, 16), (64, 1, 32, 16), (32, 129, 32, 16), (32, 161, 32, 16), (32, 257, 32, 16)])
F32_SHAPES = ([(hd, n, 2, 3) for hd in (32, 64) for n in (1, 31, 32, 33, 127, 128, 129, 161)] +
              [(16, n, 2, 3) for n in (1, 127, 129)] + [(128, n, 2, 3) for n in (1, 31, 33, 65)])


@gpu
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('path', ['mfma', 'bf16in'])
@pytest.mark.parametrize('hd,N,B,H', BF16_SHAPES)
def test_bf16_attention_exact(lib, path, mode, hd, N, B, H):
    exact_case(lib, path, mode, B, N, H, hd, seed=N + hd)


@gpu
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('hd,N,B,H', F32_SHAPES)
def test_f32_attention_exact(lib, mode, hd, N, B, H):
    exact_case(lib, 'f32', mode, B, N, H, hd, seed=N + hd)


@gpu
@pytest.mark.parametrize('hd,N', [(32, 129), (128, 33)])
def test_f32_forward_routes_arbitrary_values(lib, hd, N):
    """the fp32 kernels' forward multiplies V by p = 1 exactly: any fp32 V comes through bitwise"""
    B, H = 2, 3
    q, k, v, do, route = exact_inputs('route', B, H, N, hd, 3)
    v = torch.randn(B, H, N, hd, generator=torch.Generator().manual_seed(4)) * 1e3
    o, _ = fwd_call(lib, 'f32', q, k, v)
    assert torch.equal(o, torch.gather(v, 2, route[0][..., None].expand_as(v)))


# =========================================================================== family 2
BF16_QUALITY = [(32, 33, 2, 3), (32, 129, 2, 3), (32, 300, 2, 3), (32, 449, 2, 3), (32, 513, 2, 3), (64, 33, 2, 3), (64, 129, 2, 3), (64, 257, 2, 3), (64, 545, 2, 3)]
F32_QUALITY = [(32, 33), (32, 161), (64, 129), (16, 129), (128, 65)]


@gpu
@pytest.mark.parametrize('fam', FAMILIES)
@pytest.mark.parametrize('path', ['mfma', 'bf16in'])
@pytest.mark.parametrize('hd,N,B,H', BF16_QUALITY)
def test_bf16_attention_rounding(lib, path, fam, hd, N, B, H):
    q, k, v, do = family(fam, B, H, N, hd, seed=N + hd, step=32 * fwd_kernel(N, hd, B, H)[1])
    quality_case(lib, path, q, k, v, do, f'{path}/{fam}/hd{hd}/N{N}/BH{B * H}')


@gpu
@pytest.mark.parametrize('fam', ['plain', 'ascending-steep', 'late'])
@pytest.mark.parametrize('path', ['mfma', 'bf16in'])
def test_bf16_attention_rounding_two_query_blocks(lib, path, fam):
    """<32, 2, 2, 128> below N = 512 (B H = 512) and the one-launch backward with one workgroup per head"""
    hd, N, B, H = 32, 161, 32, 16
    assert fwd_kernel(N, hd, B, H) == (2, 2, 128) and fused_groups(N, B, H) == 1
    q, k, v, do = family(fam, B, H, N, hd, seed=N + hd, step=64)
    quality_case(lib, path, q, k, v, do, f'{path}/{fam}/hd{hd}/N{N}/BH{B * H}')


@gpu
@pytest.mark.parametrize('fam', FAMILIES)
@pytest.mark.parametrize('hd,N', F32_QUALITY)
def test_f32_attention_rounding(lib, fam, hd, N):
    B, H = 2, 3
    q, k, v, do = family(fam, B, H, N, hd, seed=N + hd)
    quality_case(lib, 'f32', q, k, v, do, f'f32/{fam}/hd{hd}/N{N}/BH{B * H}')


@pytest.mark.parametrize('path,hd,N,B,H', [(p, *s) for p in ('mfma', 'bf16in') for s in BF16_QUALITY + [(32, 161, 32, 16)]] +
                         [('f32', hd, n, 2, 3) for hd, n in F32_QUALITY])
def test_model_caps_on_the_gpu_cases(path, hd, N, B, H):
    """e_model of every family-2 case stays under its cap (a broken model cannot loosen a bound)"""
    B = min(B, 2)                                     # (the first two batches of the B H = 512 case)
    step = 32 if path == 'f32' else 32 * fwd_kernel(N, hd, 32 if H == 16 else B, H)[1]
    for fam in FAMILIES:
        q, k, v, do = family(fam, B, H, N, hd, seed=N + hd, step=step)
        if path == 'bf16in':
            q, k, v = rne(q), rne(k), rne(v)
        em = model_errors(path, q, k, v, do, old_colsum(3 * H * hd, N + hd))[4]
        for n, e in em.items():
            assert 0 <= e <= model_cap(path, n, q, k), (fam, n, e)


# =========================================================================== refusals: host-side checks that write nothing
@gpu
def test_refusals_write_nothing(lib):
    INVAL, UNSUP = -1, -2                             # VITAE_ERR_INVALID_ARG, VITAE_ERR_UNSUPPORTED_SHAPE (include/vitae_hip.h)
    B, H, N = 2, 3, 33
    for hd in (48, 16):                               # no MFMA instantiation
        q, k, v, do = family('plain', B, H, N, hd, 1)
        lse = torch.zeros(B, H, N)
        for path in ('mfma', 'bf16in'):
            fwd_call(lib, path, q, k, v, expect=UNSUP)
            assert bwd_call(lib, path, q, k, v, v, do, lse, old_cs=old_colsum(3 * H * hd, 2), expect=UNSUP) is None
    q, k, v, do = family('plain', B, H, N, 48, 1)
    fwd_call(lib, 'f32', q, k, v, expect=UNSUP)
    bwd_call(lib, 'f32', q, k, v, v, do, torch.zeros(B, H, N), expect=UNSUP)
    q, k, v, do = family('plain', B, H, N, 20, 1)     # H hd = 60: not a multiple of 8 (the bf16 rows would not be 16-byte aligned)
    fwd_call(lib, 'bf16in', q, k, v, expect=UNSUP)
    bwd_call(lib, 'bf16in', q, k, v, v, do, torch.zeros(B, H, N), old_cs=old_colsum(180, 2), expect=UNSUP)
    for path, hd, n in (('bf16in', 32, 449), ('bf16in', 64, 257), ('mfma', 32, 449), ('mfma', 32, 33)):
        assert fits(n, hd) == (n == 33)               # delta_ws == NULL: the two-kernel route needs it, vitae_sdpa_mfma_bwd always asks for it
        q, k, v, do = family('plain', 1, H, n, hd, 1)
        bwd_call(lib, path, q, k, v, v, do, torch.zeros(1, H, n), old_cs=old_colsum(3 * H * hd, 2), delta=False, expect=INVAL)
