"""What the host sequencing modules (engine.py, encoder.py) share around a launch: ABI constants by name, pointer / padding
helpers and the split-K fit."""
from __future__ import annotations

from ._abi import CONSTS as _C

PREC = {'fp32': _C['VITAE_PREC_F32'], 'bf16': _C['VITAE_PREC_BF16'], 'fp32x3': _C['VITAE_PREC_BF16X3']}
EPI_NONE, EPI_GELU, EPI_DGELU, EPI_RELU = (_C['VITAE_EPI_NONE'], _C['VITAE_EPI_GELU'], _C['VITAE_EPI_DGELU'],
                                           _C['VITAE_EPI_RELU_MASK'])
EPI_AUX_BF16, EPI_AUX_DERIV = _C['VITAE_EPI_AUX_BF16'], _C['VITAE_EPI_AUX_DERIV']     # flags, OR-ed into an epilogue above bit 3


def ptr(t):
    return None if t is None else t.data_ptr()


def pad64(M):
    return (M + 63) // 64 * 64


def fit_split(cache, key, pick, need, capacity):
    """The split-K of one GEMM shape, cached under ``key``: what the planner ``pick()`` proposes, shrunk until the ``need(s)``
    floats of scratch it takes fit into ``capacity``.  Call sites look into ``cache`` first (``cache.get(key) or fit_split(...)``),
    so ``pick`` runs once per key.  A rule that depends on the epilogue (a GELU epilogue is never split) is applied by the call
    site OUTSIDE the cache unless the epilogue is part of ``key``: a cached value must not depend on anything the key leaves out."""
    s = pick()
    while s > 1 and need(s) > capacity:
        s -= 1
    cache[key] = s
    return s
