"""
qingdai_amd/order.py -- the two building blocks of the device's summation order (csrc/qd_blockred.h), in NumPy.  The references
that restate a kernel's order bit for bit (series.reduce_reference, spectra.combine_reference, flow, spharm, eddy) are built from
them.
"""
from __future__ import annotations

import numpy as np


def wave(x, op):
    """The five-halving wave reduction of csrc/qd_blockred.h over the last axis (64 lanes) -> what lane 0 holds."""
    x = np.array(x, copy=True)
    o = 32
    while o > 0:
        x[..., :o] = op(x[..., :o], x[..., o:2 * o])
        o >>= 1
    return x[..., 0]


def lanes(v, width, fill):
    """[..., m] -> [..., rounds, width]: element k * width + l is lane l's k-th; `fill` where the plane ends."""
    m = v.shape[-1]
    rounds = max(1, -(-m // width))
    out = np.full(v.shape[:-1] + (rounds * width,), fill, dtype=np.float64)
    out[..., :m] = v
    return out.reshape(v.shape[:-1] + (rounds, width))
