"""numpy statement of the rate-distortion check of an inter TU's levels against no levels
(``hv::rd_cbf_tu``, csrc/kernels/hevc_rdcbf.h; ``HevcParams.rd_cbf``).  Plain Python integers; it
builds on the quantiser model of tests/ref_models_hevc_rdoq.py (``transform_quant_block``,
``positions``, ``rate`` and the bin costs) and imports nothing of the package.

This docstring is the normative text of the check.  All arithmetic is integer.

The check applies to one TU of one component of an inter CU, after the block function has produced
its levels (dead zone, sign data hiding and RDOQ included: the check sees the final levels) and
the dequantised, inverse-transformed residual R'.  With src and pred the TU's source and
prediction samples and maxv = 2^bit_depth - 1:

* ``D0 = sum (src - pred)^2`` and ``D1 = sum (src - clip(pred + R', 0, maxv))^2`` over the TU.
* ``Rb``, the rate of the levels in 1 / 16 bit.  Inter TUs scan diagonally (scanIdx 0); with
  ``pmax`` the largest coder scan position that holds a non-zero level, Rb is the sum of
  ``rate(|l|, seen=False, pmax)`` for the level at pmax, ``rate(|l|, seen=True, p)`` for every
  ``p < pmax`` whose 4x4 group holds a non-zero level (the zeros of an all-zero group cost
  nothing), and, for every group strictly between group 0 and the group of pmax, ``CSBF1`` when it
  holds a level, else ``CSBF0``.  A 4x4 TU has no group flags.
* The cbf flag itself costs ``CBF0 = 8`` when zero and ``CBF1 = 18`` when set (design constants,
  the values of the sub-block flag).
* ``lamq = round(rd_cbf_lambda * 0.57 * 2^((QpY - 12) / 3) * 4^(bit_depth - 8) * 16)``, HM's SSD
  lambda in 1 / 16 units (round = floor(x + 0.5) in float64), tabulated for QpY 0..51 and read at
  the CTB's QpY clamped to that range; chroma reads the same entry.
* The TU is cleared when ``256 * D0 + lamq * CBF0 <= 256 * D1 + lamq * (Rb + CBF1)``; ties clear.
  Cleared: every level is zero, R' is zero (the reconstruction is the prediction), the flag is 0.
* A TU without levels is not examined (its D1 is reported as D0, its Rb as 0).
"""
import math

import numpy as np

import ref_models_hevc_rdoq as rq

CBF0, CBF1 = 8, 18


def lamq_of(rd_cbf_lambda, qp_y, bit_depth):
    return int(math.floor(rd_cbf_lambda * 0.57 * 2.0 ** ((qp_y - 12) / 3.0) * 4.0 ** (bit_depth - 8) * 16.0 + 0.5))


def lamq_table(rd_cbf_lambda, bit_depth):
    """the 52 entries the kernel indexes by clamp(QpY, 0, 51)"""
    return [lamq_of(rd_cbf_lambda, q, bit_depth) for q in range(52)]


def tu_rate(lev, log2n):
    """Rb of the levels [v, u] of an inter TU (0 for a TU without levels)"""
    order, _ = rq.positions(0, log2n)
    a = [abs(int(lev[y, x])) for x, y in order]
    nzp = [p for p, l in enumerate(a) if l]
    if not nzp:
        return 0
    pmax = nzp[-1]
    ngr = len(a) // 16
    has = [any(a[16 * g: 16 * g + 16]) for g in range(ngr)]
    r = rq.rate(a[pmax], False, pmax)
    r += sum(rq.rate(a[p], True, p) for p in range(pmax) if has[p // 16])
    r += sum(rq.CSBF1 if has[g] else rq.CSBF0 for g in range(1, pmax // 16))
    return r


def clears(d0, d1, rb, lamq):
    return 256 * int(d0) + int(lamq) * CBF0 <= 256 * int(d1) + int(lamq) * (int(rb) + CBF1)


def rd_cbf_tu(src, pred, dct32, log2n, bd, qp, lamq, sdh=False, rdoq=0, lam=0):
    """(levels, reconstructed samples, flag, D0, D1, Rb) of a source / prediction block [y, x] at
    Qp' = qp; D1 and Rb are the terms of the comparison, also of a TU that it cleared"""
    maxv = (1 << bd) - 1
    src, pred = np.asarray(src, dtype=np.int64), np.asarray(pred, dtype=np.int64)
    res = src - pred
    d0 = int((res * res).sum())
    lev, rres, flag = rq.transform_quant_block(res, dct32, log2n, bd, qp, False, False, 0, sdh, rdoq, lam)
    if not flag:
        return lev, pred.copy(), 0, d0, d0, 0
    rec = np.clip(pred + rres, 0, maxv)
    d1 = int(((src - rec) ** 2).sum())
    rb = tu_rate(lev, log2n)
    if clears(d0, d1, rb, lamq):
        return np.zeros_like(lev), pred.copy(), 0, d0, d1, rb
    return lev, rec, 1, d0, d1, rb
