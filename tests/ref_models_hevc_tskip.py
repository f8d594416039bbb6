"""numpy statement of the transform skip decision of a 4x4 TU (``hv::tskip_tu``,
csrc/kernels/hevc_tskip.h; ``HevcParams.tskip``, x265 --tskip).  Plain Python integers; it builds on
the quantiser model of tests/ref_models_hevc_rdoq.py and the constants of
tests/ref_models_hevc_rdcbf.py and imports nothing of the package.

This docstring is the normative text of the decision.  All arithmetic is integer.

It applies to every coded 4x4 TU the encoder produces: intra luma 4x4 (PART_NxN PUs, DST-VII),
chroma 4x4 of 8x8 intra CUs and chroma 4x4 of 8x8 inter CUs (DCT).  With src and pred the TU's
source and prediction samples, r = src - pred, bd the bit depth and maxv = 2^bd - 1:

* Candidate A is the block function's result as configured (transform, dead zone or RDOQ, sign
  data hiding): levels lev_A and residual r'_A (zero for a TU without levels).
* Candidate B takes ``c[y][x] = r[y][x] << (13 - bd)`` (15 - bd - log2 with log2 = 2) as its
  coefficients, with no transform.  They go through the same quantiser at the same Qp' with the
  TU's own scanIdx (dead zone 171 intra / 85 inter, or RDOQ; then sign data hiding when on) to
  lev_B, are dequantised per 8.6.3 with flat m = 16:
  ``d = clip16((lev_B * 16 * LEVEL_SCALE[qp % 6] << (qp // 6)) + (1 << (bd - 4))) >> (bd - 3))``,
  and rescaled per 8.6.4.2 with transform_skip_flag:
  ``r'_B = ((d << 7) + (1 << (19 - bd))) >> (20 - bd)``.
* ``D_X = sum (src - clip(pred + r'_X, 0, maxv))^2`` and ``D0 = sum (src - pred)^2`` over the TU.
* ``R_X`` is the rate of X's levels in 1 / 16 bit from the static bin costs of the RDOQ model over
  the TU's own coder scan: with pmax the largest scan position that holds a non-zero level,
  ``rate(|l|, False, pmax)`` there plus ``rate(|l|, True, p)`` for every p < pmax; 0 without levels.
* ``TSF = 16`` is the cost of transform_skip_flag (one bit: both contexts start at initValue 139),
  ``CBF0 = 8`` and ``CBF1 = 18`` the cost of the cbf, as in the rd_cbf check.
* ``lamq = rd_cbf lamq_table(tskip_lambda, bd)[clamp(QpY, 0, 51)]``; chroma reads the same entry.
* If B has no levels, A stands.  Otherwise ``J_B = 256 * D_B + lamq * (R_B + TSF + CBF1)``, and
  ``J_A = 256 * D_A + lamq * (R_A + TSF + CBF1)`` when A has levels, else
  ``J_A = 256 * D0 + lamq * CBF0``.  B is chosen iff ``J_B < J_A``; ties keep A.
* The winner's levels, residual and flag are the TU's; where rd_cbf is on it then runs unchanged
  on them.
* Reported terms: D_A (= D0 when A has no levels), R_A, and D_B, R_B (D0 and 0 when B has no
  levels: it is not examined further).
"""
import numpy as np

import ref_models_hevc_rdcbf as rc
import ref_models_hevc_rdoq as rq

TSF = 16
CBF0, CBF1 = rc.CBF0, rc.CBF1


def ts_coef(res, bd):
    return np.asarray(res, dtype=np.int64) << (13 - bd)


def ts_inverse(d, bd):
    """8.6.4.2 with transform_skip_flag for a 4x4 block (tsShift = 5 + 2)"""
    return ((np.asarray(d, dtype=np.int64) << 7) + (1 << (19 - bd))) >> (20 - bd)


def ts_residual(lev, bd, qp):
    """r' of transform-skip levels [y, x] at Qp' = qp: what both decoders reconstruct"""
    return ts_inverse(rq.dequant(np.asarray(lev, dtype=np.int64), 2, bd, qp), bd)


def tu_rate4(lev, scan):
    """rate of a 4x4 TU's levels over its own scan (0 without levels)"""
    order, _ = rq.positions(scan, 2)
    a = [abs(int(lev[y, x])) for x, y in order]
    nzp = [p for p, l in enumerate(a) if l]
    if not nzp:
        return 0
    pmax = nzp[-1]
    return rq.rate(a[pmax], False, pmax) + sum(rq.rate(a[p], True, p) for p in range(pmax))


def chooses_b(d0, nz_a, d_a, r_a, d_b, r_b, lamq):
    """the comparison, for a B that has levels"""
    jb = 256 * int(d_b) + int(lamq) * (int(r_b) + TSF + CBF1)
    ja = 256 * int(d_a) + int(lamq) * (int(r_a) + TSF + CBF1) if nz_a else 256 * int(d0) + int(lamq) * CBF0
    return jb < ja


def tskip_tu(src, pred, dct32, bd, qp, lamq, intra, dst=False, scan=0, sdh=False, rdoq=0, lam=0):
    """(levels, reconstructed samples, transform_skip_flag, cbf, D_A, D_B, R_A, R_B) of a 4x4
    source / prediction block [y, x] at Qp' = qp"""
    maxv = (1 << bd) - 1
    src, pred = np.asarray(src, dtype=np.int64), np.asarray(pred, dtype=np.int64)
    res = src - pred
    d0 = int((res * res).sum())
    lev_a, res_a, nz_a = rq.transform_quant_block(res, dct32, 2, bd, qp, intra, dst, scan, sdh, rdoq, lam)
    rec_a = np.clip(pred + res_a, 0, maxv)
    d_a = int(((src - rec_a) ** 2).sum()) if nz_a else d0
    r_a = tu_rate4(lev_a, scan)
    lev_b = rq.quantise(ts_coef(res, bd), 2, bd, qp, intra, scan, sdh, rdoq, lam)
    if not lev_b.any():
        return lev_a, rec_a, 0, int(nz_a), d_a, d0, r_a, 0
    rec_b = np.clip(pred + ts_residual(lev_b, bd, qp), 0, maxv)
    d_b = int(((src - rec_b) ** 2).sum())
    r_b = tu_rate4(lev_b, scan)
    if chooses_b(d0, nz_a, d_a, r_a, d_b, r_b, lamq):
        return lev_b, rec_b, 1, 1, d_a, d_b, r_a, r_b
    return lev_a, rec_a, 0, int(nz_a), d_a, d_b, r_a, r_b
