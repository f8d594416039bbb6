"""Numpy model of HEVC inter sample prediction (clause 8.5.3.3) and of the forward proxy weight.

* :func:`interp` -- 8.5.3.3.3 fractional sample interpolation: the 8-tap luma / 4-tap chroma
  filters, reference coordinates clamped to the picture, the 14-bit intermediate predSamplesLX.
* :func:`weight_default` -- 8.5.3.3.4.2, default weighted sample prediction (uni and bi).
* :func:`weight_explicit` -- 8.5.3.3.4.3, explicit weighted sample prediction (uni and bi).
* :func:`predict` -- a block's prediction as a decoder forms it for given slice weights.
* :func:`wp_ref8` -- the forward-weighted 8-bit reference proxy of a weighted B step
  (csrc/kernels/weightp.hip wp_ref8).

Written from the standard's text; plain integer numpy (int64), loops over taps only.
"""
from __future__ import annotations

import numpy as np

LUMA_TAPS = np.array([[0, 0, 0, 64, 0, 0, 0, 0],
                      [-1, 4, -10, 58, 17, -5, 1, 0],
                      [-1, 4, -11, 40, 40, -11, 4, -1],
                      [0, 1, -5, 17, 58, -10, 4, -1]], dtype=np.int64)          # Table 8-11
CHROMA_TAPS = np.array([[0, 64, 0, 0], [-2, 58, 10, -2], [-4, 54, 16, -2], [-6, 46, 28, -4],
                        [-4, 36, 36, -4], [-4, 28, 46, -6], [-2, 16, 54, -4], [-2, 10, 58, -2]], dtype=np.int64)  # Table 8-12

DIR_L0, DIR_L1, DIR_BI = 1, 2, 3
LOG2_DENOM = 6   # luma_log2_weight_denom and the chroma denominator of this encoder's tables


def interp(ref: np.ndarray, bx: int, by: int, bw: int, bh: int, mvx: int, mvy: int, chroma: bool, bd: int) -> np.ndarray:
    """predSamplesLX [bh, bw] (int64, 14-bit scale) of the block at (bx, by) of plane ``ref`` for
    the vector (mvx, mvy) in quarter (luma) or eighth (chroma) samples."""
    ref = np.asarray(ref).astype(np.int64)
    ph, pw = ref.shape
    taps, fb = (CHROMA_TAPS, 3) if chroma else (LUMA_TAPS, 2)
    nt = taps.shape[1]
    before = nt // 2 - 1
    fx, fy = mvx & ((1 << fb) - 1), mvy & ((1 << fb) - 1)
    ix, iy = bx + (mvx >> fb), by + (mvy >> fb)
    shift1, shift2, shift3 = min(4, bd - 8), 6, 14 - bd
    xs = np.clip(ix - before + np.arange(bw + nt - 1), 0, pw - 1)
    ys = np.clip(iy - before + np.arange(bh + nt - 1), 0, ph - 1)
    win = ref[np.ix_(ys, xs)]                      # rows iy - before .., columns ix - before ..
    if fx == 0 and fy == 0:
        return win[before:before + bh, before:before + bw] << shift3
    if fy == 0:
        rows = win[before:before + bh]
        return sum(taps[fx, k] * rows[:, k:k + bw] for k in range(nt)) >> shift1
    if fx == 0:
        cols = win[:, before:before + bw]
        return sum(taps[fy, k] * cols[k:k + bh] for k in range(nt)) >> shift1
    tmp = sum(taps[fx, k] * win[:, k:k + bw] for k in range(nt)) >> shift1
    return sum(taps[fy, k] * tmp[k:k + bh] for k in range(nt)) >> shift2


def weight_default(p0, p1, bd: int) -> np.ndarray:
    """8.5.3.3.4.2: ``p1`` None = uni-prediction from ``p0``; else the average of both."""
    maxv = (1 << bd) - 1
    if p1 is None:
        sh = 14 - bd
        v = (np.asarray(p0, np.int64) + (1 << (sh - 1))) >> sh
    else:
        sh = 15 - bd
        v = (np.asarray(p0, np.int64) + np.asarray(p1, np.int64) + (1 << (sh - 1))) >> sh
    return np.clip(v, 0, maxv)


def weight_explicit(p0, w0: int, o0: int, p1, w1: int, o1: int, bd: int, log2_denom: int = LOG2_DENOM) -> np.ndarray:
    """8.5.3.3.4.3: offsets in 8-bit units (scaled by 2^(bd - 8), no high-precision offsets);
    ``p1`` None = uni-prediction with (w0, o0)."""
    maxv = (1 << bd) - 1
    lwd = log2_denom + 14 - bd
    sc = 1 << (bd - 8)
    p0 = np.asarray(p0, np.int64)
    if p1 is None:
        if lwd >= 1:
            v = ((p0 * w0 + (1 << (lwd - 1))) >> lwd) + o0 * sc
        else:
            v = p0 * w0 + o0 * sc
    else:
        v = (p0 * w0 + np.asarray(p1, np.int64) * w1 + ((o0 * sc + o1 * sc + 1) << lwd)) >> (lwd + 1)
    return np.clip(v, 0, maxv)


def predict(ref0, ref1, bx, by, bw, bh, direction: int, mv0, mv1, chroma: bool, bd: int, wp0=None, wp1=None,
            weighted: bool | None = None) -> np.ndarray:
    """A block's prediction samples.  ``wp0`` / ``wp1``: (w, o) of the component for
    RefPicList0[0] / RefPicList1[0], None = that list's flag is 0.  ``weighted`` (default: any
    weight given): whether the slice uses explicit weighting at all -- then a list without flag
    enters as (2^log2_denom, 0)."""
    if weighted is None:
        weighted = wp0 is not None or wp1 is not None
    p0 = interp(ref0, bx, by, bw, bh, mv0[0], mv0[1], chroma, bd) if direction & 1 else None
    p1 = interp(ref1, bx, by, bw, bh, mv1[0], mv1[1], chroma, bd) if direction & 2 else None
    if not weighted:
        return weight_default(p0, p1, bd) if direction & 1 else weight_default(p1, None, bd)
    ident = (1 << LOG2_DENOM, 0)
    a, b = wp0 or ident, wp1 or ident
    if direction == DIR_BI:
        return weight_explicit(p0, a[0], a[1], p1, b[0], b[1], bd)
    if direction == DIR_L0:
        return weight_explicit(p0, a[0], a[1], None, 0, 0, bd)
    return weight_explicit(p1, b[0], b[1], None, 0, 0, bd)


def wp_ref8(plane, w: int, o: int) -> np.ndarray:
    """clip8(((r * w + 32) >> 6) + o) of an 8-bit plane."""
    r = np.asarray(plane).astype(np.int64)
    return np.clip(((r * w + 32) >> 6) + o, 0, 255).astype(np.uint8)
