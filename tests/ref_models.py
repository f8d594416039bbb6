"""Plain numpy models of the kernels whose results never reach a decoder: the quality metrics
(csrc/kernels/metrics.hip and their host finish), the weighted-prediction statistics and the
inverse-weighted search source (weightp.hip), H.264 variance AQ (aq.hip) and the HEVC per-CTB
AQ (hevc_filters.hip).  A wrong result of any of them still gives a valid stream, so the
bit-exact decoder comparison cannot see it.

Everything here is int64 / float64 numpy written from the formulas the kernels document, with
no import of the package and none of its code.  tests/test_ref_models.py pins the models on
hand-computed cases; the GPU tests compare the kernels with them.
"""
from __future__ import annotations

import numpy as np

SSIM_C1 = 6.5025    # (0.01 * 255)^2
SSIM_C2 = 58.5225   # (0.03 * 255)^2
AQ_SCALE = 1.0397   # x264 aq-mode 1
AQ_BIAS = 14.427    # for 8-bit samples; + 2 per extra bit of depth


# ------------------------------------------------------------------ quality metrics
def sse_planes(src, rec, w: int, h: int) -> np.ndarray:
    """src, rec: (y, u, v) planes of one picture at any coded size >= (h, w); -> int64 [3], the
    sums of squared differences over the display window (w x h luma, w/2 x h/2 chroma)."""
    out = np.zeros(3, dtype=np.int64)
    for c in range(3):
        ph, pw = (h, w) if c == 0 else (h // 2, w // 2)
        d = np.asarray(src[c])[:ph, :pw].astype(np.int64) - np.asarray(rec[c])[:ph, :pw].astype(np.int64)
        out[c] = int((d * d).sum())
    return out


def ssim8_windows(src_y, rec_y, w: int, h: int, dtype=np.float64) -> np.ndarray:
    """SSIM of every non-overlapping 8x8 luma window of the display window, [h/8, w/8], evaluated
    in ``dtype`` in the kernel's order of operations (float32: what a device without fused
    operations would give; the tests derive their tolerance from its distance to float64)."""
    nwy, nwx = h // 8, w // 8
    f = np.dtype(dtype).type
    a = np.asarray(src_y)[:nwy * 8, :nwx * 8].astype(np.int64).reshape(nwy, 8, nwx, 8)
    b = np.asarray(rec_y)[:nwy * 8, :nwx * 8].astype(np.int64).reshape(nwy, 8, nwx, 8)
    # the five sums are integers below 2^24: exact in either type
    ma, mb = a.sum(axis=(1, 3)).astype(dtype), b.sum(axis=(1, 3)).astype(dtype)
    va, vb = (a * a).sum(axis=(1, 3)).astype(dtype), (b * b).sum(axis=(1, 3)).astype(dtype)
    cov = (a * b).sum(axis=(1, 3)).astype(dtype)
    ma, mb = ma / f(64), mb / f(64)
    va = va / f(64) - ma * ma
    vb = vb / f(64) - mb * mb
    cov = cov / f(64) - ma * mb
    c1, c2 = f(SSIM_C1), f(SSIM_C2)
    return ((f(2) * ma * mb + c1) * (f(2) * cov + c2)) / ((ma * ma + mb * mb + c1) * (va + vb + c2))


def ssim8(src_y, rec_y, w: int, h: int) -> float:
    """The float64 sum of ssim8_windows (the kernel's accumulator; the mean divides by the
    window count (w / 8) * (h / 8))."""
    return float(ssim8_windows(src_y, rec_y, w, h).sum(dtype=np.float64))


def psnr_h264(sse_per_frame, npx) -> float:
    """The H.264 encoder's definition: the mean over the frames of each frame's PSNR, a frame
    without error counting as 100 dB.  npx: samples of the plane per frame."""
    out = []
    for s in np.asarray(sse_per_frame, dtype=np.float64).ravel():
        out.append(100.0 if s == 0 else 10.0 * np.log10(255.0 ** 2 * float(npx) / s))
    return float(np.mean(out))


def psnr_hevc(sse_total, n, bd: int) -> float:
    """The HEVC encoder's definition: the PSNR of the mean squared error over all n samples of the
    segment (every frame together), 99 dB without error; peak (1 << bd) - 1."""
    if int(sse_total) == 0:
        return 99.0
    peak = float((1 << bd) - 1)
    return float(10.0 * np.log10(peak * peak * float(n) / float(sse_total)))


# ------------------------------------------------------------------ weighted prediction
def wp_stats(y, u, v) -> np.ndarray:
    """y: [N, h, w], u / v: [N, h/2, w/2] of any integer type -> int64 [N, 6]: per picture the
    sum and the sum of squares of Y, U and V."""
    cols = []
    for p in (y, u, v):
        q = np.asarray(p).astype(np.int64).reshape(np.asarray(p).shape[0], -1)
        cols += [q.sum(axis=1), (q * q).sum(axis=1)]
    return np.stack(cols, axis=1)


def wp_src(plane, w: int, o: int, d: int) -> np.ndarray:
    """The search source of a weighted picture, s' = ((s - o) << d) / w rounded to nearest (ties
    up) and clipped to a byte; a weight of 0 divides by 1.  Python's floor division is the
    kernel's rounding for both signs of the numerator."""
    wd = max(int(w), 1)
    b = np.asarray(plane).astype(np.int64)
    return np.clip(((b - int(o)) * (1 << int(d)) + (wd >> 1)) // wd, 0, 255).astype(np.uint8)


def wp_forward(pred, w: int, o: int, d: int) -> np.ndarray:
    """Explicit weighted prediction of one list (H.264 8.4.2.3.2, logWD >= 1), unclipped."""
    p = np.asarray(pred).astype(np.int64)
    return ((p * int(w) + (1 << (int(d) - 1))) >> int(d)) + int(o)


# ------------------------------------------------------------------ adaptive quantisation
def aq_energy(Y16, Cb8, Cr8) -> np.ndarray:
    """x264's ac_energy of 16x16 blocks: Y16 [..., 16, 16], Cb8 / Cr8 [..., 8, 8] of any integer
    type -> int64 [...]: ss - (s * s >> 8) of luma plus ss - (s * s >> 6) of each chroma block."""
    def term(p, shift):
        q = np.asarray(p).astype(np.int64)
        s, ss = q.sum(axis=(-2, -1)), (q * q).sum(axis=(-2, -1))
        return ss - ((s * s) >> shift)
    return term(Y16, 8) + term(Cb8, 6) + term(Cr8, 6)


def aq_adj(e, strength: float, extra=None, bd: int = 8) -> np.ndarray:
    """The unrounded offset of a block, float64: strength * 1.0397 * (log2(max(e, 1)) - 14.427
    - 2 (bd - 8)) plus the optional per-block term; strength 0 leaves that term alone."""
    e = np.maximum(np.asarray(e, dtype=np.int64), 1).astype(np.float64)
    adj = np.zeros(e.shape, dtype=np.float64)
    if strength > 0:
        adj = float(strength) * AQ_SCALE * (np.log2(e) - (AQ_BIAS + 2.0 * (bd - 8)))
    if extra is not None:
        adj = adj + np.asarray(extra, dtype=np.float64)
    return adj


def aq_offset_h264(e, strength: float, extra=None) -> np.ndarray:
    """Per-MB QP offset of the H.264 encoder: round-half-even of aq_adj, clamped to +-24."""
    return np.clip(np.rint(aq_adj(e, strength, extra)), -24, 24).astype(np.int64)


def aq_ctb_mean(e4, bd: int, strength: float, extra4=None) -> np.ndarray:
    """The unrounded QP offset of a CTB: the mean of aq_adj over its four 16x16 blocks (last axis)."""
    return 0.25 * aq_adj(e4, strength, extra4, bd).sum(axis=-1)


def aq_ctb_hevc(e4, bd: int, strength: float, extra4, base_qp) -> np.ndarray:
    """Per-CTB QP of the HEVC encoder: base_qp plus the rounded mean offset of the CTB's four
    blocks clamped to +-12, the sum clamped to 0..51.  The per-block table is this minus base_qp."""
    off = np.clip(np.rint(aq_ctb_mean(e4, bd, strength, extra4)), -12, 12).astype(np.int64)
    return np.clip(np.asarray(base_qp, dtype=np.int64) + off, 0, 51)


def mb_blocks(y, u, v):
    """Coded planes [..., H, W] / [..., H/2, W/2] (H, W multiples of 16) -> their 16x16 luma and
    8x8 chroma blocks in raster order: [..., nmb, 16, 16], [..., nmb, 8, 8] x 2."""
    def cut(p, n):
        p = np.asarray(p)
        lead, (H, W) = p.shape[:-2], p.shape[-2:]
        q = p.reshape(*lead, H // n, n, W // n, n)
        q = np.moveaxis(q, -3, -2)
        return q.reshape(*lead, (H // n) * (W // n), n, n)
    return cut(y, 16), cut(u, 8), cut(v, 8)
