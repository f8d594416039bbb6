"""Plain numpy models of the kernels whose results never reach a decoder: the quality metrics
(csrc/kernels/metrics.hip and their host finish), the weighted-prediction statistics and the
inverse-weighted search source (weightp.hip), H.264 variance AQ (aq.hip), the HEVC per-CTB
AQ, the HEVC SAO statistics, decision and filter (8.7.3) and the HEVC source preparation
(hevc_filters.hip).  A wrong result of any of them still gives a valid stream, so the bit-exact
decoder comparison cannot see it: the decoder repeats what the records say, not how they were
chosen.

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


# ------------------------------------------------------------------ HEVC sample adaptive offset
# Edge classes (8.7.3, table 8-13): the two neighbours (dx, dy) of a sample.
SAO_EO_NEIGHBOURS = (((-1, 0), (1, 0)), ((0, -1), (0, 1)), ((-1, -1), (1, 1)), ((1, -1), (-1, 1)))
SAO_NEAR_TIE = 1e-9


def sao_edge_category(plane, k: int) -> np.ndarray:
    """The edge category (8.7.3: 1 valley, 2 / 3 corners, 4 peak; 0 none) of every sample of a
    picture plane for edge class k.  A sample with a neighbour outside the picture has none."""
    d = np.asarray(plane).astype(np.int64)
    h, w = d.shape
    p = np.pad(d, 1, mode="edge")
    yy, xx = np.mgrid[0:h, 0:w]
    idx = np.full((h, w), 2, dtype=np.int64)
    ok = np.ones((h, w), dtype=bool)
    for dx, dy in SAO_EO_NEIGHBOURS[k]:
        idx += np.sign(d - p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w])
        ok &= (xx + dx >= 0) & (xx + dx < w) & (yy + dy >= 0) & (yy + dy < h)
    cat = np.array([1, 2, 0, 3, 4], dtype=np.int64)[idx]
    return np.where(ok, cat, 0)


def sao_stats(deb, src, bd: int, x0: int, y0: int, size: int) -> dict:
    """The SAO statistics of the block whose luma samples are [x0, x0 + size) x [y0, y0 + size)
    (chroma: half of each), over the part inside the picture.  deb, src: (y, u, v) planes of the
    deblocked and the source picture.  -> int64 arrays indexed by component first: ``eo_cnt`` /
    ``eo_sum`` [3, 4 classes, 4 categories] (count, and sum of source - deblocked, of the samples
    of category 1..4) and ``bo_cnt`` / ``bo_sum`` [3, 32 bands].  The neighbours of a sample are
    those of the picture, whichever block they lie in."""
    out = dict(eo_cnt=np.zeros((3, 4, 4), np.int64), eo_sum=np.zeros((3, 4, 4), np.int64),
               bo_cnt=np.zeros((3, 32), np.int64), bo_sum=np.zeros((3, 32), np.int64))
    for c in range(3):
        d = np.asarray(deb[c]).astype(np.int64)
        s = np.asarray(src[c]).astype(np.int64)
        sub = 1 if c else 0
        ys = slice(y0 >> sub, min((y0 + size) >> sub, d.shape[0]))
        xs = slice(x0 >> sub, min((x0 + size) >> sub, d.shape[1]))
        diff = (s - d)[ys, xs]
        band = d[ys, xs] >> (bd - 5)
        out["bo_cnt"][c] = np.bincount(band.ravel(), minlength=32)
        out["bo_sum"][c] = np.bincount(band.ravel(), weights=diff.ravel(), minlength=32).astype(np.int64)
        # the block with one more sample on every side that the picture has: the categories inside
        # the block are those of the whole picture
        ya, xa = max(ys.start - 1, 0), max(xs.start - 1, 0)
        around = d[ya:ys.stop + 1, xa:xs.stop + 1]
        for k in range(4):
            cat = sao_edge_category(around, k)[ys.start - ya:ys.stop - ya, xs.start - xa:xs.stop - xa]
            for e in range(4):
                hit = cat == e + 1
                out["eo_cnt"][c, k, e] = int(hit.sum())
                out["eo_sum"][c, k, e] = int(diff[hit].sum())
    return out


def sao_lambda(qp: int, bd: int) -> float:
    return 0.57 * 2.0 ** ((int(qp) - 12) / 3.0) * 4.0 ** (bd - 8)


def sao_offset_max(bd: int) -> int:
    return (1 << (min(bd, 10) - 5)) - 1


def _sao_dd(n: int, s: int, o: int) -> int:
    """Change of the squared error when o is added to n samples whose source - picture sum is s."""
    return int(n) * o * o - 2 * o * int(s)


def _round_div(s: int, n: int) -> int:
    """s / n to the nearest integer, halves away from zero; 0 for n = 0."""
    if n == 0:
        return 0
    q = (abs(int(s)) + int(n) // 2) // int(n)
    return -q if s < 0 else q


def _sao_group(group: int):
    return (0,) if group == 0 else (1, 2)


def sao_cost(stats: dict, lam: float, params: dict, group: int = 0) -> float:
    """The price distortion change + lambda * bits of a parameter set of one group (0 luma, 1 Cb
    and Cr together).  params: ``type`` [2] (0 off / 1 band / 2 edge) and ``cls`` [2] by group, ``band`` [3]
    and ``off`` [3][4] by component, as sao_decide returns them.  Bits: 1 for off; 3 plus |o| + 1 per offset for
    edge; 1 plus, per component, 5 and |o| + 1 per non-zero offset, 1 per zero offset, for band."""
    t = int(params["type"][group])
    if t == 0:
        return lam * 1.0
    if t == 2:
        k = int(params["cls"][group])
        cost = lam * 3
        for c in _sao_group(group):
            for e in range(4):
                o = int(params["off"][c][e])
                cost += float(_sao_dd(stats["eo_cnt"][c, k, e], stats["eo_sum"][c, k, e], o)) + lam * (abs(o) + 1)
        return cost
    cost = lam * 1
    for c in _sao_group(group):
        cost += _sao_window_cost(stats, lam, c, int(params["band"][c]), params["off"][c])
    return cost


def _sao_window_cost(stats: dict, lam: float, c: int, pos: int, off4) -> float:
    """The price of component c's four band offsets at window position pos (bands wrap 31 -> 0)."""
    w = lam * 5
    for i in range(4):
        b = (pos + i) & 31
        o = int(off4[i])
        w += (float(_sao_dd(stats["bo_cnt"][c, b], stats["bo_sum"][c, b], o)) + lam * (abs(o) + 1)) if o else lam
    return w


def _close(a: float, b: float) -> bool:
    """Within SAO_NEAR_TIE of each other without being equal."""
    return a != b and abs(a - b) <= SAO_NEAR_TIE * max(abs(a), abs(b))


def sao_effect(stats: dict, group: int, t: int, k: int, band, off) -> tuple:
    """What a parameter set does to the block: the offset of every category / band that holds
    samples.  Two sets with the same effect give the same picture."""
    if t == 0:
        return ()
    comps = _sao_group(group)
    if t == 2:
        eff = tuple(int(off[c][e]) if stats["eo_cnt"][c, k, e] else 0 for c in comps for e in range(4))
        return () if not any(eff) else (2, k) + eff
    eff = sum((_sao_band_map(stats, c, int(band[c]), off[c]) for c in comps), ())
    return () if not any(eff) else (1,) + eff


def _sao_band_map(stats: dict, c: int, pos: int, off4) -> tuple:
    """The offset a band window gives each of the 32 bands of component c (0 where it holds no sample)."""
    m = [0] * 32
    for i in range(4):
        b = (pos + i) & 31
        m[b] = int(off4[i]) if stats["bo_cnt"][c, b] else 0
    return tuple(m)


def sao_decide(stats: dict, qp: int, bd: int, lam: float | None = None) -> dict:
    """The encoder's SAO decision of one block from its statistics -> ``type`` [2] (luma, chroma
    pair), ``cls`` [2], ``band`` [3], ``off`` [3][4], ``cost`` [2] and ``near_tie`` [2].

    Edge offsets: per category the mean source - picture difference rounded to nearest, limited to
    0 .. max (categories 1, 2) or -max .. 0 (3, 4), then moved one step towards zero while the
    smaller offset costs no more (distortion change + lambda * |o|).  Band offsets: the rounded
    mean limited to +-max, dropped when distortion change + lambda * (|o| + 1) exceeds lambda.
    The candidates of a group are priced as in sao_cost and scanned in the order off, edge class
    0 .. 3, band (each component at its first cheapest window position); a later candidate wins
    only when it is cheaper.

    ``near_tie``: float64 on another machine may settle this group differently -- a candidate
    (or window position) with a different effect on the picture prices within SAO_NEAR_TIE
    (relative) of the chosen one without being equal to it, or a shrinking / dropping comparison
    on the way to the chosen candidate lies that close.  ``lam`` replaces the QP's lambda (the pins
    use it for prices that tie exactly)."""
    lam = sao_lambda(qp, bd) if lam is None else float(lam)
    cmax = sao_offset_max(bd)
    res = dict(type=[0, 0], cls=[0, 0], band=[0, 0, 0], off=[[0] * 4 for _ in range(3)], cost=[0.0, 0.0],
               near_tie=[False, False], lam=lam)
    for g in (0, 1):
        comps = _sao_group(g)
        cands = [dict(type=[0, 0], cls=[0, 0], band=[0, 0, 0], off=[[0] * 4 for _ in range(3)], close=False)]
        for k in range(4):
            cand = dict(type=[2, 2], cls=[k, k], band=[0, 0, 0], off=[[0] * 4 for _ in range(3)], close=False)
            for c in comps:
                for e in range(4):
                    n, s = int(stats["eo_cnt"][c, k, e]), int(stats["eo_sum"][c, k, e])
                    v = _round_div(s, n)
                    v = min(max(v, 0), cmax) if e < 2 else min(max(v, -cmax), 0)
                    while v != 0:
                        v2 = v - 1 if v > 0 else v + 1
                        d0 = float(_sao_dd(n, s, v)) + lam * abs(v)
                        d1 = float(_sao_dd(n, s, v2)) + lam * abs(v2)
                        cand["close"] |= _close(d0, d1)
                        if d1 <= d0:
                            v = v2
                        else:
                            break
                    cand["off"][c][e] = v
            cands.append(cand)
        band = dict(type=[1, 1], cls=[0, 0], band=[0, 0, 0], off=[[0] * 4 for _ in range(3)], close=False)
        for c in comps:
            ws, offs, closes = [], [], []
            for p in range(32):
                o4, cl = [], False
                for i in range(4):
                    b = (p + i) & 31
                    n, s = int(stats["bo_cnt"][c, b]), int(stats["bo_sum"][c, b])
                    v = min(max(_round_div(s, n), -cmax), cmax)
                    dv = float(_sao_dd(n, s, v)) + lam * (abs(v) + (v != 0))
                    cl |= _close(dv, lam)
                    if dv > lam:
                        v = 0
                    o4.append(v)
                ws.append(_sao_window_cost(stats, lam, c, p, o4))
                offs.append(o4)
                closes.append(cl)
            best = int(np.argmin(ws))          # the first minimum
            band["band"][c] = best
            band["off"][c] = offs[best]
            band["close"] |= closes[best]
            for p in range(32):
                if _close(ws[p], ws[best]):
                    band["close"] |= _sao_band_map(stats, c, p, offs[p]) != _sao_band_map(stats, c, best, offs[best])
        cands.append(band)
        costs = [sao_cost(stats, lam, cd, g) for cd in cands]
        pick = 0
        for i in range(1, len(cands)):
            if costs[i] < costs[pick]:
                pick = i
        ch = cands[pick]
        eff = sao_effect(stats, g, ch["type"][g], ch["cls"][g], ch["band"], ch["off"])
        near = ch["close"]
        for i, cd in enumerate(cands):
            if i != pick and _close(costs[i], costs[pick]):
                near |= sao_effect(stats, g, cd["type"][g], cd["cls"][g], cd["band"], cd["off"]) != eff
        res["type"][g], res["cls"][g] = ch["type"][g], ch["cls"][g]
        for c in comps:
            res["band"][c] = ch["band"][c]
            res["off"][c] = list(ch["off"][c])
        res["cost"][g] = costs[pick]
        res["near_tie"][g] = bool(near)
    return res


def sao_sse_delta(stats: dict, params: dict, c: int) -> int:
    """The change of component c's squared error against the source that the parameters cause, from
    the statistics alone (exact while no sample is clipped)."""
    t = int(params["type"][1 if c else 0])
    if t == 2:
        k = int(params["cls"][1 if c else 0])
        return sum(_sao_dd(stats["eo_cnt"][c, k, e], stats["eo_sum"][c, k, e], int(params["off"][c][e])) for e in range(4))
    if t == 1:
        return sum(_sao_dd(stats["bo_cnt"][c, b], stats["bo_sum"][c, b], int(params["off"][c][i]))
                   for i in range(4) for b in [(int(params["band"][c]) + i) & 31])
    return 0


def sao_apply(deb, params_per_block: dict, bd: int, clip: bool = True):
    """8.7.3 on a whole picture.  deb: (y, u, v) deblocked planes; params_per_block: ``type`` and
    ``cls`` [rows, cols, 2], ``band`` [rows, cols, 3], ``off`` [rows, cols, 3, 4] per 32x32 luma
    (16x16 chroma) block.  Band: a sample of band position + i, i in 0 .. 3 (wrapping 31 -> 0),
    gets off[i]; edge: a sample of category e gets off[e - 1]; clipped to 0 .. 2^bd - 1 (clip=False:
    the sums before clipping).  -> three int64 planes."""
    out = []
    for c in range(3):
        d = np.asarray(deb[c]).astype(np.int64)
        h, w = d.shape
        n = 16 if c else 32

        def per_sample(a):
            return np.repeat(np.repeat(np.asarray(a).astype(np.int64), n, axis=0), n, axis=1)[:h, :w]

        typ = per_sample(np.asarray(params_per_block["type"])[:, :, 1 if c else 0])
        cls = per_sample(np.asarray(params_per_block["cls"])[:, :, 1 if c else 0])
        pos = per_sample(np.asarray(params_per_block["band"])[:, :, c])
        off = [per_sample(np.asarray(params_per_block["off"])[:, :, c, i]) for i in range(4)]
        add = np.zeros_like(d)
        bi = ((d >> (bd - 5)) - pos) & 31
        for i in range(4):
            add = np.where((typ == 1) & (bi == i), off[i], add)
        for k in range(4):
            cat = sao_edge_category(d, k)
            for e in range(4):
                add = np.where((typ == 2) & (cls == k) & (cat == e + 1), off[e], add)
        out.append(np.clip(d + add, 0, (1 << bd) - 1) if clip else d + add)
    return out


# ------------------------------------------------------------------ HEVC source preparation
def hevc_prep(planes, w: int, h: int, W: int, H: int, shift: int, bd: int):
    """The encoder's source of one picture: the w x h display window of the (y, u, v) input planes
    (chroma w/2 x h/2) shifted up by ``shift`` bits and padded to the coded W x H by repeating the
    last column and row -> (y, u, v, proxy), proxy = y >> (bd - 8), the search's 8-bit luma."""
    out = []
    for c, p in enumerate(planes):
        ph, pw, PH, PW = (h, w, H, W) if c == 0 else (h // 2, w // 2, H // 2, W // 2)
        q = np.asarray(p)[:ph, :pw].astype(np.int64) << shift
        out.append(np.pad(q, ((0, PH - ph), (0, PW - pw)), mode="edge"))
    return out[0], out[1], out[2], out[0] >> (bd - 8)


def proxy8(plane, shift: int) -> np.ndarray:
    """The 8-bit proxy of a reconstructed plane: the low eight bits of sample >> shift."""
    return (np.asarray(plane).astype(np.int64) >> shift) & 255
