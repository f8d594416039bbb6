"""numpy model of the H.264 in-loop filter as csrc/kernels/deblock.hip runs it: the boundary
strengths and info words of the pre-pass (deblock_bs), and clause 8.7 on a 4:2:0 picture in
macroblock raster order.  Written from the standard's text and tables, one line of samples at a
time: nothing here shares code with the kernels or the C++ decoder.

Records are MbHeader bytes (csrc/common/h264_mb.h), [nmb, 64] uint8; non-zero flags [nmb, 16]
uint8 in 4x4 raster order.  Strengths come in the parser's layout ([nmb, 16] uint8: segment
i = dir * 16 + edge * 4 + k, 4 bits each in byte i / 2, low nibble for even i) or unpacked as
[nmb, 2, 4, 4] (dir 0: vertical edges; edge; 4-sample segment along the edge).
"""
import numpy as np

MB_HDR_BYTES = 64
_KIND, _QP, _FLAGS, _REF, _MV = 0, 2, 5, 8, 16
MBK_I4x4, MBK_I16x16, MBK_P16x16, MBK_IPCM, MBK_I8x8, MBK_B16x16 = 0, 1, 2, 4, 8, 9
INTRA_KINDS = (MBK_I4x4, MBK_I16x16, MBK_IPCM, MBK_I8x8)
MBF_T8x8 = 2
INFO_ON_SHIFT = 8

# Tables 8-16 (alpha', beta' by indexA / indexB), 8-17 (tC0' by indexA and bS 1..3), 8-15 (QPc by qPI)
ALPHA = np.array([0] * 16 + [4, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15, 17, 20, 22, 25, 28, 32, 36, 40, 45, 50, 56, 63, 71,
                             80, 90, 101, 113, 127, 144, 162, 182, 203, 226, 255, 255])
BETA = np.array([0] * 16 + [2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14,
                            14, 15, 15, 16, 16, 17, 17, 18, 18])
TC0 = np.array([[0, 0, 0]] * 17 + [[0, 0, 1]] * 4 + [[0, 1, 1]] * 2 + [[1, 1, 1]] * 4 + [[1, 1, 2]] * 4 +
               [[1, 2, 3], [1, 2, 3], [2, 2, 3], [2, 2, 4], [2, 3, 4], [2, 3, 4], [3, 3, 5], [3, 4, 6], [3, 4, 6],
                [4, 5, 7], [4, 5, 8], [4, 6, 9], [5, 7, 10], [6, 8, 11], [6, 8, 13], [7, 10, 14], [8, 11, 16],
                [9, 12, 18], [10, 13, 20], [11, 15, 23], [13, 17, 25]])
CHROMA_QP = np.array(list(range(30)) + [29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39,
                                        39, 39, 39])
assert ALPHA.size == 52 and BETA.size == 52 and TC0.shape == (52, 3) and CHROMA_QP.size == 52

# lines the model filtered since the last clear(): "off" (bS > 0 but over a threshold), "weak" (bS < 4),
# "strong" (bS 4 with the long filter on a side), "plain4" (bS 4 without)
LINE_STATS = {"off": 0, "weak": 0, "strong": 0, "plain4": 0}


# ---------------------------------------------------------------- records
def make_hdr(nmb):
    """Zeroed records: P16x16 from list 0 ref 0 with a zero vector, list 1 unused."""
    h = np.zeros((nmb, MB_HDR_BYTES), np.uint8)
    h[:, _KIND] = MBK_P16x16
    h[:, _REF + 4:_REF + 8] = 0xFF
    return h


def hdr_kind(h):
    return h[:, _KIND].astype(np.int32)


def hdr_qp(h):
    return h[:, _QP].view(np.int8).astype(np.int32)


def hdr_t8(h):
    return (h[:, _FLAGS] & MBF_T8x8) != 0


def hdr_ref(h):
    """[nmb, 2, 4] ref_idx per list and 8x8 quadrant, -1: list unused"""
    return h[:, _REF:_REF + 8].view(np.int8).reshape(-1, 2, 4).astype(np.int32)


def hdr_mv(h):
    """[nmb, 2, 4, 2] quarter-sample vectors per list and quadrant"""
    return np.ascontiguousarray(h[:, _MV:_MV + 32]).view(np.int16).reshape(-1, 2, 4, 2).astype(np.int32)


def nz_from_mask(h, mask):
    """The decoder's non-zero flags from the parser's block masks (bits 0..15: luma4x4BlkIdx with
    a level; an 8x8-transform block marks its four 4x4 blocks)."""
    nmb = h.shape[0]
    nz = np.zeros((nmb, 16), np.uint8)
    t8 = hdr_t8(h)
    for m in range(nmb):
        for blk in range(16):
            bits = (int(mask[m]) >> (blk & ~3)) & 15 if t8[m] else (int(mask[m]) >> blk) & 1
            x = (blk & 1) | ((blk >> 1) & 2)
            y = ((blk >> 1) & 1) | ((blk >> 2) & 2)
            nz[m, y * 4 + x] = 1 if bits else 0
    return nz


# ---------------------------------------------------------------- boundary strengths
def _quadrant(r):
    return ((r >> 3) & 1) * 2 + ((r & 3) >> 1)


def boundary_strengths(h, nz, wmb, hmb):
    """[nmb, 2, 4, 4] bS (8.7.2.1) with the reference identity the encoder's records allow:
    (list, ref_idx).  MB edges on the picture border and the odd inner edges of 8x8-transform MBs
    are 0."""
    nmb = wmb * hmb
    kind, t8, ref, mv = hdr_kind(h), hdr_t8(h), hdr_ref(h), hdr_mv(h)
    intra = np.isin(kind, INTRA_KINDS)
    bs = np.zeros((nmb, 2, 4, 4), np.int32)
    for q in range(nmb):
        x, y = q % wmb, q // wmb
        for d in range(2):
            for e in range(4):
                if e == 0 and (x == 0 if d == 0 else y == 0):
                    continue
                if (e & 1) and t8[q]:
                    continue
                p = q if e else (q - 1 if d == 0 else q - wmb)
                for k in range(4):
                    rq = e + 4 * k if d == 0 else k + 4 * e
                    if e == 0:
                        rp = 3 + 4 * k if d == 0 else k + 12
                    else:
                        rp = e - 1 + 4 * k if d == 0 else k + 4 * (e - 1)
                    if intra[p] or intra[q]:
                        v = 4 if e == 0 else 3
                    elif nz[p, rp] or nz[q, rq]:
                        v = 2
                    else:
                        qp_, qq_ = _quadrant(rp), _quadrant(rq)
                        v = 0
                        for l in range(2):
                            fp, fq = ref[p, l, qp_], ref[q, l, qq_]
                            if (fp >= 0) != (fq >= 0) or (fp >= 0 and fp != fq):
                                v = 1
                            elif fp >= 0 and (np.abs(mv[p, l, qp_] - mv[q, l, qq_]) >= 4).any():
                                v = 1
                    bs[q, d, e, k] = v
    return bs


def pack_bs(bs):
    """[nmb, 2, 4, 4] -> the parser's [nmb, 16] nibble layout"""
    f = bs.reshape(bs.shape[0], 32).astype(np.uint8)
    return (f[:, 0::2] | (f[:, 1::2] << 4)).astype(np.uint8)


def unpack_bs(b):
    b = np.asarray(b, np.uint8)
    f = np.empty((b.shape[0], 32), np.int32)
    f[:, 0::2] = b & 15
    f[:, 1::2] = b >> 4
    return f.reshape(-1, 2, 4, 4)


def info_words(bs, qp):
    """One word per MB: bits 0..7 the QP, bit 8 + dir * 4 + edge: some segment of the edge is on."""
    on = (bs.reshape(bs.shape[0], 8, 4) != 0).any(axis=2)
    bits = (on.astype(np.uint32) << np.arange(8, dtype=np.uint32)).sum(axis=1).astype(np.uint32)
    return (np.asarray(qp).astype(np.uint32) & 255) | (bits << INFO_ON_SHIFT)


# ---------------------------------------------------------------- clause 8.7
def _filter_lines(P, Q, bs, ia, ib, chroma):
    """P[n, 4] = p3 p2 p1 p0, Q[n, 4] = q0 q1 q2 q3 (int32), bs[n]; filtered in place (8.7.2.3 and
    8.7.2.4).  Chroma lines: p1 p0 q0 q1 only."""
    alpha, beta = int(ALPHA[ia]), int(BETA[ib])
    for i in range(P.shape[0]):
        b = int(bs[i])
        if b == 0:
            continue
        p3, p2, p1, p0 = (int(v) for v in P[i])
        q0, q1, q2, q3 = (int(v) for v in Q[i])
        if not (abs(p0 - q0) < alpha and abs(p1 - p0) < beta and abs(q1 - q0) < beta):
            LINE_STATS["off"] += 1
            continue
        ap, aq = abs(p2 - p0), abs(q2 - q0)
        if b < 4:
            LINE_STATS["weak"] += 1
            tc0 = int(TC0[ia][b - 1])
            tc = tc0 + 1 if chroma else tc0 + (ap < beta) + (aq < beta)
            delta = min(max((((q0 - p0) << 2) + (p1 - q1) + 4) >> 3, -tc), tc)
            P[i, 3] = min(max(p0 + delta, 0), 255)
            Q[i, 0] = min(max(q0 - delta, 0), 255)
            if not chroma:
                if ap < beta:
                    P[i, 2] = p1 + min(max((p2 + ((p0 + q0 + 1) >> 1) - (p1 << 1)) >> 1, -tc0), tc0)
                if aq < beta:
                    Q[i, 1] = q1 + min(max((q2 + ((p0 + q0 + 1) >> 1) - (q1 << 1)) >> 1, -tc0), tc0)
        else:
            small = abs(p0 - q0) < ((alpha >> 2) + 2)
            LINE_STATS["strong" if not chroma and small and (ap < beta or aq < beta) else "plain4"] += 1
            if not chroma and ap < beta and small:
                P[i, 3] = (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3
                P[i, 2] = (p2 + p1 + p0 + q0 + 2) >> 2
                P[i, 1] = (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3
            else:
                P[i, 3] = (2 * p1 + p0 + q1 + 2) >> 2
            if not chroma and aq < beta and small:
                Q[i, 0] = (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3
                Q[i, 1] = (p0 + q0 + q1 + q2 + 2) >> 2
                Q[i, 2] = (2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3
            else:
                Q[i, 0] = (2 * q1 + q0 + p1 + 2) >> 2


def _edge(plane, x0, y0, n, d, bs_lines, ia, ib, chroma):
    """Filter the edge whose q0 samples start at (x0, y0) and run n samples down (d 0, a vertical
    edge) or right (d 1)."""
    if not bs_lines.any():
        return False
    if d == 0:
        blk = plane[y0:y0 + n, x0 - 4:x0 + 4] if not chroma else plane[y0:y0 + n, x0 - 2:x0 + 2]
        v = blk.astype(np.int32)
    else:
        blk = plane[y0 - 4:y0 + 4, x0:x0 + n] if not chroma else plane[y0 - 2:y0 + 2, x0:x0 + n]
        v = blk.astype(np.int32).T
    if chroma:
        v = np.concatenate([np.zeros((n, 2), np.int32), v, np.zeros((n, 2), np.int32)], axis=1)
    P, Q = v[:, :4].copy(), v[:, 4:].copy()
    _filter_lines(P, Q, bs_lines, ia, ib, chroma)
    out = np.concatenate([P, Q], axis=1)
    if chroma:
        out = out[:, 2:6]
    changed = bool((out != (v[:, 2:6] if chroma else v)).any())
    blk[...] = (out if d == 0 else out.T).astype(plane.dtype)
    return changed


def deblock_picture(y, u, v, bs, qp, wmb, hmb, chroma_qp_offset=0, alpha_off=0, beta_off=0):
    """Filter the planes in place (uint8 [H, W], [H / 2, W / 2] x 2) in MB raster order: per MB the
    vertical edges left to right, then the horizontal edges top to bottom, luma and both chroma
    planes (chroma edges 0 and 2 are luma edges 0 and 2 at half size).  bs [nmb, 2, 4, 4], qp [nmb].
    Returns changed[nmb, 2, 4]: did the edge change a sample (of any plane)."""
    nmb = wmb * hmb
    qp = np.asarray(qp).astype(np.int32)
    qpc = CHROMA_QP[np.clip(qp + chroma_qp_offset, 0, 51)]
    changed = np.zeros((nmb, 2, 4), bool)

    def idx(a, b):
        av = (int(a) + int(b) + 1) >> 1
        return min(max(av + alpha_off, 0), 51), min(max(av + beta_off, 0), 51)

    for q in range(nmb):
        mx, my = q % wmb, q // wmb
        for d in range(2):
            for e in range(4):
                b4 = bs[q, d, e]
                if not b4.any():
                    continue
                p = q if e else (q - 1 if d == 0 else q - wmb)
                assert p >= 0 and (e or (mx > 0 if d == 0 else my > 0)), "bS on a picture border"
                ia, ib = idx(qp[p], qp[q])
                x0, y0 = (mx * 16 + 4 * e, my * 16) if d == 0 else (mx * 16, my * 16 + 4 * e)
                ch = _edge(y, x0, y0, 16, d, np.repeat(b4, 4), ia, ib, False)
                if e in (0, 2):
                    ia, ib = idx(qpc[p], qpc[q])
                    cx, cy = (mx * 8 + 2 * e, my * 8) if d == 0 else (mx * 8, my * 8 + 2 * e)
                    for pl in (u, v):
                        ch |= _edge(pl, cx, cy, 8, d, np.repeat(b4, 2), ia, ib, True)
                changed[q, d, e] = ch
    return changed


# ---------------------------------------------------------------- synthetic cases
# Shapes of tests/test_gpu_deblock_bs.py (MB columns x rows) and the rows made fully quiet.
SHAPES = [(1, 1), (1, 3), (5, 3), (11, 9), (21, 2), (3, 35)]


def quiet_rows(hmb):
    return [r for r in range(1, hmb) if r % 7 == 1] if hmb >= 3 else []


def make_case(wmb, hmb, seed, B=2):
    """Records, non-zero flags and planes of B slots.

    Motion comes in patches of equal vectors without levels (quiet MBs; neighbouring patches differ
    by less or by more than 4 quarter samples).  Single MBs then get a differing vector in one
    quadrant, another reference, a second list, a level, an intra kind or the 8x8 transform; rows
    quiet_rows() and the rows above them keep one motion and no level, so the former filter
    nothing.  QPs 18..42 per MB.  Planes: a ramp plus per-4x4-block steps of mixed heights, so that
    lines below and above the alpha / beta thresholds, the bS < 4 filter and the strong one occur.
    """
    rng = np.random.default_rng(seed)
    nmb = wmb * hmb
    H, W = hmb * 16, wmb * 16
    hdrs, nzs, planes = [], [], []
    for _ in range(B):
        h = make_hdr(nmb)
        nz = np.zeros((nmb, 16), np.uint8)
        mv = np.zeros((nmb, 2, 4, 2), np.int16)
        base = rng.integers(-20, 21, 2)
        for py in range(0, hmb, 2):
            for px in range(0, wmb, 3):
                v = base + rng.choice([0, 1, 2, 3, 5, 8], 2) * rng.choice([-1, 1], 2)
                for y in range(py, min(py + 2, hmb)):
                    mv[y * wmb + px:y * wmb + min(px + 3, wmb), 0] = v
        for m in range(nmb):
            r = rng.random()
            if r < 0.08:    # one quadrant moves away: inner and outer edges with bS 1
                mv[m, 0, rng.integers(0, 4)] += rng.choice([-7, 4, 9], 2)
                h[m, _KIND] = 7
            elif r < 0.13:  # another reference picture
                h[m, _REF:_REF + 4] = 1
            elif r < 0.17:  # bi-predicted
                h[m, _KIND] = MBK_B16x16
                h[m, _REF + 4:_REF + 8] = 0
                mv[m, 1] = rng.integers(-8, 9, 2)
            elif r < 0.27:  # levels in a few 4x4 blocks
                nz[m, rng.integers(0, 16, rng.integers(1, 5))] = 1
            elif r < 0.33:  # 8x8 transform: an 8x8 block marks its four 4x4 blocks
                h[m, _FLAGS] |= MBF_T8x8
                for b8 in rng.integers(0, 4, rng.integers(0, 3)):
                    for k in range(4):
                        nz[m, (b8 & 1) * 2 + (k & 1) + 4 * ((b8 >> 1) * 2 + (k >> 1))] = 1
            elif r < 0.39:
                h[m, _KIND] = rng.choice([MBK_I4x4, MBK_I16x16, MBK_I8x8])
                if h[m, _KIND] == MBK_I8x8:
                    h[m, _FLAGS] |= MBF_T8x8
                h[m, _REF:_REF + 8] = 0xFF
                nz[m] = rng.integers(0, 2, 16)
        for r in quiet_rows(hmb):
            for y in (r - 1, r):
                s = slice(y * wmb, (y + 1) * wmb)
                h[s] = make_hdr(wmb)
                nz[s] = 0
                mv[s] = 0
                mv[s, 0] = base
        h[:, _MV:_MV + 32] = mv.reshape(nmb, 16).view(np.uint8).reshape(nmb, 32)
        h[:, _QP] = rng.integers(18, 43, nmb).astype(np.uint8)
        h[:, 48:] = rng.integers(0, 256, (nmb, 16))  # the intra modes: not the filter's business
        hdrs.append(h)
        nzs.append(nz)
        pl = []
        for hh, ww, blk in ((H, W, 4), (H // 2, W // 2, 2), (H // 2, W // 2, 2)):
            yy, xx = np.mgrid[0:hh, 0:ww]
            ramp = 60 + (xx * rng.integers(0, 3) + yy * rng.integers(0, 3)) // 4
            step = rng.choice([0, 0, 1, 2, 3, 5, 8, 13, 30], (hh // blk, ww // blk)) * rng.choice([-1, 1], (hh // blk, ww // blk))
            step = np.kron(step, np.ones((blk, blk), np.int64))
            pl.append(np.clip(ramp + step + rng.integers(-1, 2, (hh, ww)), 0, 255).astype(np.uint8))
        planes.append(pl)
    return dict(B=B, wmb=wmb, hmb=hmb, hdr=np.stack(hdrs), nz=np.stack(nzs),
                y=np.stack([p[0] for p in planes]), u=np.stack([p[1] for p in planes]),
                v=np.stack([p[2] for p in planes]), cqo=int(rng.integers(-3, 4)))


def run_case(c):
    """The model's outputs for a case: bs [B, nmb, 16], info [B, nmb], filtered planes, and what
    the case covers (case_counts)."""
    B, wmb, hmb = c["B"], c["wmb"], c["hmb"]
    out = dict(bs=[], info=[], y=[], u=[], v=[])
    counts = {}
    before = dict(LINE_STATS)
    for b in range(B):
        bs = boundary_strengths(c["hdr"][b], c["nz"][b], wmb, hmb)
        qp = hdr_qp(c["hdr"][b])
        info = info_words(bs, qp)
        y, u, v = c["y"][b].copy(), c["u"][b].copy(), c["v"][b].copy()
        deblock_picture(y, u, v, bs, qp, wmb, hmb, chroma_qp_offset=c["cqo"])
        for k, a in (("bs", pack_bs(bs)), ("info", info), ("y", y), ("u", u), ("v", v)):
            out[k].append(a)
        for k, n in case_counts(bs, info, c["y"][b], y, wmb, hmb).items():
            counts[k] = counts.get(k, 0) + n
    res = {k: np.stack(a) for k, a in out.items()}
    for k, n in LINE_STATS.items():
        counts["lines_" + k] = n - before[k]
    res["counts"] = counts
    return res


def case_counts(bs, info, y0, y1, wmb, hmb):
    """What a picture covers.  Wave steps are those of deblock.hip's layout: a wave filters MB
    (x, r) of an even row r and MB (x - 2, r + 1) in one step."""
    on = ((info >> INFO_ON_SHIFT) & 255).reshape(hmb, wmb)
    quiet = on == 0
    n = {"bs%d" % v: int((bs == v).sum()) for v in range(5)}
    pad = np.zeros((hmb + 2, wmb + 2), bool)
    pad[1:-1, 1:-1] = ~quiet  # filtering neighbours; outside the picture: none
    n["quiet_left_of_busy"] = int((quiet & pad[1:-1, 2:]).sum())
    n["quiet_right_of_busy"] = int((quiet & pad[1:-1, :-2]).sum())
    n["quiet_above_busy"] = int((quiet & pad[2:, 1:-1]).sum())
    n["quiet_below_busy"] = int((quiet & pad[:-2, 1:-1]).sum())
    n["quiet_row"] = int(quiet.all(axis=1).sum())
    for k in ("step_upper_quiet", "step_lower_quiet", "step_vertical_only", "step_horizontal_only", "step_quiet"):
        n[k] = 0
    for r in range(0, hmb, 2):
        for step in range(wmb + 2):
            up = int(on[r, step]) if step < wmb else None
            lo = int(on[r + 1, step - 2]) if r + 1 < hmb and step >= 2 else None
            if up is not None and lo is not None:
                n["step_upper_quiet"] += up == 0 and lo != 0
                n["step_lower_quiet"] += lo == 0 and up != 0
            both = (up or 0) | (lo or 0)
            n["step_vertical_only"] += (both & 15) != 0 and (both >> 4) == 0
            n["step_horizontal_only"] += (both & 15) == 0 and (both >> 4) != 0
            n["step_quiet"] += both == 0
    # quiet MBs whose halo the neighbour's own edges changed: the left MB's columns 12..15 (rows
    # 0..12: rows 13..15 belong to the MB below it) and the top MB's rows 12..15 (columns 0..11:
    # columns 12..15 belong to its right neighbour)
    ch = y0 != y1
    n["quiet_left_halo_changed"] = n["quiet_top_halo_changed"] = 0
    for r in range(hmb):
        for x in range(wmb):
            if not quiet[r, x]:
                continue
            if x > 0 and ch[r * 16:r * 16 + 13, x * 16 - 4:x * 16].any():
                n["quiet_left_halo_changed"] += 1
            if r > 0 and ch[r * 16 - 4:r * 16, x * 16:x * 16 + 12].any():
                n["quiet_top_halo_changed"] += 1
    return {k: int(v) for k, v in n.items()}
