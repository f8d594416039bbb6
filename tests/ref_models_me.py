"""numpy statement of the 16x16 motion search (csrc/kernels/me_search.h), array form.

The same search as ``_me_ref`` of tests/test_gpu_me_golden.py (tests/test_ref_models_me.py holds
the two against each other), restated on whole blocks so that a 99-MB picture takes a second, and
extended by what that model leaves out: the seed candidate (``seed_mv``), vector costs against
another predictor (``cost_mv``), a lambda per MB (``aq``), early termination (``early_sad``), no
intra estimate, the gate, and slots a routed launch skips (the caller's business: a skipped slot
is simply not modelled).  Per slot; every quantity is an exact integer.
"""
import numpy as np

PAD = 192  # edge extension: vectors clamp to +-128 samples, plus the window and the 6-tap margins
KNO = 0x3FFFFFFF

_H4 = np.array([[1, 1, 1, 1], [1, 1, -1, -1], [1, -1, -1, 1], [1, -1, 1, -1]], dtype=np.int64)

# quarter phase (xf, yf) -> two (plane, dx, dy) taps; planes 0 G, 1 b (half x), 2 h (half y), 3 j
_TAPS = {
    (0, 0): ((0, 0, 0), (0, 0, 0)), (1, 0): ((0, 0, 0), (1, 0, 0)), (2, 0): ((1, 0, 0), (1, 0, 0)),
    (3, 0): ((0, 1, 0), (1, 0, 0)), (0, 1): ((0, 0, 0), (2, 0, 0)), (1, 1): ((1, 0, 0), (2, 0, 0)),
    (2, 1): ((3, 0, 0), (1, 0, 0)), (3, 1): ((1, 0, 0), (2, 1, 0)), (0, 2): ((2, 0, 0), (2, 0, 0)),
    (1, 2): ((3, 0, 0), (2, 0, 0)), (2, 2): ((3, 0, 0), (3, 0, 0)), (3, 2): ((3, 0, 0), (2, 1, 0)),
    (0, 3): ((0, 0, 1), (2, 0, 0)), (1, 3): ((1, 0, 1), (2, 0, 0)), (2, 3): ((3, 0, 0), (1, 0, 1)),
    (3, 3): ((1, 0, 1), (2, 1, 0)),
}


def se_bits(v):
    u = -2 * v if v <= 0 else 2 * v - 1
    return 2 * (int(u + 1).bit_length() - 1) + 1


def ring(c, step):
    idx = 4 if c == 0 else (c - 1 if c <= 4 else c)
    return (idx % 3 - 1) * step, (idx // 3 - 1) * step


def hsum_mb(t):
    """sum over the 16 4x4 blocks of a 16x16 residual of |H4 T H4^T|"""
    b = t.reshape(4, 4, 4, 4).transpose(0, 2, 1, 3)  # [block row, block col, y, x]
    return int(np.abs(_H4 @ b @ _H4.T).sum())


class Planes:
    """Edge-extended reference and its half-sample planes (clause 8.4.2.2.1)."""

    def __init__(self, ref):
        g = np.pad(ref.astype(np.int64), PAD, mode="edge")

        def tap(a, axis):
            sl = lambda o: np.roll(a, -o, axis=axis)  # noqa: E731
            return sl(-2) - 5 * sl(-1) + 20 * sl(0) + 20 * sl(1) - 5 * sl(2) + sl(3)
        b1, h1 = tap(g, 1), tap(g, 0)
        self.p = (g, np.clip((b1 + 16) >> 5, 0, 255), np.clip((h1 + 16) >> 5, 0, 255),
                  np.clip((tap(b1, 0) + 512) >> 10, 0, 255))

    def int_block(self, x, y):
        return self.p[0][PAD + y:PAD + y + 16, PAD + x:PAD + x + 16]

    def block(self, x0, y0, mvx, mvy):
        x, y = x0 + (mvx >> 2) + PAD, y0 + (mvy >> 2) + PAD
        (pa, ax, ay), (pb, bx, by) = _TAPS[(mvx & 3, mvy & 3)]
        a = self.p[pa][y + ay:y + ay + 16, x + ax:x + ax + 16]
        b = self.p[pb][y + by:y + by + 16, x + bx:x + bx + 16]
        return (a + b + 1) >> 1


def intra16_estimate(s, mx, my):
    """open-loop Intra16x16 SATD estimate of MB (mx, my) on source neighbours, without lambda"""
    X0, Y0 = mx * 16, my * 16
    S = s[Y0:Y0 + 16, X0:X0 + 16]
    top = s[Y0 - 1, X0:X0 + 16] if my > 0 else np.zeros(16, dtype=np.int64)
    left = s[Y0:Y0 + 16, X0 - 1] if mx > 0 else np.zeros(16, dtype=np.int64)
    tl = int(s[Y0 - 1, X0 - 1]) if mx > 0 and my > 0 else 0
    modes = []
    if my > 0:
        modes.append(np.tile(top, (16, 1)))
    if mx > 0:
        modes.append(np.tile(left[:, None], (1, 16)))
    st, sl = int(top.sum()), int(left.sum())
    dc = (st + sl + 16) >> 5 if (mx > 0 and my > 0) else ((sl + 8) >> 4 if mx > 0 else ((st + 8) >> 4 if my > 0 else 128))
    modes.append(np.full((16, 16), dc, dtype=np.int64))
    if mx > 0 and my > 0:
        hh = sum((i + 1) * (int(top[8 + i]) - (tl if i == 7 else int(top[6 - i]))) for i in range(8))
        vv = sum((i + 1) * (int(left[8 + i]) - (tl if i == 7 else int(left[6 - i]))) for i in range(8))
        a, b, c = 16 * (int(left[15]) + int(top[15])), (5 * hh + 32) >> 6, (5 * vv + 32) >> 6
        yy, xx = np.mgrid[0:16, 0:16]
        modes.append(np.clip((a + b * (xx - 7) + c * (yy - 7) + 16) >> 5, 0, 255))
    return min((hsum_mb(S - m) + 1) >> 1 for m in modes)


def me_search(src, ref, pred_mv, qp, R, lam_tab, wmb, hmb, seed_mv=None, cost_mv=None, aq=None, early_sad=0,
              with_intra=True, gate_cost=None, gate_thresh=0):
    """One slot.  -> dict(mv [nmb, 2], cost [nmb], pred [nmb, 256], intra [nmb] or None, searched
    [nmb] bool, early [nmb] bool, centre [nmb, 2], window [nmb, 2] (its left and top sample), zero_outside [nmb]
    bool, best_sad [nmb]: the SAD of the chosen centre).  An MB the gate stops has cost KNO (intra KNO when with_intra) and searched False; the caller
    leaves its other outputs alone."""
    nmb = wmb * hmb
    pl = Planes(ref)
    s = src.astype(np.int64)
    out = dict(mv=np.zeros((nmb, 2), dtype=np.int64), cost=np.zeros(nmb, dtype=np.int64),
               pred=np.zeros((nmb, 256), dtype=np.int64), intra=np.zeros(nmb, dtype=np.int64) if with_intra else None,
               searched=np.ones(nmb, dtype=bool), early=np.zeros(nmb, dtype=bool), centre=np.zeros((nmb, 2), dtype=np.int64),
               window=np.zeros((nmb, 2), dtype=np.int64), zero_outside=np.zeros(nmb, dtype=bool),
               best_sad=np.zeros(nmb, dtype=np.int64))
    side = 2 * R + 1
    for mb in range(nmb):
        mx, my = mb % wmb, mb // wmb
        X0, Y0 = mx * 16, my * 16
        lam = int(lam_tab[int(np.clip(qp + (0 if aq is None else int(aq[mb])), 0, 51))])
        if gate_cost is not None:
            thr = gate_thresh if gate_thresh >= 0 else -gate_thresh * lam
            if int(gate_cost[mb]) <= thr:
                out["cost"][mb] = KNO
                if with_intra:
                    out["intra"][mb] = KNO
                out["searched"][mb] = False
                continue
        S = s[Y0:Y0 + 16, X0:X0 + 16]
        q = lambda v: ((int(v[0]) + 2) >> 2, (int(v[1]) + 2) >> 2)  # noqa: E731
        pmx = pmy = 0
        cands = [(0, 0)] * 5
        if pred_mv is not None:
            pmx, pmy = int(pred_mv[mb, 0]), int(pred_mv[mb, 1])
            cands = [q(pred_mv[mb]), q(pred_mv[mb - 1]) if mx > 0 else (0, 0), q(pred_mv[mb - wmb]) if my > 0 else (0, 0),
                     q(pred_mv[mb + 1]) if mx < wmb - 1 else (0, 0), (0, 0)]
            if cost_mv is not None:
                pmx, pmy = int(cost_mv[mb, 0]), int(cost_mv[mb, 1])
        if seed_mv is not None:
            cands.append(q(seed_mv[mb]))

        def vcost(mvx, mvy):
            return lam * (se_bits(mvx - pmx) + se_bits(mvy - pmy))

        def sad(dx, dy):
            return int(np.abs(S - pl.int_block(X0 + dx, Y0 + dy)).sum())
        best = None
        for dx, dy in cands:
            dx, dy = max(-128, min(128, dx)), max(-128, min(128, dy))
            sd = sad(dx, dy)
            c = sd + vcost(dx * 4, dy * 4)
            if best is None or c < best:
                best, cx, cy, best_sad = c, dx, dy, sd
        out["best_sad"][mb] = best_sad
        out["centre"][mb] = (cx, cy)
        out["window"][mb] = (X0 + cx - R - 4, Y0 + cy - R - 4)
        bx, by = cx, cy
        if early_sad > 0 and best_sad <= early_sad:
            out["early"][mb] = True
        else:
            # all (2R+1)^2 SADs at once: windows of the region around the centre
            reg = pl.p[0][PAD + Y0 + cy - R:PAD + Y0 + cy + R + 16, PAD + X0 + cx - R:PAD + X0 + cx + R + 16]
            win = np.lib.stride_tricks.sliding_window_view(reg, (16, 16))
            sads = np.abs(win - S).sum(axis=(2, 3))
            bkey = None
            for dy in range(side):
                cyb = lam * se_bits((cy + dy - R) * 4 - pmy)
                for dx in range(side):
                    c = int(sads[dy, dx]) + lam * se_bits((cx + dx - R) * 4 - pmx) + cyb
                    key = (c << 12) | (dy * side + dx)
                    bkey = key if bkey is None or key < bkey else bkey
            if abs(cx) > R or abs(cy) > R:
                out["zero_outside"][mb] = True
                bkey = min(bkey, ((sad(0, 0) + vcost(0, 0)) << 12) | 4095)
            bp = bkey & 4095
            bx, by = (0, 0) if bp == 4095 else (cx + bp % side - R, cy + bp // side - R)

        def cost_q(mvx, mvy):
            return ((hsum_mb(S - pl.block(X0, Y0, mvx, mvy)) + 1) >> 1) + vcost(mvx, mvy)
        bm = (bx * 4, by * 4)
        hk = min(((cost_q(bm[0] + ring(c, 2)[0], bm[1] + ring(c, 2)[1]) << 4) | c) for c in range(9))
        hx, hy = ring(hk & 15, 2)
        qk = hk & ~15
        for c in range(1, 9):
            ox, oy = ring(c, 1)
            qk = min(qk, (cost_q(bm[0] + hx + ox, bm[1] + hy + oy) << 4) | c)
        qx, qy = ring(qk & 15, 1)
        mv = (bm[0] + hx + qx, bm[1] + hy + qy)
        out["mv"][mb] = mv
        out["cost"][mb] = qk >> 4
        out["pred"][mb] = pl.block(X0, Y0, mv[0], mv[1]).reshape(-1)
        if with_intra:
            out["intra"][mb] = intra16_estimate(s, mx, my) + lam * 4
    return out
