"""numpy statement of ``p_mixed_refs`` (csrc/kernels/h264_p_mixed.hip): the reference selection of
H.264 P macroblocks with a reference per 8x8 quadrant (x264 --mixed-refs).  This is the rule's
definition; the kernel is held to it exactly (tests/test_gpu_h264_mixed_model.py).

Per P macroblock of a slot with ``nr = min(nref, n0)`` active list-0 pictures, lambda ``L`` of
its own QP (slot QP + AQ offset):

(a) the list-0[0] decision as it stands: ``cost + L``.
(b) farther picture k (``xcost[k - 1] < KNO``: it was searched) as one 16x16 partition:
    ``xcost[k - 1] + L * (k + 2)``.  (a) against (b), in this order and strictly, is
    ``me_ref_select``.
(c) a reference per quadrant, priced only for an MB with at least one searched farther picture
    whose list-0[0] SATD -- the sum over its quadrants of the 8x8 SATD of ``src0`` against
    RefPicList0[0] at ``mv8[q]`` -- is above ``min_satd``:

    * reference 0 keeps ``mv8[q]``: that SATD + ``L * (bits(mv8[q] - pm) + 1)``;
    * a searched picture k: candidates ``xmv[k - 1]``, ``scale_k(mv8[q])``, ``scale_k(mv)``, zero
      (each clamped; the first of equal prices stays), then a half- and a quarter-sample ring of
      eight positions (clamped, the first of equal prices, taken when strictly cheaper than the
      centre), priced ``SATD(src, picture k) + L * (bits(v - scale_k(pm)) + k + 2)``;
    * the quadrant takes the cheapest, the nearer picture on a tie; the MB costs the sum +
      ``L * overhead``.

    ``pm`` is the search-time predictor: one vector per MB (the encoder passes what the farther
    searches were priced against, the MB's own final 16x16 list-0[0] vector), so the mvd bits
    are an estimate -- the writer codes against the predictor of clause 8.4.1.3.  ``scale_k(v) = clamp((s * v + 128) >> 8)`` with the slot's
    distance ratio ``s`` of picture k in 1/256 units; vectors live in [-2048, 2047] x [-512, 511].
    (c) counts when at least one quadrant leaves reference 0 (``pm`` is not what ``cost`` priced
    a split on reference 0 against: that choice stays ``p_part8x8``'s), its quadrants do not
    share one (reference, vector), and it is strictly cheaper than the better of (a) and (b).

Outputs: ``mv, mv8, cost, pred, mref`` as ``me_ref_select`` leaves them when (a) or (b) wins, plus
``mref4`` = that reference four times.  When (c) wins: ``mv8`` / ``mref4`` per quadrant, ``mv`` and
``mref`` of quadrant 0, ``cost`` = what the better of (a) and (b) would have left, shifted by the
gain, and the quadrants of ``pred`` on a farther picture rewritten with its plain prediction.
A slot that codes no P picture is not touched.  Every quantity is an exact integer.
"""
import numpy as np

from ref_models_me import _TAPS, PAD, Planes, ring, se_bits

KNO = 0x3FFFFFFF
MVX = (-2048, 2047)
MVY = (-512, 511)

_H4 = np.array([[1, 1, 1, 1], [1, 1, -1, -1], [1, -1, -1, 1], [1, -1, 1, -1]], dtype=np.int64)


def clampi(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def scale_mv(s, v, lo, hi):
    """(s * v + 128) >> 8 (arithmetic shift: floor), clamped"""
    return clampi((int(s) * int(v) + 128) >> 8, lo, hi)


def ref_bits(k):
    """ref_idx bins of the CABAC unary code, about 1 / 3 / 4 / 5 bits"""
    return 1 if k == 0 else k + 2


def satd8(a, b):
    """8x8 SATD: the four 4x4 blocks' sum |H d H^T| / 2 (x264's normalisation)"""
    d = (a.astype(np.int64) - b.astype(np.int64)).reshape(2, 4, 2, 4).transpose(0, 2, 1, 3)
    return int((np.abs(_H4 @ d @ _H4.T).sum(axis=(2, 3)) // 2).sum())


class Pic:
    """A reference picture and its half-sample planes, fetched as the kernels do: coordinates
    clamp to the picture (integer samples) or to the planes' 4-sample margin, which equals the
    edge extension at any distance."""

    def __init__(self, ref):
        self.H, self.W = ref.shape
        self.p = Planes(ref).p

    def _fetch(self, pl, x, y, n):
        m = 0 if pl == 0 else 4
        xs = np.clip(np.arange(x, x + n), -m, self.W - 1 + m) + PAD
        ys = np.clip(np.arange(y, y + n), -m, self.H - 1 + m) + PAD
        return self.p[pl][np.ix_(ys, xs)]

    def block(self, x0, y0, mvx, mvy, n=8):
        x, y = x0 + (mvx >> 2), y0 + (mvy >> 2)
        (pa, ax, ay), (pb, bx, by) = _TAPS[(mvx & 3, mvy & 3)]
        return (self._fetch(pa, x + ax, y + ay, n) + self._fetch(pb, x + bx, y + by, n) + 1) >> 1


def quadrant_search(pic, src8, X, Y, L, k, cands, spx, spy):
    """the search of one quadrant in farther picture k -> (cost, x, y)"""
    def price(x, y):
        return satd8(src8, pic.block(X, Y, x, y)) + L * (se_bits(x - spx) + se_bits(y - spy) + ref_bits(k))
    kc = None
    for cx, cy in cands:
        x, y = clampi(int(cx), *MVX), clampi(int(cy), *MVY)
        p = price(x, y)
        if kc is None or p < kc:
            kc, kx, ky = p, x, y
    for step in (2, 1):
        ox, oy, rb = kx, ky, None
        for i in range(8):
            dx, dy = ring(i + 1, step)
            x, y = clampi(ox + dx, *MVX), clampi(oy + dy, *MVY)
            p = price(x, y)
            if rb is None or p < rb[0]:
                rb = (p, x, y)
        if rb[0] < kc:
            kc, kx, ky = rb
    return kc, kx, ky


def mixed_candidate(L, wmb, m, mv, mv8, pm, xmv, searched, scale, src0, src, pics, overhead, min_satd):
    """(c) of one MB -> None (not priced) or (cost, [(ref, x, y)] * 4).
    searched: the farther pictures k with a cost; scale[k - 1], xmv[k - 1] and pics[k] belong to k"""
    mx, my = m % wmb, m // wmb
    px, py = int(pm[0]), int(pm[1])
    quad, satd0 = [], 0
    for q in range(4):
        X, Y = mx * 16 + (q & 1) * 8, my * 16 + (q >> 1) * 8
        vx, vy = int(mv8[q][0]), int(mv8[q][1])
        s = satd8(src0[Y:Y + 8, X:X + 8], pics[0].block(X, Y, vx, vy))
        satd0 += s
        quad.append([s + L * (se_bits(vx - px) + se_bits(vy - py) + 1), 0, vx, vy])
    if satd0 <= min_satd:
        return None
    for k in searched:
        s = int(scale[k - 1])
        spx, spy = scale_mv(s, px, *MVX), scale_mv(s, py, *MVY)
        for q in range(4):
            X, Y = mx * 16 + (q & 1) * 8, my * 16 + (q >> 1) * 8
            cands = [(int(xmv[k - 1][0]), int(xmv[k - 1][1])),
                     (scale_mv(s, mv8[q][0], *MVX), scale_mv(s, mv8[q][1], *MVY)),
                     (scale_mv(s, mv[0], *MVX), scale_mv(s, mv[1], *MVY)), (0, 0)]
            kc, kx, ky = quadrant_search(pics[k], src[Y:Y + 8, X:X + 8], X, Y, L, k, cands, spx, spy)
            if kc < quad[q][0]:
                quad[q] = [kc, k, kx, ky]
    return sum(c[0] for c in quad) + L * overhead, [(c[1], c[2], c[3]) for c in quad]


def p_mixed_refs(lam, wmb, hmb, nref, kinds, n0, l0, qp, aq, mv, mv8, cost, pred, xmv, xcost, xpred, mref, mref4,
                 src0, src, pool, pm, scale, overhead, min_satd):
    """The whole launch.  kinds / n0 / l0: the route rows ([B], [B], [B, 4]); pool [B, nbuf, H, W];
    scale [nref - 1, B]; aq may be None.  Returns a dict of the outputs and ``winner`` [B, nmb]
    (0 untouched slot, 1 (a), 2 (b), 3 (c))."""
    mv, mv8, cost, pred, mref, mref4 = (np.array(x) for x in (mv, mv8, cost, pred, mref, mref4))
    B, nmb = cost.shape
    winner = np.zeros((B, nmb), dtype=np.int8)
    pics = {}
    for b in range(B):
        if kinds[b] != 0:
            continue
        nr = min(nref, int(n0[b]))

        def pic(k, b=b):
            key = (b, int(l0[b][k]))
            if key not in pics:
                pics[key] = Pic(pool[b, max(0, int(l0[b][k]))])
            return pics[key]
        for m in range(nmb):
            L = int(lam[clampi(int(qp[b]) + (0 if aq is None else int(aq[b, m])), 0, 51)])
            c_in = int(cost[b, m])
            best, bk, bc, searched = c_in + L, 0, 0, []
            for k in range(1, nr):
                c = int(xcost[k - 1, b, m])
                if c >= KNO:
                    continue
                searched.append(k)
                if c + L * (k + 2) < best:
                    best, bk, bc = c + L * (k + 2), k, c
            cc = None
            if searched:
                cc = mixed_candidate(L, wmb, m, mv[b, m], mv8[b, m], pm[b, m], xmv[:, b, m], searched, scale[:, b],
                                     src0[b], src[b], {k: pic(k) for k in [0] + searched}, overhead, min_satd)
            if cc is not None and len(set(cc[1])) > 1 and any(r for r, _, _ in cc[1]) and cc[0] < best:
                winner[b, m] = 3
                mx, my = m % wmb, m // wmb
                p16 = pred[b, m].reshape(16, 16)
                for q, (r, x, y) in enumerate(cc[1]):
                    mv8[b, m, q] = (x, y)
                    mref4[b, m, q] = r
                    if r > 0:
                        X, Y = mx * 16 + (q & 1) * 8, my * 16 + (q >> 1) * 8
                        p16[(q >> 1) * 8:(q >> 1) * 8 + 8, (q & 1) * 8:(q & 1) * 8 + 8] = pic(r).block(X, Y, x, y)
                mv[b, m] = mv8[b, m, 0]
                mref[b, m] = mref4[b, m, 0]
                cost[b, m] = (bc if bk else c_in) + cc[0] - best
                continue
            winner[b, m] = 2 if bk else 1
            mref[b, m] = bk
            mref4[b, m] = bk
            if bk:
                mv[b, m] = xmv[bk - 1, b, m]
                mv8[b, m] = xmv[bk - 1, b, m]
                cost[b, m] = bc
                pred[b, m] = xpred[bk - 1, b, m]
    return dict(mv=mv, mv8=mv8, cost=cost, pred=pred, mref=mref, mref4=mref4, winner=winner)
