"""numpy statement of the HEVC merge decision passes (csrc/kernels/hevc_merge.hip): ``b_choose``,
``b_init_p``, ``b_merge_pass`` and ``merge_refine_pass``, one slot at a time, plain int64.

Written from the HEVC specification (6.4.1 z-scan availability, 8.5.3.2.2 - 8.5.3.2.5 merge
candidates) and from what the kernels' header comments document as their deliberate
approximations (the quarter-sample proxy prediction of qpel.h, SATD + lambda * bins prices, the
Jacobi passes, ``hevc_merge_refine``'s neighbour-vector list).  It imports nothing of the package.

A *motion* is the tuple ``(dir, x0, y0, x1, y1)``: ``dir`` is the direction byte (CuDir 1 = L0,
2 = L1, 3 = bi in bits 0-1, the list-0 refIdx in bits 2-3), the vectors are in quarter samples,
and the vector of a list the motion does not use is zero.  Two motions are equal when all five
numbers are.

``merge_list`` is the normative list of a 16x16 CU (2Nx2N, parallel merge level 2) whose
neighbours are all inter 16x16 CUs, under the encoder's restrictions:

* a B picture uses refIdx 0 in both lists (so the direction byte of a B motion is 1, 2 or 3), and
* RefPicList0[0] and RefPicList1[0] are different pictures, so the combined bi-predictive
  candidate's "different pictures or different vectors" test (8.5.3.2.4) is always true.

Every function also returns a per-block record of what happened (which neighbours were available,
which pruning rule fired, where each list entry came from, which entry won), from which the GPU
tests assert their coverage.
"""
import numpy as np

import ref_models_me as mm

KNO = 0x3FFFFFFF
NEIGHBOURS = ("A1", "B1", "B0", "A0", "B2")
SOURCES = NEIGHBOURS + ("T", "C", "Z")  # spatial, temporal, combined bi-predictive, zero
RULES = ("A1-B1", "B1-B0", "A1-A0", "A1-B2", "B1-B2", "four-no-B2", "T-full")

# 8.5.3.2.4, table of l0CandIdx / l1CandIdx by combIdx
COMB_L0 = (0, 1, 0, 2, 1, 2, 0, 3, 1, 3, 2, 3)
COMB_L1 = (1, 0, 2, 0, 2, 1, 3, 0, 3, 1, 3, 2)

# quarter phase (xf, yf) -> two (plane, dx, dy) taps of the G / b / h / j form (qpel.h kQTap):
# planes 0 G (integer), 1 b (half x), 2 h (half y), 3 j (centre); the sample is (a + b + 1) >> 1
QTAP = {
    (0, 0): ((0, 0, 0), (0, 0, 0)), (1, 0): ((0, 0, 0), (1, 0, 0)), (2, 0): ((1, 0, 0), (1, 0, 0)),
    (3, 0): ((0, 1, 0), (1, 0, 0)), (0, 1): ((0, 0, 0), (2, 0, 0)), (1, 1): ((1, 0, 0), (2, 0, 0)),
    (2, 1): ((3, 0, 0), (1, 0, 0)), (3, 1): ((1, 0, 0), (2, 1, 0)), (0, 2): ((2, 0, 0), (2, 0, 0)),
    (1, 2): ((3, 0, 0), (2, 0, 0)), (2, 2): ((3, 0, 0), (3, 0, 0)), (3, 2): ((3, 0, 0), (2, 1, 0)),
    (0, 3): ((0, 0, 1), (2, 0, 0)), (1, 3): ((1, 0, 1), (2, 0, 0)), (2, 3): ((3, 0, 0), (1, 0, 1)),
    (3, 3): ((1, 0, 1), (2, 1, 0)),
}

_EDGE = 32  # beyond 3 samples outside the picture every plane repeats its edge; clamp well past that


class Pred:
    """Quarter-sample prediction from an 8-bit picture extended infinitely by its edge samples.

    The half-sample planes are those of ``ref_models_me.Planes`` (padded by 192 samples, with
    wrap-around garbage in its outermost samples); a sample further than ``_EDGE`` outside the
    picture equals the one ``_EDGE`` outside, so coordinates clamp there and any vector is valid.
    """

    def __init__(self, ref):
        self.H, self.W = ref.shape
        self.p = mm.Planes(ref).p

    def _fetch(self, plane, x, y):
        ys = np.clip(y + np.arange(16), -_EDGE, self.H - 1 + _EDGE) + mm.PAD
        xs = np.clip(x + np.arange(16), -_EDGE, self.W - 1 + _EDGE) + mm.PAD
        return self.p[plane][np.ix_(ys, xs)]

    def block(self, x0, y0, mvx, mvy):
        """the 16x16 block at (x0, y0) displaced by (mvx, mvy) quarter samples"""
        mvx, mvy = int(mvx), int(mvy)
        x, y = x0 + (mvx >> 2), y0 + (mvy >> 2)
        (pa, ax, ay), (pb, bx, by) = QTAP[(mvx & 3, mvy & 3)]
        return (self._fetch(pa, x + ax, y + ay) + self._fetch(pb, x + bx, y + by) + 1) >> 1


def bipred(p0, p1):
    return (p0 + p1 + 1) >> 1


def satd16(src, pred):
    """sum over the sixteen 4x4 blocks of |H4 d H4^T|, halved (the sum is even)"""
    t = mm.hsum_mb(np.asarray(src, dtype=np.int64) - np.asarray(pred, dtype=np.int64))
    assert t % 2 == 0
    return t // 2


def lambdas(lam_tab, qp, aq):
    """lambda of every block of a slot: lam_tab[clip(qp + aq[blk], 0, 51)]"""
    q = np.clip(int(qp) + np.asarray(aq, dtype=np.int64), 0, 51)
    return np.asarray(lam_tab, dtype=np.int64)[q]


se_bits = mm.se_bits


def mvd_bits(mv, pm):
    return se_bits(int(mv[0]) - int(pm[0])) + se_bits(int(mv[1]) - int(pm[1]))


def ref_bins(r, nref0):
    """ref_idx_l0 bins: truncated Rice with cMax nref0 - 1"""
    return 0 if nref0 <= 1 else min(r + 1, nref0 - 1)


def motion(d, v):
    """(dir byte, 4 vector components) -> motion, the unused list's vector zeroed"""
    d = int(d)
    return (d, int(v[0]) if d & 1 else 0, int(v[1]) if d & 1 else 0, int(v[2]) if d & 2 else 0, int(v[3]) if d & 2 else 0)


def predict(m, X0, Y0, l0, l1):
    """luma prediction of a motion: l0 the list of RefPicList0's ``Pred``s, l1 that of RefPicList1[0]"""
    d = m[0] & 3
    if d == 1:
        return l0[(m[0] >> 2) & 3].block(X0, Y0, m[1], m[2])
    if d == 2:
        return l1.block(X0, Y0, m[3], m[4])
    return bipred(l0[(m[0] >> 2) & 3].block(X0, Y0, m[1], m[2]), l1.block(X0, Y0, m[3], m[4]))


# ---------------------------------------------------------------------------- 6.4.1 availability

def coding_order(wmb, hmb, ctu_shift):
    """[hmb, wmb] position in coding order of every 16x16 block: CTUs of (1 << ctu_shift)^2 blocks
    in raster order, the blocks of a CTU in z-order (blocks outside the picture are not coded)"""
    n = 1 << ctu_shift
    order = np.full((hmb, wmb), -1, dtype=np.int64)
    k = 0

    def z(x, y, size):
        nonlocal k
        if x >= wmb or y >= hmb:
            return
        if size == 1:
            order[y, x] = k
            k += 1
            return
        h = size // 2
        for qy, qx in ((0, 0), (0, 1), (1, 0), (1, 1)):
            z(x + qx * h, y + qy * h, h)
    for cy in range(0, hmb, n):
        for cx in range(0, wmb, n):
            z(cx, cy, n)
    return order


def available(order, nx, ny, mx, my):
    """6.4.1: the neighbour lies in the picture and precedes the current block in coding order"""
    hmb, wmb = order.shape
    if nx < 0 or ny < 0 or nx >= wmb or ny >= hmb:
        return False
    return bool(order[ny, nx] < order[my, mx])


def neighbour_positions(mx, my):
    return {"A1": (mx - 1, my), "B1": (mx, my - 1), "B0": (mx + 1, my - 1), "A0": (mx - 1, my + 1), "B2": (mx - 1, my - 1)}


# ---------------------------------------------------------------------------- the merge list

def merge_list(nb, temporal, bslice, max_merge, nref0=1):
    """8.5.3.2.2 - 8.5.3.2.5.  ``nb``: the motions of the available neighbours by name (an
    unavailable one is missing or None); ``temporal``: the temporal candidate's motion or None.
    -> (list of motions, list of their sources, list of the pruning rules that fired)"""
    g = lambda k: nb.get(k)  # noqa: E731
    fired = []
    flag = {k: g(k) is not None for k in NEIGHBOURS}

    def prune(k, against, rule):
        if flag[k] and g(against) is not None and g(against) == g(k):
            flag[k] = False
            fired.append(rule)
    prune("B1", "A1", "A1-B1")
    prune("B0", "B1", "B1-B0")
    prune("A0", "A1", "A1-A0")
    prune("B2", "A1", "A1-B2")
    prune("B2", "B1", "B1-B2")
    if flag["B2"] and flag["A0"] and flag["A1"] and flag["B0"] and flag["B1"]:
        flag["B2"] = False
        fired.append("four-no-B2")
    lst = [g(k) for k in NEIGHBOURS if flag[k]]
    src = [k for k in NEIGHBOURS if flag[k]]
    if temporal is not None:
        if len(lst) < max_merge:
            lst.append(temporal)
            src.append("T")
        else:
            fired.append("T-full")
    norig = len(lst)
    if bslice and 1 < norig < max_merge:
        for comb in range(norig * (norig - 1)):
            if len(lst) == max_merge:
                break
            c0, c1 = lst[COMB_L0[comb]], lst[COMB_L1[comb]]
            # predFlagL0 of the one, predFlagL1 of the other; the picture / vector test always holds
            if (c0[0] & 1) and (c1[0] & 2):
                lst.append((3, c0[1], c0[2], c1[3], c1[4]))
                src.append("C")
    zero_idx = 0
    num_ref = 1 if bslice else nref0  # B: min of the two lists' sizes
    while len(lst) < max_merge:
        r = zero_idx if zero_idx < num_ref else 0
        lst.append((3, 0, 0, 0, 0) if bslice else (1 | (r << 2), 0, 0, 0, 0))
        src.append("Z")
        zero_idx += 1
    return lst[:max_merge], src[:max_merge], fired


def block_merge_list(dirs, mvs, order, mx, my, tdir, tmv, bslice, max_merge, nref0=1):
    """the list of block (mx, my) on a motion field (dirs [nmb], mvs [nmb, 4]); tdir / tmv: the
    block's temporal candidate (direction 0 or None: none).  -> (list, sources, fired, inpic, avail)"""
    hmb, wmb = order.shape
    nb, inpic, avail = {}, {}, {}
    for k, (nx, ny) in neighbour_positions(mx, my).items():
        inpic[k] = 0 <= nx < wmb and 0 <= ny < hmb
        avail[k] = available(order, nx, ny, mx, my)
        if avail[k]:
            n = ny * wmb + nx
            nb[k] = motion(dirs[n], mvs[n])
    t = None
    if tdir is not None and int(tdir) != 0:
        t = motion(3, tmv) if bslice else motion(1, tmv)
    lst, src, fired = merge_list(nb, t, bslice, max_merge, nref0)
    return lst, src, fired, inpic, avail


# ---------------------------------------------------------------------------- the passes

def b_choose(src, p0, p1, mv0, mv1, cost0, cost1, pm0, pm1, lam, wmb, hmb):
    """L0 / L1 / bi from the two searches of a B picture's slot.  -> dict(mvb [nmb, 4], dir, cost,
    bits [nmb]), record [nmb] of dict(choice)"""
    nmb = wmb * hmb
    s = src.astype(np.int64)
    out = dict(mvb=np.zeros((nmb, 4), dtype=np.int64), dir=np.zeros(nmb, dtype=np.int64),
               cost=np.zeros(nmb, dtype=np.int64), bits=np.zeros(nmb, dtype=np.int64))
    rec = []
    for mb in range(nmb):
        X0, Y0 = (mb % wmb) * 16, (mb // wmb) * 16
        S = s[Y0:Y0 + 16, X0:X0 + 16]
        la = int(lam[mb])
        b0, b1 = mvd_bits(mv0[mb], pm0[mb]), mvd_bits(mv1[mb], pm1[mb])
        bi = bipred(p0.block(X0, Y0, *mv0[mb]), p1.block(X0, Y0, *mv1[mb]))
        # inter_pred_idc: one bin for bi, two for a single list
        best, d, bits = int(cost0[mb]) + 2 * la, 1, b0 + 2
        c = int(cost1[mb]) + 2 * la
        if c < best:
            best, d, bits = c, 2, b1 + 2
        c = satd16(S, bi) + la * (b0 + b1 + 1)
        if c < best:
            best, d, bits = c, 3, b0 + b1 + 1
        out["mvb"][mb] = motion(d, (mv0[mb][0], mv0[mb][1], mv1[mb][0], mv1[mb][1]))[1:]
        out["dir"][mb], out["cost"][mb], out["bits"][mb] = d, best, bits
        rec.append(dict(choice=("L0", "L1", "bi")[d - 1]))
    return out, rec


def b_init_p(mv0, cost0, pm0, lam, nref0=1, xmv=None, xcost=None, xpm=None):
    """A P picture's list-0 searches as B-form motion: search r = 0 is (mv0, cost0, pm0), the
    farther ones xmv / xcost / xpm [nref0 - 1, nmb, ...].  -> dict(mvb, dir, cost, bits), record
    [nmb] of dict(ref, skipped: unsearched refs, lost_to_bins: refs cheaper than the winner
    before the ref_idx bins)"""
    nmb = len(cost0)
    out = dict(mvb=np.zeros((nmb, 4), dtype=np.int64), dir=np.zeros(nmb, dtype=np.int64),
               cost=np.zeros(nmb, dtype=np.int64), bits=np.zeros(nmb, dtype=np.int64))
    rec = []
    for mb in range(nmb):
        la = int(lam[mb]) if nref0 > 1 else 0
        cands = [(0, int(cost0[mb]), mv0[mb], pm0[mb])]
        skipped = []
        for r in range(1, nref0):
            if int(xcost[r - 1][mb]) >= KNO:
                skipped.append(r)
                continue
            cands.append((r, int(xcost[r - 1][mb]), xmv[r - 1][mb], xpm[r - 1][mb]))
        best = None
        for r, c, mv, pm in cands:
            full = c + la * ref_bins(r, nref0)
            if best is None or full < best[0]:
                best = (full, r, mv, pm, c)
        full, r, mv, pm, raw = best
        out["mvb"][mb] = (int(mv[0]), int(mv[1]), 0, 0)
        out["dir"][mb] = 1 | (r << 2)
        out["cost"][mb] = full
        out["bits"][mb] = mvd_bits(mv, pm) + ref_bins(r, nref0)
        rec.append(dict(ref=r, skipped=skipped, lost_to_bins=[q for q, c, _, _ in cands if q != r and c < raw]))
    return out, rec


def merge_bins(j, max_merge):
    """merge_flag and the truncated-unary merge_idx of entry j"""
    return 1 + (min(j + 1, max_merge - 1) if max_merge > 1 else 0)


def b_merge_pass(src, l0, l1, dirs, mvs, cost, bits, lam, wmb, hmb, bslice, max_merge, ctu_shift, tdir=None,
                 tmv=None, nref0=1):
    """One Jacobi pass over a slot: every block is offered its merge list on the input field.
    l0: list of ``Pred`` (RefPicList0), l1: ``Pred`` of RefPicList1[0] (B) or None.
    -> dict(mvb, dir, cost, bits, chg), record [nmb]"""
    nmb = wmb * hmb
    s = src.astype(np.int64)
    order = coding_order(wmb, hmb, ctu_shift)
    out = dict(mvb=np.zeros((nmb, 4), dtype=np.int64), dir=np.zeros(nmb, dtype=np.int64),
               cost=np.zeros(nmb, dtype=np.int64), bits=np.zeros(nmb, dtype=np.int64), chg=np.zeros(nmb, dtype=np.int64))
    rec = []
    for mb in range(nmb):
        mx, my = mb % wmb, mb // wmb
        X0, Y0 = mx * 16, my * 16
        S = s[Y0:Y0 + 16, X0:X0 + 16]
        la = int(lam[mb])
        lst, srcs, fired, inpic, avail = block_merge_list(
            dirs, mvs, order, mx, my, None if tdir is None else tdir[mb], None if tmv is None else tmv[mb], bslice,
            max_merge, nref0)
        cur = motion(dirs[mb], mvs[mb])
        satd_cur = int(cost[mb]) - la * int(bits[mb])
        best, bbits, bj = int(cost[mb]), int(bits[mb]), -1
        dups = []
        for j, m in enumerate(lst):
            if m in lst[:j]:
                dups.append(j)
                continue
            sat = satd_cur if m == cur else satd16(S, predict(m, X0, Y0, l0, l1))
            nb = merge_bins(j, max_merge)
            if sat + la * nb < best:
                best, bbits, bj = sat + la * nb, nb, j
        if bj >= 0:
            out["mvb"][mb], out["dir"][mb] = lst[bj][1:], lst[bj][0]
        else:
            out["mvb"][mb], out["dir"][mb] = mvs[mb], dirs[mb]
        out["cost"][mb], out["bits"][mb] = best, bbits
        out["chg"][mb] = int(bj >= 0 and lst[bj] != cur)
        rec.append(dict(inpic=inpic, avail=avail, fired=fired, sources=srcs, list=lst, dups=dups, winner=bj,
                        winner_source=srcs[bj] if bj >= 0 else None, moved=bool(out["chg"][mb]),
                        repriced=bj >= 0 and lst[bj] == cur, kept=bj < 0))
    return out, rec


def chg_nearby(chg, wmb, hmb):
    """[nmb] bool: the block or one of the five blocks at its merge neighbours' picture positions
    (whatever their availability) carries a changed flag -- what a pass wired with the previous
    pass's flags re-evaluates; every other block copies its motion through"""
    c = np.asarray(chg).reshape(hmb, wmb) != 0
    p = np.zeros((hmb + 2, wmb + 2), dtype=bool)
    p[1:-1, 1:-1] = c
    near = p[1:-1, 1:-1] | p[1:-1, :-2] | p[:-2, 1:-1] | p[:-2, 2:] | p[2:, :-2] | p[:-2, :-2]
    return near.reshape(-1)


def merge_refine_pass(src, p, mv, cost, pm, lam, wmb, hmb):
    """hevc_merge_refine's documented approximation, one Jacobi pass over a slot: the vectors of
    A1, B1, B0, A0 (by picture position, no z-scan test) and B2, without repeats, then zero.
    -> dict(mv [nmb, 2], cost [nmb]), record [nmb]"""
    nmb = wmb * hmb
    s = src.astype(np.int64)
    out = dict(mv=np.zeros((nmb, 2), dtype=np.int64), cost=np.zeros(nmb, dtype=np.int64))
    rec = []
    for mb in range(nmb):
        mx, my = mb % wmb, mb // wmb
        X0, Y0 = mx * 16, my * 16
        S = s[Y0:Y0 + 16, X0:X0 + 16]
        la = int(lam[mb])
        pos = neighbour_positions(mx, my)
        cands, srcs = [], []
        for k in NEIGHBOURS:
            nx, ny = pos[k]
            if 0 <= nx < wmb and 0 <= ny < hmb:
                v = (int(mv[ny * wmb + nx][0]), int(mv[ny * wmb + nx][1]))
                if v not in cands:
                    cands.append(v)
                    srcs.append(k)
        if (0, 0) not in cands:
            cands.append((0, 0))
            srcs.append("Z")
        cur = (int(mv[mb][0]), int(mv[mb][1]))
        c_me = int(cost[mb])
        pmv = (0, 0) if pm is None else pm[mb]
        best, bv, bj, repriced, took_back = c_me, cur, -1, False, False
        for j, v in enumerate(cands):
            if v == cur:
                c = c_me - la * mvd_bits(cur, pmv) + la * (1 + j)
                if c < best:  # the searched vector, coded as merge: cheaper than anything so far
                    took_back = bj >= 0  # ... an earlier candidate that had beaten the search included
                    best, bv, bj, repriced = c, cur, -1, True
                continue
            c = satd16(S, p.block(X0, Y0, *v)) + la * (1 + j)
            if c < best:
                best, bv, bj = c, v, j
        out["mv"][mb], out["cost"][mb] = bv, best
        rec.append(dict(sources=srcs, list=cands, winner=bj, winner_source=srcs[bj] if bj >= 0 else None,
                        is_candidate=cur in cands, repriced=repriced and bj < 0, took_back=took_back and bj < 0,
                        kept=bj < 0))
    return out, rec
