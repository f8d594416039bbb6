"""numpy statement of the HEVC transform / quantiser / reconstruction of one transform block
(``hv::transform_quant_block``, csrc/kernels/hevc_common.h) with rate-distortion optimised
quantisation (csrc/kernels/hevc_rdoq.h, x265 --rdoq-level 1 / 2).  Plain int64; it imports
nothing of the package: the DST-VII matrix and the scans of 6.5.3 - 6.5.5 are its own copies,
the 32-point DCT matrix is handed in (``host.table("hevc_dct32")``).

This docstring is the normative text of the RDOQ rule.  All arithmetic is integer.

Quantiser constants of a TU of size n = 1 << log2n at Qp' = qp and bit depth bd:
``qbits = 14 + qp // 6 + (15 - bd - log2n)`` (>= 14), ``qscale = QUANT_SCALE[qp % 6]``.

Level 0 (today's quantiser): ``l = min(32767, (|c| * qscale + (off << (qbits - 9))) >> qbits)``
with the dead zone off = 171 (intra) or 85 (inter).

Levels 1 and 2.  For the coefficient c at coder scan position ``p = 16 * group + q`` (groups and
positions inside a group both in the order of the TU's scanIdx; the DC coefficient is p = 0):

* ``z = |c| * qscale``; ``lr = min(32767, (z + (1 << (qbits - 1))) >> qbits)`` (to nearest).
* Candidates: lr, then lr - 1 when that is >= 1, then 0 when lr <= 2.
* ``e(l) = min(16383, (z - (l << qbits)) >> (qbits - 8))`` (arithmetic shift), ``D(l) = e(l)^2``
  in (1 / 256 step)^2.  Only a clipped lr reaches the bound; it keeps e in the 15-bit field of the
  kernel's packed word.  e(l) = e(lr) + 256 (lr - l) below the bound.
* Rate R(l, seen, p) in 1 / 16 bit, ``seen`` = a later scan position keeps a non-zero level:
  R(0) = SIG0 when seen, else 0.  R(l >= 1) = SIG1 + SIGN + G(l), plus LAST(p) when not seen.
  G(1) = GT1_NO, G(2) = GT1_YES + GT2_NO, G(l >= 3) = GT1_YES + GT2_YES + 16 * bins(l - 3) with
  bins(r) = r + 1 for r < 4, else 5 + 2 floor(log2(r - 3)) (Golomb-Rice, cRiceParam 0).
  LAST(p) = LAST_BASE + LAST_STEP * floor(log2(p + 1)).
* ``J(l) = D(l) + lam * R(l, seen, p)``, ``lam = round(rdoq_lambda * 368)`` (0 <= lam <= 1472);
  the smallest J wins, ties go to the smaller level.
* The pass runs from the last scan position to the first; seen starts false and becomes true at
  the first non-zero choice.

Level 2 then clears whole 4x4 groups.  Every group decides from the levels of the pass above
(no group sees another's decision).  A group is a candidate when it is not group 0 of the scan,
holds a non-zero level, and every lr in it is <= 2; it is cleared when
``sum D(0) + lam * CSBF0 < sum (D(l) + lam * R(l, true, p)) + lam * CSBF1`` over its 16 positions.

Sign data hiding runs after this on the chosen levels, with the remainder e(level) where the
dead-zone quantiser has its own remainder ``(z - (l << qbits)) >> (qbits - 8)`` (kept modulo 2^15
there, as the kernel's field does).  Its rule, from the kernel's comments (7.4.9.11; HM's parity
fix): in every 4x4 group whose significant span exceeds 3 scan positions the sum of absolute levels
must be odd exactly when the first significant coefficient is negative; otherwise one level moves
by one, at the position with the smallest cost: a non-zero level with remainder > 0 grows at cost
-remainder, otherwise shrinks at cost +remainder (never a +-1 at the group's first significant
position); a zero grows at cost -remainder, unless it lies before the first significant position
and its coefficient's sign differs from that position's.  Candidates are visited from scan position
15 (from the last significant one in the TU's last significant group) down to 0, the first
strictly smallest cost wins; 32767 shrinks.
"""
import numpy as np

QUANT_SCALE = (26214, 23302, 20560, 18396, 16384, 14564)
LEVEL_SCALE = (40, 45, 51, 57, 64, 72)
DST4 = np.array([[29, 55, 74, 84], [74, 74, 0, -74], [84, -29, -74, 55], [55, -84, 74, -29]], dtype=np.int64)

SIG0, SIG1, SIGN = 9, 22, 16
GT1_NO, GT1_YES, GT2_NO, GT2_YES = 10, 24, 11, 22
LAST_BASE, LAST_STEP = 24, 20
CSBF0, CSBF1 = 8, 18
LAM_SCALE = 368
ERR_MAX = 16383


def lam_of(rdoq_lambda):
    return int(round(rdoq_lambda * LAM_SCALE))


# ---------------------------------------------------------------------------- scans (6.5.3 - 6.5.5)

def scan_order(scan, log2size):
    """[(x, y)] of scan positions 0 .. of a (1 << log2size)^2 grid: 0 up-right diagonal,
    1 horizontal, 2 vertical"""
    n = 1 << log2size
    if scan == 1:
        return [(i % n, i // n) for i in range(n * n)]
    if scan == 2:
        return [(i // n, i % n) for i in range(n * n)]
    out = []
    x, y = 0, 0
    while len(out) < n * n:  # 6.5.3
        while y >= 0:
            if x < n and y < n:
                out.append((x, y))
            y -= 1
            x += 1
        y = x
        x = 0
    return out


_POS = {}


def positions(scan, log2n):
    """(order, pos): order[p] = (x, y) of coder scan position p of the TU, pos[y, x] = p"""
    key = (scan, log2n)
    if key not in _POS:
        order = [(4 * gx + x, 4 * gy + y) for gx, gy in scan_order(scan, log2n - 2) for x, y in scan_order(scan, 2)]
        pos = np.zeros((1 << log2n, 1 << log2n), dtype=np.int64)
        for p, (x, y) in enumerate(order):
            pos[y, x] = p
        _POS[key] = (order, pos)
    return _POS[key]


def tu_scan_idx(intra, luma, log2n, mode):
    """7.4.9.11: intra luma 4x4 / 8x8 and intra chroma 4x4 follow the prediction mode"""
    if not intra or not (log2n == 2 or (log2n == 3 and luma)):
        return 0
    return 2 if 6 <= mode <= 14 else (1 if 22 <= mode <= 30 else 0)


# ---------------------------------------------------------------------------- transforms

def matrix(dct32, log2n, dst=False):
    if dst:
        return DST4
    return np.asarray(dct32, dtype=np.int64).reshape(32, 32)[:: 32 >> log2n, : 1 << log2n]


def forward(res, C, log2n, bd):
    """coefficients [v, u] of the residual [y, x] with the encoder's stage shifts"""
    sh1, sh2 = log2n + bd - 9, log2n + 6
    s = (res.astype(np.int64) @ C.T + (1 << (sh1 - 1))) >> sh1
    return (C @ s + (1 << (sh2 - 1))) >> sh2


def dequant(lev, log2n, bd, qp):
    """8.6.3, flat scaling (m = 16)"""
    dsh = bd + log2n - 5
    d = (((lev.astype(np.int64) * (16 * LEVEL_SCALE[qp % 6])) << (qp // 6)) + (1 << (dsh - 1))) >> dsh
    return np.clip(d, -32768, 32767)


def inverse(d, C, bd):
    """8.6.4.2: columns, clip to 16 bits, rows"""
    s = np.clip((C.T @ d + 64) >> 7, -32768, 32767)
    sh = 20 - bd
    return (s @ C + (1 << (sh - 1))) >> sh


# ---------------------------------------------------------------------------- quantisers

def qparams(log2n, bd, qp):
    return 14 + qp // 6 + (15 - bd - log2n), QUANT_SCALE[qp % 6]


def quant_deadzone(coef, log2n, bd, qp, intra):
    """today's quantiser: (absolute levels, remainders as the kernel's 15-bit field holds them)"""
    qbits, qscale = qparams(log2n, bd, qp)
    z = np.abs(coef.astype(np.int64)) * qscale
    l = np.minimum(32767, (z + ((171 if intra else 85) << (qbits - 9))) >> qbits)
    dl = (z - (l << qbits)) >> (qbits - 8)
    return l, ((dl & 0x7FFF) ^ 0x4000) - 0x4000


def g_bits(l):
    if l == 1:
        return GT1_NO
    if l == 2:
        return GT1_YES + GT2_NO
    r = l - 3
    bins = r + 1 if r < 4 else 5 + 2 * ((r - 3).bit_length() - 1)
    return GT1_YES + GT2_YES + 16 * bins


def rate(l, seen, p):
    if l == 0:
        return SIG0 if seen else 0
    return SIG1 + SIGN + g_bits(l) + (0 if seen else LAST_BASE + LAST_STEP * ((p + 1).bit_length() - 1))


def round_nearest(a, qscale, qbits):
    """(lr, e(lr)) of |c| = a"""
    z = int(a) * qscale
    lr = min(32767, (z + (1 << (qbits - 1))) >> qbits)
    return lr, min(ERR_MAX, (z - (lr << qbits)) >> (qbits - 8))


def err(e0, lr, l):
    return min(ERR_MAX, e0 + (lr - l) * 256)


def candidates(lr):
    c = [lr]
    if lr - 1 >= 1:
        c.append(lr - 1)
    if lr <= 2 and lr > 0:
        c.append(0)
    return c


def choose(lr, e0, lam, p, seen):
    best, jb = None, None
    for l in candidates(lr):  # descending: `<=` gives ties to the smaller level
        e = err(e0, lr, l)
        j = e * e + lam * rate(l, seen, p)
        if jb is None or j <= jb:
            best, jb = l, j
    return best


def rdoq_serial(coef, log2n, bd, qp, scan, level, lam):
    """the rule as written above: (absolute levels [v, u], remainders e(level))"""
    qbits, qscale = qparams(log2n, bd, qp)
    order, _ = positions(scan, log2n)
    n = 1 << log2n
    z = np.abs(coef.astype(np.int64)) * qscale
    lr = np.minimum(32767, (z + (1 << (qbits - 1))) >> qbits)
    e0 = np.minimum(ERR_MAX, (z - (lr << qbits)) >> (qbits - 8))
    lev = np.zeros((n, n), dtype=np.int64)
    seen = False
    for p in range(n * n - 1, -1, -1):
        x, y = order[p]
        if lr[y, x] == 0:  # 0 is the only candidate
            continue
        l = choose(int(lr[y, x]), int(e0[y, x]), lam, p, seen)
        lev[y, x] = l
        seen = seen or l != 0
    if level >= 2:
        clear = []
        for g in range(1, n * n // 16):
            xy = order[16 * g: 16 * g + 16]
            ls = [int(lev[y, x]) for x, y in xy]
            if not any(ls) or any(lr[y, x] > 2 for x, y in xy):
                continue
            d0 = sum(err(int(e0[y, x]), int(lr[y, x]), 0) ** 2 for x, y in xy)
            d1 = sum(err(int(e0[y, x]), int(lr[y, x]), l) ** 2 + lam * rate(l, True, 16 * g + q)
                     for q, ((x, y), l) in enumerate(zip(xy, ls)))
            if d0 + lam * CSBF0 < d1 + lam * CSBF1:
                clear.append(g)
        for g in clear:
            for x, y in order[16 * g: 16 * g + 16]:
                lev[y, x] = 0
    return lev, np.minimum(ERR_MAX, e0 + (lr - lev) * 256)


def rdoq_parallel(coef, log2n, bd, qp, scan, lam):
    """the lane-parallel form of the level-1 pass, vectorised: every coefficient evaluates its
    seen = false and its seen = true choice; the largest p whose false choice is non-zero takes it,
    positions above take 0, positions below their true choice"""
    qbits, qscale = qparams(log2n, bd, qp)
    _, pos = positions(scan, log2n)
    z = np.abs(coef.astype(np.int64)) * qscale
    lr = np.minimum(32767, (z + (1 << (qbits - 1))) >> qbits)
    e0 = np.minimum(ERR_MAX, (z - (lr << qbits)) >> (qbits - 8))
    lastc = LAST_BASE + LAST_STEP * (np.floor(np.log2(pos + 1.0)).astype(np.int64))
    gv = np.vectorize(lambda l: g_bits(int(l)) if l > 0 else 0, otypes=[np.int64])

    def pick(seen):
        best = lr.copy()
        jb = None
        for k, ok in ((0, lr >= 0), (1, lr >= 2), (2, (lr >= 1) & (lr <= 2))):
            l = lr - k if k < 2 else np.zeros_like(lr)
            e = np.minimum(ERR_MAX, e0 + (lr - l) * 256)
            r = np.where(l == 0, SIG0 if seen else 0, SIG1 + SIGN + gv(l) + (0 if seen else lastc))
            j = e * e + lam * r
            if jb is None:
                jb = j
                continue
            take = ok & (j <= jb)
            best = np.where(take, l, best)
            jb = np.where(take, j, jb)
        return best

    lf, lt = pick(False), pick(True)
    pmax = int(pos[lf != 0].max()) if (lf != 0).any() else -1
    return np.where(pos > pmax, 0, np.where(pos == pmax, lf, lt))


# ---------------------------------------------------------------------------- sign data hiding

def sdh_parity(lev, rem, neg, log2n, scan):
    """the parity pass on signed levels [v, u] (changed in place): rem the remainders, neg the
    coefficients' signs"""
    order, _ = positions(scan, log2n)
    ngr = (1 << log2n) ** 2 // 16
    gnz = [any(lev[order[p][1], order[p][0]] != 0 for p in range(16 * g, 16 * g + 16)) for g in range(ngr)]
    lastg = max([g for g in range(ngr) if gnz[g]], default=-1)
    for g in range(ngr):
        if not gnz[g]:
            continue
        xy = [order[16 * g + q] for q in range(16)]
        lv = [int(lev[y, x]) for x, y in xy]
        sig = [q for q in range(16) if lv[q]]
        first, last = sig[0], sig[-1]
        signbit = 1 if lv[first] < 0 else 0
        if not (last - first > 3 and (sum(abs(v) for v in lv) & 1) != signbit):
            continue
        best, bq, bch = 0x7FFFFFFF, first, 1
        for q in range(last if g == lastg else 15, -1, -1):
            x, y = xy[q]
            dl = int(rem[y, x])
            ch = 1
            if lv[q] != 0:
                if dl > 0:
                    cost = -dl
                elif q == first and abs(lv[q]) == 1:
                    cost = 0x7FFFFFFF
                else:
                    cost, ch = dl, -1
            elif q < first and int(neg[y, x]) != signbit:
                cost = 0x7FFFFFFF
            else:
                cost = -dl
            if cost < best:
                best, bq, bch = cost, q, ch
        x, y = xy[bq]
        if abs(lv[bq]) == 32767:
            bch = -1
        lev[y, x] = lv[bq] + (-bch if neg[y, x] else bch)
    return lev


# ---------------------------------------------------------------------------- the block function

def quantise(coef, log2n, bd, qp, intra, scan, sdh, rdoq, lam):
    """signed levels [v, u] of a coefficient block"""
    if rdoq:
        a, rem = rdoq_serial(coef, log2n, bd, qp, scan, rdoq, lam)
    else:
        a, rem = quant_deadzone(coef, log2n, bd, qp, intra)
    neg = coef < 0
    lev = np.where(neg, -a, a)
    if sdh:
        lev = sdh_parity(lev, rem, neg, log2n, scan)
    return lev


def transform_quant_block(res, dct32, log2n, bd, qp, intra, dst=False, scan=0, sdh=False, rdoq=0, lam=0):
    """(levels, reconstructed residual, flag) of the residual block [y, x]; the reconstructed
    residual of a block without levels is zero"""
    C = matrix(dct32, log2n, dst)
    lev = quantise(forward(res, C, log2n, bd), log2n, bd, qp, intra, scan, sdh, rdoq, lam)
    if not lev.any():
        return lev, np.zeros_like(lev), 0
    return lev, inverse(dequant(lev, log2n, bd, qp), C, bd), 1
