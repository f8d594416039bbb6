"""The B decision's block fetch (``mc4x4``) and its lean passes against the general instance.

``b_decide`` has four instances.  The general one (``direct_only = 0, have_direct = 0``) prices
and writes everything itself and fetches its predictions row by row (``mc4``); the default
configuration runs the temporal-direct pre-pass (``direct_only = 1``) and the lean main pass
(``have_direct = 1``) instead, which fetch whole 4x4 blocks (``mc4x4``).  Both ways must give
the same bytes, so every case here is the general instance against pre-pass + main pass on the
same inputs, in one library.

1. Block fetch: the direct vectors are constructed so that every one of the 16 quarter-sample
   phases meets every edge class per list -- blocks well inside, across each picture edge by 1
   to ``kHpMargin + 3`` samples, far outside (40 samples), and columns whose aligned 8 bytes
   end exactly at the last byte of the integer or of the half-sample planes.  The test counts
   that from its own inputs and fails if a combination is missing.

   A quadrant without a temporal direct prediction (``dref = -1``) is priced from list 1 alone
   by the general instance and from list-0 entry 0 by the pre-pass (its MB's cost is kNoCost
   either way and the quadrant is never coded direct), so the prediction bytes of every MB are
   compared with a general launch whose -1 entries are replaced by 0, and the costs and the
   records with the launch on ``dref`` itself.

2. Gated and searched MBs: cost buffers holding a pattern of searched MBs (both list costs
   below kNoCost; the others are gated and stay B_Direct_16x16); ``hdr``, ``pred_out`` and
   ``cost_out`` must match whole, with and without ``bparts``; a routed launch leaves a slot
   that codes no B picture untouched.  The patterns and shapes (6, 15 and 99 MBs) are those a
   main pass that visits the searched MBs only, a wave per run of MBs, would have to get right.

3. End to end: whole encodes (temporal direct with weightb, two list-0 pictures with a
   b-pyramid, bpartitions, spatial direct on the fast path and in the wavefront with its gate).
   A decoder round trip cannot see a changed decision, so every case is checked three ways: the
   CPU decoder's reconstruction of the emitted stream equals the encoder's, bit for bit; the
   SHA-256 of every slot's bitstream equals the value the parent commit's kernels (row-by-row
   fetches) emitted for the same arguments, recorded on the GPU
   by ``tools/record_inter_layout.py bfetch`` into tests/golden/b_block_fetch_parent.json; and
   the counts below equal the parent's and are above zero where the case is there for them:

     b_gated / b_searched   MBs the gate stopped / let through in the B pictures' list searches
                            (from the encoder's cost buffers after each gated launch)
     direct                 B_Direct_16x16 / B_Skip MBs of the decoded records
     b8x8_direct            B_8x8 MBs with a B_Direct_8x8 quadrant

   The clips are synthetic ones with, per slot and frame, planted MBs that the direct prediction
   cannot follow: a texture that jumps from frame to frame (searched, explicit motion), one that
   covers two quadrants of an MB only (direct in the others), and noise.
"""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KNO = 0x3FFFFFFF
HP_MARGIN = 4
SENT = 0xEE
S_COST = -9

# csrc/kernels/qpel.h kQTap: per phase two (plane, du, dv) taps; plane 0 = integer samples
QTAP = [
    ((0, 0, 0), (0, 0, 0)), ((0, 0, 0), (1, 0, 0)), ((1, 0, 0), (1, 0, 0)), ((0, 1, 0), (1, 0, 0)),
    ((0, 0, 0), (2, 0, 0)), ((1, 0, 0), (2, 0, 0)), ((3, 0, 0), (1, 0, 0)), ((1, 0, 0), (2, 1, 0)),
    ((2, 0, 0), (2, 0, 0)), ((3, 0, 0), (2, 0, 0)), ((3, 0, 0), (3, 0, 0)), ((3, 0, 0), (2, 1, 0)),
    ((0, 0, 1), (2, 0, 0)), ((1, 0, 1), (2, 0, 0)), ((3, 0, 0), (1, 0, 1)), ((1, 0, 1), (2, 1, 0)),
]
CLASSES = ["inside", "left", "right", "top", "bottom", "far", "last8"]
NTABLES = 16


def _direct_vectors(B, wmb, hmb, t):
    """dmv [B, nmb, 2, 4, 2] of table t: vector n of a list takes class n % 8 and, over the
    16 tables, every phase."""
    W, H, nmb = wmb * 16, hmb * 16, wmb * hmb
    dmv = np.zeros((B, nmb, 2, 4, 2), dtype=np.int16)
    for b in range(B):
        for mb in range(nmb):
            for q in range(4):
                for l in range(2):
                    n = (b * nmb + mb) * 4 + q + 3 * l
                    c, s = n % 8, n // 8 + t
                    phase, d = s % 16, 1 + s % 7
                    qx, qy = (mb % wmb) * 16 + (q & 1) * 8, (mb // wmb) * 16 + (q >> 1) * 8
                    dx = 4 + (7 * n + 5 * t) % (W - 15) - qx   # both blocks of the quadrant well inside
                    dy = 4 + (3 * n + t) % (H - 15) - qy
                    if c == 1:
                        dx = -d - qx                            # first column d samples left of the picture
                    elif c == 2:
                        dx = (W - 1 + d - 3) - (qx + 4)         # second column d samples past the right edge
                    elif c == 3:
                        dy = -d - qy
                    elif c == 4:
                        dy = (H - 1 + d - 3) - (qy + 4)
                    elif c == 5:
                        v = (n // 8) % 4
                        if v == 0:
                            dx = -40 - qx
                        elif v == 1:
                            dx = W + 40 - qx
                        elif v == 2:
                            dy = -40 - qy
                        else:
                            dy = H + 40 - qy
                    elif c >= 6:
                        # second column: its aligned 8 bytes end at the last byte of the integer
                        # plane (c 6) or of the half-sample planes (c 7)
                        k = (n // 16 + t // 4) % 4
                        dx = (W - 8 if c == 6 else W - 4) + k - (qx + 4)
                    dmv[b, mb, l, q] = (4 * dx + (phase & 3), 4 * dy + (phase >> 2))
    return dmv


def _count_classes(dmv, wmb, hmb, seen, dists):
    """Which (list, phase, class) the blocks of a table fall in; dists: (list, edge, distance)."""
    W, H = wmb * 16, hmb * 16
    B, nmb = dmv.shape[:2]
    for b in range(B):
        for mb in range(nmb):
            for blk in range(16):
                X, Y = (mb % wmb) * 16 + (blk & 3) * 4, (mb // wmb) * 16 + (blk >> 2) * 4
                q = (blk >> 3) * 2 + ((blk >> 1) & 1)
                for l in range(2):
                    mvx, mvy = int(dmv[b, mb, l, q, 0]), int(dmv[b, mb, l, q, 1])
                    ph = (mvy & 3) * 4 + (mvx & 3)
                    xi, yi = X + (mvx >> 2), Y + (mvy >> 2)
                    xin, yin = 4 <= xi <= W - 8, 4 <= yi <= H - 8
                    if xin and yin:
                        seen.add((l, ph, "inside"))
                    if yin and -(HP_MARGIN + 3) <= xi <= -1:
                        seen.add((l, ph, "left"))
                        dists.add((l, "left", -xi))
                    if yin and 1 <= xi + 3 - (W - 1) <= HP_MARGIN + 3:
                        seen.add((l, ph, "right"))
                        dists.add((l, "right", xi + 3 - (W - 1)))
                    if xin and -(HP_MARGIN + 3) <= yi <= -1:
                        seen.add((l, ph, "top"))
                        dists.add((l, "top", -yi))
                    if xin and 1 <= yi + 3 - (H - 1) <= HP_MARGIN + 3:
                        seen.add((l, ph, "bottom"))
                        dists.add((l, "bottom", yi + 3 - (H - 1)))
                    if xi <= -36 or xi >= W + 36 or yi <= -36 or yi >= H + 36:
                        seen.add((l, ph, "far"))
                    for pl, du, dv in QTAP[ph]:
                        m = 0 if pl == 0 else HP_MARGIN
                        u, v = xi + du, yi + dv
                        a = (u + m) & ~3
                        if u >= -m and a + 8 == W + 2 * m and v >= -m and v + 3 <= H + m - 1:
                            seen.add((l, ph, "last8"))
                            dists.add((l, "last8", "integer" if pl == 0 else "half"))


def test_direct_vector_tables_cover_every_phase_and_edge():
    """(No GPU work: the coverage the block-fetch cases rely on, stated once per shape.)"""
    for wmb, hmb in ((3, 2), (4, 3), (5, 3)):
        seen, dists = set(), set()
        for t in range(NTABLES):
            _count_classes(_direct_vectors(2, wmb, hmb, t), wmb, hmb, seen, dists)
        missing = [(l, ph, c) for l in range(2) for ph in range(16) for c in CLASSES if (l, ph, c) not in seen]
        assert not missing, missing
        for l in range(2):
            for e in ("left", "right", "top", "bottom"):
                for d in range(1, HP_MARGIN + 4):
                    assert (l, e, d) in dists, (l, e, d)
            assert (l, "last8", "integer") in dists and (l, "last8", "half") in dists


# ---------------------------------------------------------------- launches


def _up(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda")


_PICS = {}


def _pictures(hip, B, wmb, hmb, nref=1):
    """Random source and reference pictures with their half-sample planes, made once per shape."""
    import torch
    key = (B, wmb, hmb, nref)
    if key not in _PICS:
        W, H = wmb * 16, hmb * 16
        rng = np.random.default_rng(1000 * wmb + 10 * hmb + nref)
        src = _up(rng.integers(0, 256, size=(B, H, W), dtype=np.uint8))
        # [list-0 pictures ..., the list-1 picture][B]
        refs = _up(rng.integers(0, 256, size=(nref + 1, B, H, W), dtype=np.uint8))
        hp = torch.zeros((nref + 1, B, 3, H + 8, W + 8), dtype=torch.uint8, device="cuda")
        hip.me_halfpel((nref + 1) * B, W, H, refs.data_ptr(), hp.data_ptr(), torch.cuda.current_stream().cuda_stream)
        nmb = wmb * hmb
        _PICS[key] = dict(
            src=src, refs=refs, hp=hp, qp=_up(np.array([26, 33][:B], dtype=np.int32)),
            aq=_up(rng.integers(-5, 6, size=(B, nmb)).astype(np.int8)),
            mv0=_up(rng.integers(-30, 31, size=(B, nmb, 2)).astype(np.int16)),
            mv1=_up(rng.integers(-30, 31, size=(B, nmb, 2)).astype(np.int16)),
            pm0=_up(rng.integers(-12, 13, size=(B, nmb, 2)).astype(np.int16)),
            pm1=_up(rng.integers(-12, 13, size=(B, nmb, 2)).astype(np.int16)),
            pred0=_up(rng.integers(0, 256, size=(B, nmb, 256), dtype=np.uint8)),
            pred1=_up(rng.integers(0, 256, size=(B, nmb, 256), dtype=np.uint8)),
            list_cost=rng.integers(300, 6000, size=(2, B, nmb)).astype(np.int32))
    return _PICS[key]


class _Outs:
    def __init__(self, B, nmb):
        import torch
        self.hdr = torch.full((B, nmb, 64), SENT, dtype=torch.uint8, device="cuda")
        self.pred = torch.full((B, nmb, 256), SENT, dtype=torch.uint8, device="cuda")
        self.cost = torch.full((B, nmb), S_COST, dtype=torch.int32, device="cuda")

    def numpy(self):
        import torch
        torch.cuda.synchronize()
        return self.hdr.cpu().numpy(), self.pred.cpu().numpy(), self.cost.cpu().numpy()


def _decide(hip, B, wmb, hmb, p, outs, dmv, cost0, cost1, *, direct_only, have_direct, bparts=0, w1=(32,), dref=None,
            route=None, nbuf=0, pools=None):
    import torch
    nref = len(w1)
    if pools is not None:  # routed: every plane pointer is a pool base
        r0 = r1 = pools[0].data_ptr()
        h0 = h1 = pools[1].data_ptr()
        rk, hk = [], []
    else:
        r0, r1, h0, h1 = p["refs"][0].data_ptr(), p["refs"][nref].data_ptr(), p["hp"][0].data_ptr(), p["hp"][nref].data_ptr()
        rk = [p["refs"][k].data_ptr() for k in range(1, nref)]
        hk = [p["hp"][k].data_ptr() for k in range(1, nref)]
    hip.b_decide(B, wmb, hmb, p["src"].data_ptr(), r0, r1, h0, h1, p["mv0"].data_ptr(), p["mv1"].data_ptr(),
                 cost0.data_ptr(), cost1.data_ptr(), p["pred0"].data_ptr(), p["pred1"].data_ptr(), p["pm0"].data_ptr(),
                 p["pm1"].data_ptr(), dmv.data_ptr(), p["qp"].data_ptr(), p["aq"].data_ptr(), outs.hdr.data_ptr(),
                 outs.pred.data_ptr(), outs.cost.data_ptr(), torch.cuda.current_stream().cuda_stream, list(w1),
                 dref.data_ptr() if dref is not None else 0, rk, hk, direct_only, bparts, have_direct, 0, 0,
                 route.data_ptr() if route is not None else 0, nbuf, 0)


def _general(hip, B, wmb, hmb, p, dmv, c0, c1, **kw):
    o = _Outs(B, wmb * hmb)
    _decide(hip, B, wmb, hmb, p, o, dmv, c0, c1, direct_only=0, have_direct=0, **kw)
    return o


def _two_pass(hip, B, wmb, hmb, p, dmv, c0, c1, **kw):
    """-> outputs after the pre-pass (numpy), outputs after the main pass"""
    o = _Outs(B, wmb * hmb)
    _decide(hip, B, wmb, hmb, p, o, dmv, c0, c1, direct_only=1, have_direct=0, **{**kw, "bparts": 0})
    pre = o.numpy()
    _decide(hip, B, wmb, hmb, p, o, dmv, c0, c1, direct_only=0, have_direct=1, **kw)
    return pre, o


# ---------------------------------------------------------------- 1. block fetch against mc4


def _dref_pattern(B, nmb):
    """refIdxL0 per quadrant in {0, 1, -1}: most MBs keep all four direct predictions."""
    d = np.zeros((B, nmb, 4), dtype=np.int8)
    for b in range(B):
        for mb in range(nmb):
            for q in range(4):
                d[b, mb, q] = -1 if (mb % 3 == 2 and q == (mb // 3 + b) % 4) else (mb + q + b) % 2
    return d


@pytest.mark.parametrize("weights", [(32,), (20,), (24, 41)], ids=["w32", "w20", "two-refs"])
@pytest.mark.parametrize("wmb,hmb", [(3, 2), (4, 3), (5, 3)], ids=["48x32", "64x48", "80x48"])
def test_block_fetch_equals_row_fetch(wmb, hmb, weights):
    from govideocompressor_amd.ops import native
    hip = native.hip()
    B, nmb, nref = 2, wmb * hmb, len(weights)
    p = _pictures(hip, B, wmb, hmb, nref)
    kno = _up(np.full((B, nmb), KNO, dtype=np.int32))
    dref_np = _dref_pattern(B, nmb) if nref > 1 else None
    dref = _up(dref_np) if nref > 1 else None
    dref0 = _up(np.maximum(dref_np, 0)) if nref > 1 else None
    seen, dists = set(), set()
    for t in range(NTABLES):
        dmv_np = _direct_vectors(B, wmb, hmb, t)
        _count_classes(dmv_np, wmb, hmb, seen, dists)
        dmv = _up(dmv_np)
        g_hdr, g_pred, g_cost = _general(hip, B, wmb, hmb, p, dmv, kno, kno, w1=weights, dref=dref).numpy()
        if nref > 1:  # the prediction of a quadrant without direct prediction: entry 0 (see above)
            g_pred = _general(hip, B, wmb, hmb, p, dmv, kno, kno, w1=weights, dref=dref0).numpy()[1]
        (_, pre_pred, pre_cost), o = _two_pass(hip, B, wmb, hmb, p, dmv, kno, kno, w1=weights, dref=dref)
        hdr, pred, cost = o.numpy()
        assert (g_pred != SENT).any() and (g_cost != S_COST).all()
        assert np.array_equal(pre_pred, g_pred), f"table {t}: pre-pass prediction"
        assert np.array_equal(pre_cost, g_cost), f"table {t}: pre-pass cost"
        assert np.array_equal(pred, g_pred) and np.array_equal(cost, g_cost), f"table {t}: main pass changed a gated MB"
        assert np.array_equal(hdr, g_hdr), f"table {t}: records"
        if nref > 1:
            una = (dref_np < 0).any(axis=2)
            assert una.any() and not una.all()
            assert (g_cost[una] == KNO).all() and (g_cost[~una] < KNO).all()
        else:
            assert (g_cost < KNO).all()
    missing = [(l, ph, c) for l in range(2) for ph in range(16) for c in CLASSES if (l, ph, c) not in seen]
    assert not missing, missing
    for l in range(2):
        for e in ("left", "right", "top", "bottom"):
            assert all((l, e, d) in dists for d in range(1, HP_MARGIN + 4)), (l, e)
        assert (l, "last8", "integer") in dists and (l, "last8", "half") in dists


# ---------------------------------------------------------------- 2. survivor loop against the general instance


def _survivors(name, nmb, slot):
    i = np.arange(nmb)
    if name == "none":
        return np.zeros(nmb, dtype=bool)
    if name == "all":
        return np.ones(nmb, dtype=bool)
    if name == "first":
        return i == 0
    if name == "last":
        return i == nmb - 1
    if name == "five":  # consecutive, across a group of four (and, from slot to slot, another place)
        lo = min(2 + 3 * slot, max(nmb - 5, 0))
        return (i >= lo) & (i < lo + 5)
    if name == "alternate":
        return (i + slot) % 2 == 0
    raise AssertionError(name)


_SURV = ["none", "all", "first", "last", "five", "alternate"]


def _list_costs(p, surv):
    c = np.where(surv[None], p["list_cost"], KNO).astype(np.int32)
    return _up(c[0]), _up(c[1])


def _moving_vectors(B, wmb, hmb):
    """Direct vectors for the survivor cases: table 5 of the block-fetch set (every class)."""
    return _up(_direct_vectors(B, wmb, hmb, 5))


@pytest.mark.parametrize("bparts", [0, 1])
@pytest.mark.parametrize("pattern", _SURV)
@pytest.mark.parametrize("wmb,hmb", [(3, 2), (5, 3), (11, 9)], ids=["48x32", "80x48", "176x144"])
def test_two_passes_equal_general_instance(wmb, hmb, pattern, bparts):
    from govideocompressor_amd.ops import native
    hip = native.hip()
    B, nmb = 2, wmb * hmb
    p = _pictures(hip, B, wmb, hmb)
    surv = np.stack([_survivors(pattern, nmb, b) for b in range(B)])
    c0, c1 = _list_costs(p, surv)
    dmv = _moving_vectors(B, wmb, hmb)
    g_hdr, g_pred, g_cost = _general(hip, B, wmb, hmb, p, dmv, c0, c1, bparts=bparts).numpy()
    _, o = _two_pass(hip, B, wmb, hmb, p, dmv, c0, c1, bparts=bparts)
    hdr, pred, cost = o.numpy()
    assert (g_hdr[..., 0][~surv] == 13).all()  # gated: B_Direct_16x16
    if surv.any():
        assert (g_hdr[..., 0][surv] != 13).any()  # the list costs are low enough to win somewhere
    assert np.array_equal(hdr, g_hdr)
    assert np.array_equal(pred, g_pred)
    assert np.array_equal(cost, g_cost)


def _route(kinds, l0, l1, w1):
    from govideocompressor_amd.models.h264_gpu import ROUTE_DTYPE
    rt = np.zeros(len(kinds), dtype=ROUTE_DTYPE)
    rt["kind"], rt["n0"], rt["l1"], rt["w1"], rt["dcopy"], rt["disp"] = kinds, 1, l1, w1, 1, -1
    rt["l0"] = l0
    return _up(rt.view(np.uint8).reshape(len(kinds), 32).copy())


@pytest.mark.parametrize("bparts", [0, 1])
def test_routed_two_passes_skip_other_slots(bparts):
    """Slot 0 codes a P picture this step: the pre-pass and the main pass leave its rows of every
    output alone.  Slot 1 codes a B picture between pool buffers 2 and 1 with an implicit weight."""
    import torch
    from govideocompressor_amd.ops import native
    hip = native.hip()
    B, wmb, hmb, nbuf = 2, 5, 3, 3
    nmb, W, H = wmb * hmb, wmb * 16, hmb * 16
    p = _pictures(hip, B, wmb, hmb)
    rng = np.random.default_rng(77)
    pool = _up(rng.integers(0, 256, size=(B, nbuf, H, W), dtype=np.uint8))
    hpp = torch.zeros((B, nbuf, 3, H + 8, W + 8), dtype=torch.uint8, device="cuda")
    hip.me_halfpel(B * nbuf, W, H, pool.data_ptr(), hpp.data_ptr(), torch.cuda.current_stream().cuda_stream)
    rt = _route([0, 1], [[0, -1, -1, -1], [2, -1, -1, -1]], [-1, 1], 27)
    surv = np.stack([_survivors("alternate", nmb, b) for b in range(B)])
    c0, c1 = _list_costs(p, surv)
    dmv = _moving_vectors(B, wmb, hmb)
    dref = _up(np.zeros((B, nmb, 4), dtype=np.int8))
    kw = dict(bparts=bparts, dref=dref, route=rt, nbuf=nbuf, pools=(pool, hpp))
    g = _general(hip, B, wmb, hmb, p, dmv, c0, c1, **kw).numpy()
    pre, o = _two_pass(hip, B, wmb, hmb, p, dmv, c0, c1, **kw)
    two = o.numpy()
    for outs in (g, pre, two):
        assert (outs[0][0] == SENT).all() and (outs[1][0] == SENT).all() and (outs[2][0] == S_COST).all()
    assert (g[2][1] != S_COST).all() and (g[0][1][:, 0] != SENT).all()
    for a_, b_ in zip(two, g):
        assert np.array_equal(a_[1], b_[1])
    # the routed launch read buffers 2 and 1 of slot 1 with weight 27: an unrouted launch on them agrees
    p1 = {k: (v[1:2].contiguous() if hasattr(v, "contiguous") else v) for k, v in p.items()}
    p1["refs"] = torch.stack([pool[1:2, 2], pool[1:2, 1]]).contiguous()
    p1["hp"] = torch.stack([hpp[1:2, 2], hpp[1:2, 1]]).contiguous()
    u = _general(hip, 1, wmb, hmb, p1, dmv[1:2].contiguous(), c0[1:2].contiguous(), c1[1:2].contiguous(),
                 bparts=bparts, w1=(27,)).numpy()
    for a_, b_ in zip(u, g):
        assert np.array_equal(a_[0], b_[1])


# ---------------------------------------------------------------- 3. end to end
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "b_block_fetch_parent.json")
with open(_GOLDEN) as _f:
    _DOC = json.load(_f)
_CASES = _DOC["cases"]


def clip(case, slots):
    """The synthetic clip of the case with three planted MBs per slot and frame t >= 1."""
    import torch
    from govideocompressor_amd.models.h264_gpu import synth_clip

    w, h = case["width"], case["height"]
    y, u, v = (p.cpu().numpy().copy() for p in synth_clip(slots, case["frames"], w, h, seed=case["seed"], kind=case["kind"]))
    rng = np.random.default_rng(2000 + case["seed"])
    wmb, hmb = w // 16, h // 16
    nmb = wmb * hmb
    tex = rng.integers(0, 256, (slots, 64, 64), dtype=np.uint8)
    for b in range(slots):
        for t in range(1, case["frames"]):
            mbs = [(3 * b + 1) % nmb, (nmb // 2 + b) % nmb, (nmb - 1 - 2 * b) % nmb]
            # a texture that moves 3 samples a frame inside a fixed MB
            mx, my = mbs[0] % wmb, mbs[0] // wmb
            o = (3 * t) % 40
            y[b, t, my * 16:my * 16 + 16, mx * 16:mx * 16 + 16] = tex[b, 8:24, o:o + 16]
            # the same over quadrants 0 and 3 only
            mx, my = mbs[1] % wmb, mbs[1] // wmb
            y[b, t, my * 16:my * 16 + 8, mx * 16:mx * 16 + 8] = tex[b, 32:40, o:o + 8]
            y[b, t, my * 16 + 8:my * 16 + 16, mx * 16 + 8:mx * 16 + 16] = tex[b, 40:48, o + 8:o + 16]
            # noise
            mx, my = mbs[2] % wmb, mbs[2] // wmb
            blk = y[b, t, my * 16:my * 16 + 16, mx * 16:mx * 16 + 16].astype(np.int16)
            y[b, t, my * 16:my * 16 + 16, mx * 16:mx * 16 + 16] = np.clip(blk + rng.integers(-50, 51, blk.shape), 0, 255).astype(np.uint8)
    return [torch.from_numpy(p).cuda() for p in (y, u, v)]


def b_stats(host, bitstreams):
    out = dict(direct=0, b8x8_direct=0)
    for seg in host.parse(list(bitstreams), 1):
        hdr = np.asarray(seg["hdr"])
        out["direct"] += int((hdr[:, :, 0] == 13).sum())
        out["b8x8_direct"] += int(((hdr[:, :, 0] == 12) & (hdr[:, :, 6] != 0)).sum())
    return out


def encode(case, slots):
    """-> (encoder, results, counts of the gate); the caller closes the encoder."""
    import torch
    from govideocompressor_amd.models.h264_gpu import GpuH264Encoder, H264Params
    from tools.record_inter_layout import _GateCounter

    enc = GpuH264Encoder(H264Params(width=case["width"], height=case["height"], **case["params"]), slots=slots)
    counter = _GateCounter(enc)
    enc.hip = counter
    y, u, v = clip(case, slots)
    res = enc.encode(y, u, v, keep_recon=True)
    torch.cuda.synchronize()
    return enc, res, {k: n for k, n in counter.counts.items() if k.startswith("b_")}


def test_cases_cover_the_configurations():
    assert _DOC["slots"] == 2
    ps = [c["params"] for c in _CASES]
    assert all(p["bframes"] == 3 for p in ps) and all(7 <= c["frames"] <= 9 for c in _CASES)
    assert all(48 <= c["width"] <= 176 and 48 <= c["height"] <= 144 for c in _CASES)
    assert any(p.get("direct", "temporal") == "temporal" and p["weightb"] for p in ps)
    assert any(p.get("refs") == 2 and p.get("pyramid") for p in ps)
    assert any(p.get("bpartitions") and p.get("partitions") for p in ps)
    assert any(p.get("direct") == "spatial" and not p.get("spatial_wavefront") for p in ps)
    assert any(p.get("direct") == "spatial" and p.get("spatial_wavefront") and p.get("spatial_gate") for p in ps)
    for c in _CASES:  # the recorded (parent) counts are not vacuous
        for key in c["need"]:
            assert c["counts"][key] > 0, (c["id"], key)
    assert any("b8x8_direct" in c["need"] for c in _CASES)


@pytest.mark.parametrize("case", _CASES, ids=[c["id"] for c in _CASES])
def test_b_decide_roundtrip_counts_and_parent_bytes(host, case):
    enc, res, counts = encode(case, _DOC["slots"])
    rec = enc.last_recon
    streams = [bytes(r.bitstream) for r in res]
    for b, r in enumerate(res):
        pics = host.decode(r.bitstream)
        assert len(pics) == r.frames == case["frames"]
        for t, pic in enumerate(pics):
            for k, name in enumerate(("y_coded", "u_coded", "v_coded")):
                assert np.array_equal(pic[name], rec[t][k][b].cpu().numpy()), f"slot {b} frame {t} plane {name}"
    enc.close()
    counts.update(b_stats(host, streams))
    print(case["id"], [len(s) for s in streams], counts)
    for key in case["need"]:
        assert counts[key] > 0, (key, counts)
    assert counts == case["counts"]
    assert [hashlib.sha256(s).hexdigest() for s in streams] == case["sha256"]
