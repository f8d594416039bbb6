"""The HEVC merge decision kernels (csrc/kernels/hevc_merge.hip: ``hevc_b_choose``,
``hevc_b_init_p``, ``hevc_b_merge``, ``hevc_merge_refine``) against the numpy model of
tests/ref_models_hevc_merge.py, one launch at a time through ``hip.hevc_b`` and
``hip.hevc_merge_refine``.

Everything these kernels compute is an exact integer: every output of every block of both slots
must equal the model, after every pass.  Output buffers are poisoned before each launch.  Inputs
are built in numpy from the seeds stated in the builders below: smooth random pictures, motion fields drawn
from a small palette (all 16 quarter phases, the zero vector, vectors reaching more than the
picture size outside the picture; equal neighbours are common, so every pruning rule occurs), a
source made per block of the prediction of one particular candidate plus noise (so that each kind
of candidate wins somewhere), search costs consistent with the model's SATD (cost = SATD + lambda *
bits), two slots at QP 22 and 37 and an AQ plane that drives lambda's QP into both clips.

What the cases are there for is asserted from the model's record (``test_coverage_*``), never
from the kernels' output.  Shapes in 16x16 blocks: 6x4 and 10x6 (waves of four blocks straddle
block rows, blocks on CTU edges of both CTU sizes) and 5x3 (15 blocks: the last wave has a dead
row; production pads pictures to the CTB and never launches it).
"""
import numpy as np
import pytest

import ref_models_hevc_merge as hm

pytestmark = pytest.mark.gpu

QP = (22, 37)
B = 2
P_MV, P_DIR, P_CHG, P_INT = -77, 0xA5, 0x5A, -5  # what output buffers hold before a launch
PASSES = 3


# ---------------------------------------------------------------------------- inputs

def _smooth(rng, H, W):
    base = rng.integers(0, 256, size=(H + 8, W + 8)).astype(np.float64)
    k = np.ones(5) / 5
    base = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 1, base)
    base = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 0, base)
    return np.ascontiguousarray(np.clip(base[4:-4, 4:-4] * 1.6 - 70, 0, 255).astype(np.uint8))


def _palette():
    """all 16 quarter phases around a few integer offsets, zero, and vectors far outside any picture here
    (at most 160x96 samples)"""
    v = [((4 * ((ph * 3) % 5 - 2)) + (ph & 3), (4 * ((ph * 7) % 5 - 2)) + (ph >> 2)) for ph in range(16)]
    assert {(x & 3, y & 3) for x, y in v} == {(a, b) for a in range(4) for b in range(4)}
    far = [(700, -450), (-2000, 1999), (3, 32767), (-32768, -5)]
    return v, far


def _draw_vec(rng):
    v, far = _palette()
    u = rng.random()
    if u < 0.18:
        return (0, 0)
    if u < 0.26:
        return far[rng.integers(len(far))]
    return v[rng.integers(len(v))]


def _field(rng, wmb, hmb, draw):
    """a motion per block: often the left or the upper neighbour's, else a fresh draw"""
    out = []
    for mb in range(wmb * hmb):
        mx, my = mb % wmb, mb // wmb
        u = rng.random()
        if mx > 0 and u < 0.4:
            out.append(out[mb - 1])
        elif my > 0 and 0.4 <= u < 0.6:
            out.append(out[mb - wmb])
        elif my > 0 and mx + 1 < wmb and 0.6 <= u < 0.68:
            out.append(out[mb - wmb + 1])
        else:
            out.append(draw(rng))
    return out


def _aq(rng, nmb):
    """slot 0 (QP 22) reaches below 0, slot 1 (QP 37) above 51"""
    aq = rng.integers(-9, 10, size=(B, nmb))
    aq[0, rng.random(nmb) < 0.2] = -30
    aq[1, rng.random(nmb) < 0.2] = 20
    aq = aq.astype(np.int8)
    q = np.array(QP)[:, None] + aq.astype(np.int64)
    assert (q < 0).any() and (q > 51).any() and (aq != 0).any()
    return aq


def _block(a, mb, wmb):
    X0, Y0 = (mb % wmb) * 16, (mb // wmb) * 16
    return a[Y0:Y0 + 16, X0:X0 + 16]


def _noisy(rng, pred, sd=1.5):
    return np.clip(np.rint(pred + rng.normal(0, sd, size=pred.shape)), 0, 255).astype(np.uint8)


_CACHE = {}


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


# ---------------------------------------------------------------------------- hevc_b_merge cases

# (shape, bslice, nref0, ctu64, max_merge, temporal, seed); seeds chosen on the CPU so that the coverage tests hold
def _merge_cases():
    out = []
    seed = 100
    for ctu64 in (0, 1):
        for mmg in (1, 2, 3, 5):
            for tmp in (0, 1):
                out.append(((10, 6), 1, 1, ctu64, mmg, tmp, seed))
                seed += 1
    for shape in ((6, 4), (5, 3)):
        for ctu64 in (0, 1):
            for mmg, tmp in ((5, 1), (2, 0)):
                out.append((shape, 1, 1, ctu64, mmg, tmp, seed))
                seed += 1
    for nref0 in (1, 3):
        for shape, ctu64, mmg, tmp in (((10, 6), 0, 5, 1), ((10, 6), 1, 3, 0), ((6, 4), 1, 5, 1), ((6, 4), 0, 2, 1),
                                       ((5, 3), 0, 5, 0)):
            out.append((shape, 0, nref0, ctu64, mmg, tmp, seed))
            seed += 1
    return out


_MERGE_CASES = _merge_cases()


def _merge_id(c):
    (w, h), bs, nr, c64, mmg, tmp, seed = c
    return f"{w}x{h}-{'B' if bs else 'P'}-ref{nr}-ctu{64 if c64 else 32}-max{mmg}-{'tmvp' if tmp else 'notmvp'}"


def _build_merge(case, lam_tab):
    """inputs of one case and the model's three chained passes per slot"""
    (wmb, hmb), bslice, nref0, ctu64, max_merge, temporal, seed = case
    rng = np.random.default_rng(seed)
    nmb, W, H = wmb * hmb, wmb * 16, hmb * 16
    sh = 2 if ctu64 else 1
    nl0 = nref0 if not bslice else 1
    refs0 = np.stack([np.stack([_smooth(rng, H, W) for _ in range(B)]) for _ in range(nl0)])  # [nl0, B, H, W]
    ref1 = np.stack([_smooth(rng, H, W) for _ in range(B)])
    aq = _aq(rng, nmb)

    def draw(rng):
        if bslice:
            d = int(rng.integers(1, 4))
        else:
            d = 1 | (int(rng.integers(0, nref0)) << 2)
        return hm.motion(d, _draw_vec(rng) + _draw_vec(rng))
    dirs = np.zeros((B, nmb), dtype=np.uint8)
    mvs = np.zeros((B, nmb, 4), dtype=np.int16)
    tdir = np.zeros((B, nmb), dtype=np.uint8)
    tmv = np.zeros((B, nmb, 4), dtype=np.int16)
    src = np.zeros((B, H, W), dtype=np.uint8)
    cost = np.zeros((B, nmb), dtype=np.int32)
    bits = np.zeros((B, nmb), dtype=np.int32)
    order = hm.coding_order(wmb, hmb, sh)
    slots = []
    for b in range(B):
        l0 = [hm.Pred(refs0[r, b]) for r in range(nl0)]
        l1 = hm.Pred(ref1[b]) if bslice else None
        lam = hm.lambdas(lam_tab, QP[b], aq[b])
        f = _field(rng, wmb, hmb, draw)
        dirs[b] = [m[0] for m in f]
        mvs[b] = [m[1:] for m in f]
        if temporal:
            tdir[b] = rng.choice([0, 1, 2, 3, 3], size=nmb)
            tmv[b] = [_draw_vec(rng) + _draw_vec(rng) for _ in range(nmb)]  # a P slice ignores the list-1 half
        # "chain": the motion planted for the left neighbour, which gets there a pass after that neighbour does
        plans = rng.choice(list(hm.SOURCES) + ["keep", "keep", "chain", "chain", "chain"], size=nmb)
        targets = []
        for mb in range(nmb):
            mx, my = mb % wmb, mb // wmb
            lst, srcs, _, _, _ = hm.block_merge_list(dirs[b], mvs[b], order, mx, my, tdir[b, mb] if temporal else None,
                                                     tmv[b, mb], bslice, max_merge, nref0)
            cur = hm.motion(dirs[b, mb], mvs[b, mb])
            target = lst[srcs.index(plans[mb])] if plans[mb] in srcs else cur
            if plans[mb] == "chain" and mx > 0:
                target = targets[mb - 1]
            targets.append(target)
            _block(src[b], mb, wmb)[:] = _noisy(rng, hm.predict(target, mx * 16, my * 16, l0, l1))
            bits[b, mb] = rng.integers(2, 24) if rng.random() < 0.8 else 1
            cost[b, mb] = hm.satd16(_block(src[b], mb, wmb), hm.predict(cur, mx * 16, my * 16, l0, l1)) + lam[mb] * bits[b, mb]
        d_, m_, c_, b_ = dirs[b].astype(np.int64), mvs[b].astype(np.int64), cost[b].astype(np.int64), bits[b].astype(np.int64)
        passes = []
        for _ in range(PASSES):
            out, rec = hm.b_merge_pass(src[b], l0, l1, d_, m_, c_, b_, lam, wmb, hmb, bslice, max_merge, sh,
                                       tdir[b] if temporal else None, tmv[b] if temporal else None, nref0)
            passes.append((out, rec))
            d_, m_, c_, b_ = out["dir"], out["mvb"], out["cost"], out["bits"]
        slots.append(passes)
    return dict(case=case, refs0=refs0, ref1=ref1, aq=aq, dirs=dirs, mvs=mvs, tdir=tdir, tmv=tmv, src=src, cost=cost,
                bits=bits, slots=slots)


def _merge_model(host, case):
    return _cached(("merge", case), lambda: _build_merge(case, host.table("lambda")[0]))


class _Dev:
    """uploads, half-sample planes and launches"""

    def __init__(self):
        import torch
        from govideocompressor_amd.ops import native
        self.torch, self.hip, self.dev = torch, native.hip(), torch.device("cuda")
        self.stream = torch.cuda.current_stream().cuda_stream

    def up(self, x):
        return self.torch.from_numpy(np.ascontiguousarray(x)).to(self.dev)

    def full(self, shape, value, dtype):
        return self.torch.full(shape, value, dtype=getattr(self.torch, dtype), device=self.dev)

    def planes(self, t_ref, W, H):
        n = t_ref.numel() // (W * H)
        hp = self.torch.zeros((n, 3, H + 8, W + 8), dtype=self.torch.uint8, device=self.dev)
        self.hip.me_halfpel(n, W, H, t_ref.data_ptr(), hp.data_ptr(), self.stream)
        return hp

    def sync(self):
        self.torch.cuda.synchronize()


def _np(t):
    return t.cpu().numpy().astype(np.int64)


def _run_merge(m, wired):
    """the three passes on the GPU, ping-ponging the motion buffers as models/hevc_gpu.py drives them;
    every output compared with the model after every pass"""
    (wmb, hmb), bslice, nref0, ctu64, max_merge, temporal, _ = m["case"]
    d = _Dev()
    nmb, W, H = wmb * hmb, wmb * 16, hmb * 16
    t_src = d.up(m["src"])
    t_refs = [d.up(m["refs0"][r]) for r in range(m["refs0"].shape[0])]
    t_hps = [d.planes(t, W, H) for t in t_refs]
    t_ref1 = d.up(m["ref1"])
    t_hp1 = d.planes(t_ref1, W, H)
    t_qp, t_aq = d.up(np.asarray(QP, dtype=np.int32)), d.up(m["aq"])
    t_tdir, t_tmv = d.up(m["tdir"]), d.up(m["tmv"])
    mvb = [d.up(m["mvs"]), d.full((B, nmb, 4), P_MV, "int16")]
    dirb = [d.up(m["dirs"]), d.full((B, nmb), P_DIR, "uint8")]
    cost, bits = d.up(m["cost"]), d.up(m["bits"])
    chg = [d.full((B, nmb), P_CHG, "uint8") for _ in range(2)]
    far = dict(nref0=nref0, xref=[t.data_ptr() for t in t_refs[1:]], xhp=[t.data_ptr() for t in t_hps[1:]]) if nref0 > 1 else {}
    for it in range(PASSES):
        i_, o_ = it % 2, (it + 1) % 2
        mvb[o_].fill_(P_MV)
        dirb[o_].fill_(P_DIR)
        ci, co = (0, 0)
        if wired:
            chg[it % 2].fill_(P_CHG)
            ci, co = (0 if it == 0 else chg[(it - 1) % 2].data_ptr()), chg[it % 2].data_ptr()
        d.hip.hevc_b(1, B, wmb, hmb, t_src.data_ptr(), t_refs[0].data_ptr(), t_ref1.data_ptr() if bslice else t_refs[0].data_ptr(),
                     t_hps[0].data_ptr(), t_hp1.data_ptr() if bslice else t_hps[0].data_ptr(), 0, 0, 0, 0, 0, 0,
                     t_tmv.data_ptr() if temporal else 0, t_tdir.data_ptr() if temporal else 0, mvb[i_].data_ptr(),
                     dirb[i_].data_ptr(), mvb[o_].data_ptr(), dirb[o_].data_ptr(), cost.data_ptr(), bits.data_ptr(),
                     t_qp.data_ptr(), t_aq.data_ptr(), d.stream, bslice, max_merge, ctu64, ci, co, **far)
        d.sync()
        g_mv, g_dir, g_cost, g_bits, g_chg = _np(mvb[o_]), _np(dirb[o_]), _np(cost), _np(bits), _np(chg[it % 2])
        for b in range(B):
            out, rec = m["slots"][b][it]
            bad = np.flatnonzero((g_mv[b] != out["mvb"]).any(axis=1) | (g_dir[b] != out["dir"]) | (g_cost[b] != out["cost"])
                                 | (g_bits[b] != out["bits"]))
            assert bad.size == 0, (f"pass {it} slot {b} blocks {bad[:6]}", g_mv[b][bad[:6]], out["mvb"][bad[:6]],
                                   g_dir[b][bad[:6]], out["dir"][bad[:6]], g_cost[b][bad[:6]], out["cost"][bad[:6]],
                                   g_bits[b][bad[:6]], out["bits"][bad[:6]], [rec[i]["sources"] for i in bad[:6]])
            if wired:
                assert np.array_equal(g_chg[b], out["chg"]), (it, b)
        if not wired:
            assert all((_np(c) == P_CHG).all() for c in chg)


@pytest.mark.parametrize("wired", [True, False], ids=["chg", "nochg"])
@pytest.mark.parametrize("case", _MERGE_CASES, ids=[_merge_id(c) for c in _MERGE_CASES])
def test_hevc_b_merge_three_passes(host, case, wired):
    """``wired``: chg_in / chg_out as the encoder wires them (pass 1 evaluates every block, later passes
    copy a block through when no flag is set nearby); otherwise both null.  The model re-evaluates
    every block every pass: that the shortcut changes nothing is part of what is checked."""
    _run_merge(_merge_model(host, case), wired)


def _merge_records(host, pick=lambda c: True):
    """(case, slot, pass, block index, record) of every block of the selected cases"""
    for case in _MERGE_CASES:
        if pick(case):
            m = _merge_model(host, case)
            for b in range(B):
                for it in range(PASSES):
                    for mb, r in enumerate(m["slots"][b][it][1]):
                        yield case, b, it, mb, r


def test_coverage_merge_lists_and_winners(host):
    seen, won, fired, kept, repriced, dups = set(), set(), set(), 0, 0, 0
    refidx_cand, refidx_zero = set(), set()
    for case, b, it, mb, r in _merge_records(host):
        seen.update(r["sources"])
        fired.update(r["fired"])
        dups += len(r["dups"])
        kept += r["kept"]
        repriced += r["repriced"]
        if r["moved"]:
            won.add(r["winner_source"])
        if not case[1] and case[2] == 3:
            for s, mo in zip(r["sources"], r["list"]):
                (refidx_zero if s == "Z" else refidx_cand).add(mo[0] >> 2)
    assert seen == set(hm.SOURCES), seen
    # each of spatial (every neighbour), temporal, combined and zero moves a block somewhere; the current motion
    # is kept somewhere, and re-priced (a candidate equal to it, at fewer bits) somewhere
    assert won == set(hm.SOURCES), won
    assert kept > 0 and repriced > 0 and dups > 0
    assert fired == set(hm.RULES), fired
    assert refidx_cand >= {0, 1, 2} and refidx_zero == {0, 1, 2}


def test_coverage_inputs(host):
    """what the motion fields are drawn from actually occurs in them"""
    dirs_b, phases, far, zero, refidx = set(), set(), 0, 0, set()
    for case in _MERGE_CASES:
        m = _merge_model(host, case)
        (wmb, hmb), bslice = case[0], case[1]
        d, v = m["dirs"].astype(np.int64), m["mvs"].astype(np.int64)
        (dirs_b if bslice else refidx).update((d if bslice else d >> 2).reshape(-1).tolist())
        for lst, bit in ((v[..., 0:2], 1), (v[..., 2:4], 2)):
            used = lst[(d & bit) != 0]
            phases.update(map(tuple, (used & 3).tolist()))
            zero += int((used == 0).all(axis=1).sum())
            # the whole block lies outside the picture, by more than the picture's size
            far += int(((np.abs(used[:, 0]) > 4 * 2 * wmb * 16) & (np.abs(used[:, 1]) > 4 * 2 * hmb * 16)).sum())
    assert dirs_b == {1, 2, 3} and refidx == {0, 1, 2}
    assert phases == {(a, b) for a in range(4) for b in range(4)}
    assert far > 0 and zero > 0


@pytest.mark.parametrize("ctu64", [0, 1])
def test_coverage_z_scan_refusals(host, ctu64):
    """B0 and A0 each refused by coding order while inside the picture (and each accepted somewhere)"""
    for k in ("B0", "A0"):
        refused = accepted = 0
        for case, b, it, mb, r in _merge_records(host, lambda c: c[3] == ctu64):
            refused += r["inpic"][k] and not r["avail"][k]
            accepted += r["avail"][k]
        assert refused > 0 and accepted > 0, k


def test_coverage_chg_shortcut_taken(host):
    """in passes 2 and 3 of a wired run some block has no changed flag nearby (it is copied through), and some has"""
    for it in (1, 2):
        quiet = busy = 0
        for case in _MERGE_CASES:
            m = _merge_model(host, case)
            (wmb, hmb) = case[0]
            for b in range(B):
                near = hm.chg_nearby(m["slots"][b][it - 1][0]["chg"], wmb, hmb)
                quiet += int((~near).sum())
                busy += int(near.sum())
                # the claim behind the shortcut, on the model alone: a quiet block does not move
                assert not m["slots"][b][it][0]["chg"][~near].any()
        assert quiet > 0 and busy > 0, (it, quiet, busy)


# ---------------------------------------------------------------------------- hevc_b_choose

_SHAPES = [(6, 4), (10, 6), (5, 3)]


def _build_choose(shape, lam_tab):
    wmb, hmb = shape
    rng = np.random.default_rng(300 + wmb)
    nmb, W, H = wmb * hmb, wmb * 16, hmb * 16
    ref0 = np.stack([_smooth(rng, H, W) for _ in range(B)])
    ref1 = np.stack([_smooth(rng, H, W) for _ in range(B)])
    aq = _aq(rng, nmb)
    mv0 = np.array([[_draw_vec(rng) for _ in range(nmb)] for _ in range(B)], dtype=np.int16)
    mv1 = np.array([[_draw_vec(rng) for _ in range(nmb)] for _ in range(B)], dtype=np.int16)
    delta = lambda: rng.integers(-6, 7, size=(B, nmb, 2)) * (rng.random((B, nmb, 1)) < 0.7)  # noqa: E731
    pm0 = np.clip(mv0.astype(np.int64) + delta(), -32768, 32767).astype(np.int16)
    pm1 = np.clip(mv1.astype(np.int64) + delta(), -32768, 32767).astype(np.int16)
    src = np.zeros((B, H, W), dtype=np.uint8)
    cost0 = np.zeros((B, nmb), dtype=np.int32)
    cost1 = np.zeros((B, nmb), dtype=np.int32)
    slots = []
    for b in range(B):
        p0, p1 = hm.Pred(ref0[b]), hm.Pred(ref1[b])
        lam = hm.lambdas(lam_tab, QP[b], aq[b])
        plans = rng.integers(0, 3, size=nmb)
        for mb in range(nmb):
            X0, Y0 = (mb % wmb) * 16, (mb // wmb) * 16
            a0, a1 = p0.block(X0, Y0, *mv0[b, mb]), p1.block(X0, Y0, *mv1[b, mb])
            S = _noisy(rng, (a0, a1, hm.bipred(a0, a1))[plans[mb]])
            _block(src[b], mb, wmb)[:] = S
            cost0[b, mb] = hm.satd16(S, a0) + lam[mb] * hm.mvd_bits(mv0[b, mb], pm0[b, mb])
            cost1[b, mb] = hm.satd16(S, a1) + lam[mb] * hm.mvd_bits(mv1[b, mb], pm1[b, mb])
        slots.append(hm.b_choose(src[b], p0, p1, mv0[b], mv1[b], cost0[b], cost1[b], pm0[b], pm1[b], lam, wmb, hmb))
    return dict(ref0=ref0, ref1=ref1, aq=aq, mv0=mv0, mv1=mv1, pm0=pm0, pm1=pm1, src=src, cost0=cost0, cost1=cost1, slots=slots)


@pytest.mark.parametrize("shape", _SHAPES, ids=["6x4", "10x6", "5x3"])
def test_hevc_b_choose(host, shape):
    wmb, hmb = shape
    nmb, W, H = wmb * hmb, wmb * 16, hmb * 16
    m = _cached(("choose", shape), lambda: _build_choose(shape, host.table("lambda")[0]))
    choices = {r["choice"] for _, rec in m["slots"] for r in rec}
    assert choices == {"L0", "L1", "bi"}
    d = _Dev()
    t = {k: d.up(m[k]) for k in ("src", "ref0", "ref1", "aq", "mv0", "mv1", "pm0", "pm1", "cost0", "cost1")}
    hp0, hp1 = d.planes(t["ref0"], W, H), d.planes(t["ref1"], W, H)
    t_qp = d.up(np.asarray(QP, dtype=np.int32))
    mvb, dirb = d.full((B, nmb, 4), P_MV, "int16"), d.full((B, nmb), P_DIR, "uint8")
    cost, bits = d.full((B, nmb), P_INT, "int32"), d.full((B, nmb), P_INT, "int32")
    p = lambda k: t[k].data_ptr()  # noqa: E731
    d.hip.hevc_b(0, B, wmb, hmb, p("src"), p("ref0"), p("ref1"), hp0.data_ptr(), hp1.data_ptr(), p("mv0"), p("mv1"),
                 p("cost0"), p("cost1"), p("pm0"), p("pm1"), 0, 0, 0, 0, mvb.data_ptr(), dirb.data_ptr(), cost.data_ptr(),
                 bits.data_ptr(), t_qp.data_ptr(), p("aq"), d.stream, 1, 5, 0)
    d.sync()
    for b in range(B):
        out, _ = m["slots"][b]
        assert np.array_equal(_np(dirb)[b], out["dir"]), b
        assert np.array_equal(_np(mvb)[b], out["mvb"]), b
        assert np.array_equal(_np(cost)[b], out["cost"]) and np.array_equal(_np(bits)[b], out["bits"]), b


# ---------------------------------------------------------------------------- hevc_b_init_p

def _build_init_p(shape, nref0, lam_tab):
    wmb, hmb = shape
    rng = np.random.default_rng(400 + 10 * wmb + nref0)
    nmb = wmb * hmb
    aq = _aq(rng, nmb)
    vec = lambda n: np.array([[[_draw_vec(rng) for _ in range(nmb)] for _ in range(B)] for _ in range(n)], dtype=np.int16)  # noqa: E731
    near = lambda v: np.clip(v.astype(np.int64) + rng.integers(-9, 10, size=v.shape) * (rng.random(v.shape[:-1] + (1,)) < 0.7),  # noqa: E731
                             -32768, 32767).astype(np.int16)
    mv0 = vec(1)[0]
    pm0 = near(mv0)
    cost0 = rng.integers(150, 4000, size=(B, nmb)).astype(np.int32)
    xmv = vec(max(nref0 - 1, 1))
    xpm = near(xmv)
    lam = np.stack([hm.lambdas(lam_tab, QP[b], aq[b]) for b in range(B)])
    # the farther searches: around the list-0[0] cost, within a few lambdas (so that the ref_idx bins decide
    # some), one below it (loses by the bins alone), or not searched
    u = rng.random((xmv.shape[0], B, nmb))
    xcost = cost0[None].astype(np.int64) + rng.integers(-4, 5, size=u.shape) * lam[None]
    xcost = np.where(u < 0.25, cost0[None].astype(np.int64) - 1, xcost)
    xcost = np.where(u > 0.8, hm.KNO, xcost).astype(np.int32)
    slots = [hm.b_init_p(mv0[b], cost0[b], pm0[b], lam[b], nref0, xmv[:, b], xcost[:, b], xpm[:, b]) for b in range(B)]
    return dict(aq=aq, mv0=mv0, pm0=pm0, cost0=cost0, xmv=xmv, xpm=xpm, xcost=xcost, slots=slots)


@pytest.mark.parametrize("nref0", [1, 3])
@pytest.mark.parametrize("shape", [(10, 6), (5, 3)], ids=["10x6", "5x3"])
def test_hevc_b_init_p(host, shape, nref0):
    wmb, hmb = shape
    nmb = wmb * hmb
    m = _cached(("init_p", shape, nref0), lambda: _build_init_p(shape, nref0, host.table("lambda")[0]))
    recs = [r for _, rec in m["slots"] for r in rec]
    if nref0 == 3:
        assert {r["ref"] for r in recs} == {0, 1, 2}                  # far searches win
        assert any(r["skipped"] for r in recs)                         # kNoCost entries
        assert any(r["ref"] == 0 and r["lost_to_bins"] for r in recs)  # cheaper before the bins, lost by them alone
    d = _Dev()
    t = {k: d.up(m[k]) for k in ("aq", "mv0", "pm0", "cost0", "xmv", "xpm", "xcost")}
    t_qp = d.up(np.asarray(QP, dtype=np.int32))
    dummy = d.full((3, B, 16, 16), 0, "uint8")  # the init pass reads no picture; the binding wants the pointers
    mvb, dirb = d.full((B, nmb, 4), P_MV, "int16"), d.full((B, nmb), P_DIR, "uint8")
    cost, bits = d.full((B, nmb), P_INT, "int32"), d.full((B, nmb), P_INT, "int32")
    p = lambda k: t[k].data_ptr()  # noqa: E731
    far = dict(nref0=3, xref=[dummy.data_ptr()] * 2, xhp=[dummy.data_ptr()] * 2, xmv=p("xmv"), xcost=p("xcost"),
               xpm=p("xpm")) if nref0 == 3 else {}
    d.hip.hevc_b(2, B, wmb, hmb, 0, 0, 0, 0, 0, p("mv0"), 0, p("cost0"), 0, p("pm0"), 0, 0, 0, 0, 0, mvb.data_ptr(),
                 dirb.data_ptr(), cost.data_ptr(), bits.data_ptr(), t_qp.data_ptr(), p("aq"), d.stream, 0, 5, 0, **far)
    d.sync()
    for b in range(B):
        out, _ = m["slots"][b]
        assert np.array_equal(_np(dirb)[b], out["dir"]), b
        assert np.array_equal(_np(mvb)[b], out["mvb"]), b
        assert np.array_equal(_np(cost)[b], out["cost"]) and np.array_equal(_np(bits)[b], out["bits"]), b


# ---------------------------------------------------------------------------- hevc_merge_refine

def _build_refine(shape, with_pm, lam_tab):
    wmb, hmb = shape
    rng = np.random.default_rng(500 + 10 * wmb + with_pm)
    nmb, W, H = wmb * hmb, wmb * 16, hmb * 16
    ref = np.stack([_smooth(rng, H, W) for _ in range(B)])
    aq = _aq(rng, nmb)
    mv = np.zeros((B, nmb, 2), dtype=np.int16)
    pm = np.zeros((B, nmb, 2), dtype=np.int16)
    src = np.zeros((B, H, W), dtype=np.uint8)
    cost = np.zeros((B, nmb), dtype=np.int32)
    slots = []
    for b in range(B):
        p = hm.Pred(ref[b])
        lam = hm.lambdas(lam_tab, QP[b], aq[b])
        mv[b] = _field(rng, wmb, hmb, _draw_vec)
        plans = rng.choice(list(hm.NEIGHBOURS) + ["Z", "keep", "keep", "keep"], size=nmb)
        # "twin" sites: the left neighbour a quarter sample off the block's vector, the upper one equal to it --
        # the left one can beat the search, and the search re-priced as the second candidate beat the left one
        twins = [mb for mb in range(wmb + 1, nmb, 7) if mb % wmb > 0]
        for mb in twins:
            mv[b, mb] = _palette()[0][rng.integers(16)]
            mv[b, mb - wmb] = mv[b, mb]
            mv[b, mb - 1] = mv[b, mb] + (1, 0)
            plans[mb] = "keep"
        if with_pm:
            # near the vector, or far from it: many mvd bits, so that the vector as a merge candidate is cheaper
            d_ = np.where(rng.random((nmb, 1)) < 0.5, rng.integers(-3, 4, size=(nmb, 2)), rng.integers(-300, 300, size=(nmb, 2)))
            d_[twins] = (-260, 170)
            pm[b] = np.clip(mv[b].astype(np.int64) + d_, -32768, 32767)
        for mb in range(nmb):
            mx, my = mb % wmb, mb // wmb
            pos = dict(hm.neighbour_positions(mx, my), Z=None)
            target = tuple(int(v) for v in mv[b, mb])
            if plans[mb] == "Z":
                target = (0, 0)
            elif plans[mb] != "keep":
                nx, ny = pos[plans[mb]]
                if 0 <= nx < wmb and 0 <= ny < hmb:
                    target = tuple(int(v) for v in mv[b, ny * wmb + nx])
            S = _noisy(rng, p.block(mx * 16, my * 16, *target), sd=3.0 if plans[mb] == "keep" else 1.5)
            _block(src[b], mb, wmb)[:] = S
            cost[b, mb] = hm.satd16(S, p.block(mx * 16, my * 16, *mv[b, mb])) + lam[mb] * hm.mvd_bits(mv[b, mb], pm[b, mb])
        v_, c_ = mv[b].astype(np.int64), cost[b].astype(np.int64)
        passes = []
        for _ in range(2):
            out, rec = hm.merge_refine_pass(src[b], p, v_, c_, pm[b] if with_pm else None, lam, wmb, hmb)
            passes.append((out, rec))
            v_, c_ = out["mv"], out["cost"]
        slots.append(passes)
    return dict(ref=ref, aq=aq, mv=mv, pm=pm, src=src, cost=cost, slots=slots)


def _refine_model(host, shape, with_pm):
    return _cached(("refine", shape, with_pm), lambda: _build_refine(shape, with_pm, host.table("lambda")[0]))


@pytest.mark.parametrize("with_pm", [1, 0], ids=["pm", "nopm"])
@pytest.mark.parametrize("shape", _SHAPES, ids=["6x4", "10x6", "5x3"])
def test_hevc_merge_refine_two_passes(host, shape, with_pm):
    """The documented neighbour-vector approximation, ``pm`` given and null.  (This comparison found the kernel
    keeping an earlier candidate's vector at the searched vector's merge price: ``took_back`` in the record.)"""
    wmb, hmb = shape
    nmb, W, H = wmb * hmb, wmb * 16, hmb * 16
    m = _refine_model(host, shape, with_pm)
    d = _Dev()
    t_src, t_ref, t_aq, t_pm = d.up(m["src"]), d.up(m["ref"]), d.up(m["aq"]), d.up(m["pm"])
    hp = d.planes(t_ref, W, H)
    t_qp = d.up(np.asarray(QP, dtype=np.int32))
    mvs = [d.up(m["mv"]), d.full((B, nmb, 2), P_MV, "int16")]
    cost = d.up(m["cost"])
    for it in range(2):
        a_, b_ = mvs[it % 2], mvs[(it + 1) % 2]
        b_.fill_(P_MV)
        d.hip.hevc_merge_refine(B, wmb, hmb, t_src.data_ptr(), t_ref.data_ptr(), hp.data_ptr(), a_.data_ptr(), b_.data_ptr(),
                                cost.data_ptr(), t_pm.data_ptr() if with_pm else 0, t_qp.data_ptr(), t_aq.data_ptr(), d.stream)
        d.sync()
        g_mv, g_cost = _np(b_), _np(cost)
        for b in range(B):
            out, rec = m["slots"][b][it]
            bad = np.flatnonzero((g_mv[b] != out["mv"]).any(axis=1) | (g_cost[b] != out["cost"]))
            assert bad.size == 0, (f"pass {it} slot {b} blocks {bad[:6]}", g_mv[b][bad[:6]], out["mv"][bad[:6]],
                                   g_cost[b][bad[:6]], out["cost"][bad[:6]], [rec[i] for i in bad[:3]])


def test_coverage_merge_refine(host):
    won, seen = set(), set()
    repriced = took_back = kept = 0
    for shape in _SHAPES:
        for with_pm in (1, 0):
            m = _refine_model(host, shape, with_pm)
            for b in range(B):
                for out, rec in m["slots"][b]:
                    for r in rec:
                        seen.update(r["sources"])
                        won.add(r["winner_source"])
                        repriced += r["repriced"]
                        took_back += r["took_back"]
                        kept += r["kept"] and not r["repriced"]
    assert seen == set(hm.NEIGHBOURS) | {"Z"}
    assert won == set(hm.NEIGHBOURS) | {"Z", None}
    # the searched vector is itself a candidate and is re-priced as merge; also after an earlier candidate had
    # already beaten the search (the block then keeps the searched vector at the merge price)
    assert repriced > 0 and took_back > 0 and kept > 0
