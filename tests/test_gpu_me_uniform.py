"""The 16x16 motion search (``hip.me``) against the numpy model of tests/ref_models_me.py, at the
shapes where keeping its wave-uniform work on the scalar unit can go wrong (csrc/kernels/me_search.h).

The search takes one path when everything a phase reads lies inside the picture (the candidate
blocks, the reference window, the four sub-sample plane regions: one scalar test each, no clamps,
lane offsets from a scalar base) and the clamping path otherwise; vectors, costs and centres live
in scalar registers.  Every output must equal the model exactly: vector, cost, the 256 prediction
bytes, the intra estimate, and ``kNoCost`` where the gate closes.  What a case is there for is
asserted from the model's own record of it (window origins, alignments, early exits), so no case
passes vacuously.
"""
import numpy as np
import pytest

import ref_models_me as mm

pytestmark = pytest.mark.gpu

KNO = mm.KNO
P_MV, P_COST, P_PRED, P_INTRA = -77, -5, 0xA5, -6  # what the output buffers hold before a launch


def _pictures(seed, W, H, dy=3, dx=-2, noise=2.0):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(H + 40, W + 40)).astype(np.float64)
    k = np.ones(5) / 5
    base = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 1, base)
    base = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 0, base)
    ref = base[10:10 + H, 12:12 + W]
    src = base[10 + dy:10 + dy + H, 12 + dx:12 + dx + W] + rng.normal(0, noise, size=(H, W))
    return (np.ascontiguousarray(np.clip(src, 0, 255).astype(np.uint8)),
            np.ascontiguousarray(np.clip(ref, 0, 255).astype(np.uint8)))


def _launch(B, wmb, hmb, src, ref, pred, qp, R, seed_mv=None, cost_mv=None, aq=None, early_sad=0, with_intra=True,
            gate=None, gate_thresh=0, route=None, nbuf=0, role=0, want=0, hp=None):
    """-> mv [B, nmb, 2], cost [B, nmb], pred [B, nmb, 256], intra [B, nmb]; buffers poisoned first.
    ``ref``: [B, H, W], or the pool of a routed launch (a device tensor, with ``hp`` its planes)."""
    import torch
    from govideocompressor_amd.ops import native
    hip = native.hip()
    dev = torch.device("cuda")
    nmb = wmb * hmb
    up = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    t_src, t_pred, t_seed, t_cmv, t_aq, t_gate = up(src), up(pred), up(seed_mv), up(cost_mv), up(aq), up(gate)
    t_ref = ref if hasattr(ref, "data_ptr") else up(ref)
    t_qp = up(np.asarray(qp, dtype=np.int32))
    mv = torch.full((B, nmb, 2), P_MV, dtype=torch.int16, device=dev)
    cost = torch.full((B, nmb), P_COST, dtype=torch.int32, device=dev)
    outp = torch.full((B, nmb, 256), P_PRED, dtype=torch.uint8, device=dev)
    intra = torch.full((B, nmb), P_INTRA, dtype=torch.int32, device=dev)
    hip.me(B, wmb, hmb, t_src.data_ptr(), t_ref.data_ptr(), ptr(t_pred), mv.data_ptr(), cost.data_ptr(), outp.data_ptr(),
           intra.data_ptr() if with_intra else 0, t_qp.data_ptr(), R, 2, torch.cuda.current_stream().cuda_stream,
           hp=ptr(hp), aq=ptr(t_aq), planes_ready=1 if hp is not None else 0, early_sad=early_sad, gate_cost=ptr(t_gate),
           gate_thresh=gate_thresh, cost_mv=ptr(t_cmv), route=ptr(route), nbuf=nbuf, role=role, want=want,
           seed_mv=ptr(t_seed))
    torch.cuda.synchronize()
    return mv.cpu().numpy(), cost.cpu().numpy(), outp.cpu().numpy(), intra.cpu().numpy()


def _assert_slot(got, b, m, with_intra=True):
    """slot b of a launch's outputs against the model m of that slot"""
    mv, cost, pred, intra = (x[b] for x in got)
    s = m["searched"]
    bad = np.flatnonzero((mv[s] != m["mv"][s]).any(axis=1) | (cost[s] != m["cost"][s]))
    assert bad.size == 0, (np.flatnonzero(s)[bad][:8], mv[s][bad][:8], m["mv"][s][bad][:8], cost[s][bad][:8], m["cost"][s][bad][:8])
    assert np.array_equal(pred[s].astype(np.int64), m["pred"][s])
    g = ~s
    assert (cost[g] == KNO).all() and (mv[g] == P_MV).all() and (pred[g] == P_PRED).all()
    if with_intra:
        assert np.array_equal(intra, m["intra"])  # kNoCost where the gate closes
    else:
        assert (intra == P_INTRA).all()


def _window_inside(m, W, H, R):
    """the search's own test: every aligned word of an MB's window inside the picture"""
    rows = 16 + 2 * R + 10
    words = (rows + 3) // 4 + 1
    xa = m["window"][:, 0] & ~3
    return (xa >= 0) & (xa + 4 * words <= W) & (m["window"][:, 1] >= 0) & (m["window"][:, 1] + rows <= H)


_MODELS = {}


def _model(host, key, *a, **kw):
    if key not in _MODELS:
        _MODELS[key] = mm.me_search(*a, host.table("lambda")[0], **kw)
    return _MODELS[key]


def test_seam_between_interior_and_edge_80x80(host):
    """5x5 MBs, radius 8, zero predictors: the six MBs (1..2, 1..3) have their 48-byte x 42-row
    windows wholly inside (12 samples to the left / above the MB, 36 / 30 to the right / below its
    origin), every MB around them touches an edge; both paths next to each other.  The sub-sample
    plane regions and the candidate blocks have their own, wider interiors."""
    wmb = hmb = 5
    src, ref = _pictures(11, 80, 80)
    pred = np.zeros((25, 2), dtype=np.int16)
    m = _model(host, "80x80", src, ref, pred, 27, 8, wmb=wmb, hmb=hmb)
    inside = _window_inside(m, 80, 80, 8)
    assert np.array_equal(np.flatnonzero(inside), [6, 7, 11, 12, 16, 17])
    _assert_slot(_launch(1, wmb, hmb, src[None], ref[None], pred[None], [27], 8), 0, m)


@pytest.mark.parametrize("dx,dy", [(-1, 0), (1, 0), (0, -1), (0, 1)])
def test_candidate_blocks_one_sample_outside_80x80(host, dx, dy):
    """The candidate blocks' inside test at its edge.  The picture moves by one sample and every
    predictor says so: the candidate blocks of the MBs along one picture edge reach one sample
    outside, those of all other MBs lie inside.  Every MB ends early on its predictor: the
    candidates' SADs alone decide, and unlike the window, whose margins the integer search never
    reads, every byte of a candidate block counts.  The picture is a ramp from 0 to 255 along
    the motion with a little texture, so a sample taken from the far end of a neighbouring row
    instead of the replicated edge costs the predictor about 4,000 of SAD against the 800 by
    which it beats the zero vector, and the choice flips."""
    wmb = hmb = 5
    rng = np.random.default_rng(13)
    ax = np.arange(-1, 81) * 255.0 / 79
    base = (np.tile(ax, (82, 1)) if dx else np.tile(ax[:, None], (1, 82))) + rng.normal(0, 3, size=(82, 82))
    ref = np.ascontiguousarray(np.clip(base[1:81, 1:81], 0, 255).astype(np.uint8))
    src = np.ascontiguousarray(np.clip(base[1 + dy:81 + dy, 1 + dx:81 + dx] + rng.normal(0, 1, size=(80, 80)), 0, 255)
                               .astype(np.uint8))
    pred = np.tile(np.array([4 * dx, 4 * dy], dtype=np.int16), (25, 1))
    m = _model(host, ("80x80-cand", dx, dy), src, ref, pred, 27, 8, wmb=wmb, hmb=hmb, early_sad=1 << 20)
    assert m["early"].all() and (m["centre"] == (dx, dy)).all()
    _assert_slot(_launch(1, wmb, hmb, src[None], ref[None], pred[None], [27], 8, early_sad=1 << 20), 0, m)


def test_radius_16_instance_112x112(host):
    """search range 16 (the other kernel instance): 112x112 is the smallest picture in which an
    MB of it could have its window inside (16 + 32 + 10 rows)."""
    wmb = hmb = 7
    src, ref = _pictures(12, 112, 112, dy=-5, dx=9)
    pred = np.random.default_rng(12).integers(-12, 12, size=(49, 2)).astype(np.int16)
    m = _model(host, "112x112", src, ref, pred, 30, 16, wmb=wmb, hmb=hmb)
    inside = _window_inside(m, 112, 112, 16)
    assert inside.any() and not inside.all()
    _assert_slot(_launch(1, wmb, hmb, src[None], ref[None], pred[None], [30], 16), 0, m)


def _qcif_predictors(seed):
    """99 MBs: mostly a few samples, every tenth one far out (past the +-128 sample clamp)"""
    rng = np.random.default_rng(seed)
    pred = rng.integers(-48, 48, size=(99, 2)).astype(np.int16)
    far = np.arange(99) % 10 == 3
    pred[far] = rng.choice([-2000, -700, -560, 540, 900, 2040], size=(int(far.sum()), 2))
    return pred


@pytest.mark.parametrize("R", [8, 4, 2, 6])
def test_alignments_clamps_and_zero_outside_176x144(host, R):
    """Radius 8 and 4 (the compile-time searches) and 2 and 6 (the generic one).  The predictors
    put the window at all four byte alignments, reach past +-128 samples (the clamp, and windows
    wholly outside the picture) and leave the zero vector outside the window."""
    wmb, hmb = 11, 9
    src, ref = _pictures(20 + R, 176, 144)
    # (seeds under which, at radius 8 and 4, windows sit one word outside the interior test)
    pred = _qcif_predictors({8: 18, 4: 134}.get(R, R))
    m = _model(host, ("qcif", R), src, ref, pred, 27, R, wmb=wmb, hmb=hmb)
    if R in (8, 4):
        # the seam of the window's inside test from the outside: one word too far left, one too
        # far right (rows inside), and rows above the picture (columns inside)
        rows = 16 + 2 * R + 10
        words = (rows + 3) // 4 + 1
        xa, wy = m["window"][:, 0] & ~3, m["window"][:, 1]
        assert ((xa == -4) & (wy >= 1) & (wy + rows <= 144)).any()
        assert ((xa + 4 * words == 176 + 4) & (wy >= 0) & (wy + rows <= 143)).any()
        assert ((xa >= 0) & (xa + 4 * words <= 176) & (wy < 0)).any()
    assert set((m["window"][:, 0] & 3).tolist()) == {0, 1, 2, 3}
    assert (np.abs(pred.astype(np.int64)) > 512).any() and (np.abs(m["centre"]) == 128).any()
    assert ((m["window"][:, 0] >= 176) | (m["window"][:, 0] + 64 <= 0)).any()  # a window wholly outside
    assert m["zero_outside"].any() and not m["zero_outside"].all()
    inside = _window_inside(m, 176, 144, R)
    assert inside.any() and not inside.all()
    _assert_slot(_launch(1, wmb, hmb, src[None], ref[None], pred[None], [27], R), 0, m)


def _qcif_options():
    rng = np.random.default_rng(31)
    return dict(seed_mv=rng.integers(-60, 60, size=(99, 2)).astype(np.int16),
                cost_mv=rng.integers(-20, 20, size=(99, 2)).astype(np.int16),
                aq=rng.integers(-6, 7, size=99).astype(np.int8))


@pytest.mark.parametrize("case", ["seed", "cost_mv", "aq", "early", "nointra", "all"])
def test_flags_and_options_176x144(host, case):
    wmb, hmb = 11, 9
    src, ref = _pictures(32, 176, 144, noise=6.0)
    pred = _qcif_predictors(32)
    o = _qcif_options()
    kw = dict()
    if case in ("seed", "all"):
        kw["seed_mv"] = o["seed_mv"]
    if case in ("cost_mv", "all"):
        kw["cost_mv"] = o["cost_mv"]
    if case in ("aq", "early", "all"):
        kw["aq"] = o["aq"]
    if case in ("early", "all"):
        # the median SAD of the chosen centres without early exit: about half of the MBs end early
        base = _model(host, ("opt-base", case), src, ref, pred, 27, 8, wmb=wmb, hmb=hmb,
                      **{k: v for k, v in kw.items()})
        kw["early_sad"] = int(np.median(base["best_sad"]))
    if case in ("nointra", "all"):
        kw["with_intra"] = False
    m = _model(host, ("opt", case), src, ref, pred, 27, 8, wmb=wmb, hmb=hmb, **kw)
    if "aq" in kw:
        lam = np.asarray(host.table("lambda")[0])[np.clip(27 + o["aq"].astype(np.int64), 0, 51)]
        assert (lam[1:] != lam[:-1]).mean() > 0.5  # neighbouring MBs with different lambdas
    if "early_sad" in kw:
        share = m["early"].mean()
        assert 0.1 <= share <= 0.9, share
    if "seed_mv" in kw:  # the seed wins somewhere: its candidate is not dead weight
        seed_c = np.clip((o["seed_mv"].astype(np.int64) + 2) >> 2, -128, 128)
        assert (m["centre"] == seed_c).all(axis=1).any()
    got = _launch(1, wmb, hmb, src[None], ref[None], pred[None], [27], 8,
                  **{k: (v[None] if isinstance(v, np.ndarray) else v) for k, v in kw.items()})
    _assert_slot(got, 0, m, with_intra=kw.get("with_intra", True))


def _route(kinds, n0, l0, l1):
    import torch
    from govideocompressor_amd.models.h264_gpu import ROUTE_DTYPE
    rt = np.zeros(len(kinds), dtype=ROUTE_DTYPE)
    rt["kind"], rt["n0"], rt["l1"], rt["w1"], rt["dcopy"], rt["disp"] = kinds, n0, l1, 32, 1, -1
    rt["l0"] = l0
    return torch.from_numpy(rt.view(np.uint8).reshape(len(kinds), 32).copy()).to("cuda")


def test_three_slots_middle_routed_away(host):
    """A routed launch over P slots: slot 1 codes a B picture and keeps every poisoned byte; slots
    0 and 2 search the pool buffers their routes name (2 and 1)."""
    import torch
    from govideocompressor_amd.ops import native
    hip = native.hip()
    B, wmb, hmb, nbuf = 3, 5, 5, 3
    W = H = 80
    pics = [_pictures(40 + b, W, H, dy=2 - b, dx=b) for b in range(B)]
    src = np.stack([p[0] for p in pics])
    pool = np.stack([np.stack([_pictures(50 + 3 * b + k, W, H)[1] for k in range(nbuf)]) for b in range(B)])
    use = [2, 0, 1]
    for b in range(B):
        pool[b, use[b]] = pics[b][1]
    pred = np.random.default_rng(41).integers(-24, 24, size=(B, 25, 2)).astype(np.int16)
    qp = [24, 27, 33]
    t_pool = torch.from_numpy(np.ascontiguousarray(pool)).to("cuda")
    hp = torch.zeros((B, nbuf, 3, H + 8, W + 8), dtype=torch.uint8, device="cuda")
    hip.me_halfpel(B * nbuf, W, H, t_pool.data_ptr(), hp.data_ptr(), torch.cuda.current_stream().cuda_stream)
    rt = _route([0, 1, 0], [1, 1, 1], [[use[0], -1, -1, -1], [use[1], -1, -1, -1], [use[2], -1, -1, -1]], [-1, 1, -1])
    got = _launch(B, wmb, hmb, src, t_pool, pred, qp, 8, route=rt, nbuf=nbuf, role=0, want=0, hp=hp)
    mv, cost, outp, intra = got
    assert (mv[1] == P_MV).all() and (cost[1] == P_COST).all() and (outp[1] == P_PRED).all() and (intra[1] == P_INTRA).all()
    for b in (0, 2):
        m = _model(host, ("route", b), src[b], pool[b, use[b]], pred[b], qp[b], 8, wmb=wmb, hmb=hmb)
        _assert_slot(got, b, m)


def _gate_case(host, surv, with_intra, thresh):
    """80x80: 25 MBs are four runs of 8, the last with one MB"""
    wmb = hmb = 5
    src, ref = _pictures(11, 80, 80)
    pred = np.random.default_rng(61).integers(-24, 24, size=(25, 2)).astype(np.int16)
    aq = np.random.default_rng(62).integers(-6, 7, size=25).astype(np.int8)
    lam = np.asarray(host.table("lambda")[0])[np.clip(27 + aq.astype(np.int64), 0, 51)].astype(np.int64)
    thr = np.full(25, thresh, dtype=np.int64) if thresh >= 0 else -thresh * lam
    gate = (thr + surv).astype(np.int32)  # on the threshold: stopped; one above: searched
    m = mm.me_search(src, ref, pred, 27, 8, host.table("lambda")[0], wmb, hmb, aq=aq, with_intra=with_intra,
                     gate_cost=gate, gate_thresh=thresh)
    assert np.array_equal(m["searched"], surv)
    got = _launch(1, wmb, hmb, src[None], ref[None], pred[None], [27], 8, aq=aq[None], with_intra=with_intra,
                  gate=gate[None], gate_thresh=thresh)
    _assert_slot(got, 0, m, with_intra=with_intra)


@pytest.mark.parametrize("with_intra", [True, False], ids=["intra", "nointra"])
@pytest.mark.parametrize("thresh", [2400, -150])
def test_gated_launch_runs_80x80(host, thresh, with_intra):
    """Survivors at positions 0 and 7 of a run (two in one run), a run with none, one in the
    middle of a run, and the one-MB last run."""
    surv = np.zeros(25, dtype=bool)
    surv[[0, 7, 19, 24]] = True
    _gate_case(host, surv, with_intra, thresh)


def test_gated_launch_without_survivors(host):
    _gate_case(host, np.zeros(25, dtype=bool), True, 2400)
