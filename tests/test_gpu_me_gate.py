"""Gated launches of the motion search (``hip.me`` with ``gate_cost``) and ``me_ref_select``.

A gated launch runs one wave per run of consecutive MBs of a slot: a lane per MB tests the gate,
the wave searches the survivors in turn.  Every case here is the gated launch against the ungated
one on the same inputs (the ungated instance is pinned to numpy by
``test_gpu_me_golden.py::test_me_matches_numpy_reference``): an MB at or below the gate gets
``out_cost = kNoCost`` (``out_intra`` likewise when passed) and nothing else, every other MB
equals the ungated search bit for bit.  Gate costs sit exactly on the threshold (gated) or one
above it (searched), so the threshold arithmetic (``gate_thresh < 0``: lambdas of the MB's own QP)
is part of the check.  Shapes: 15 MBs (one partial run), 72 MBs (crosses 64, partial tail), two
slots with different patterns (a run must not leak into the next slot).

``me_ref_select`` (a lane per MB, a wave per 64 MBs) is checked against a numpy statement of
its rule."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KNO = 0x3FFFFFFF
S_MV, S_COST, S_PRED, S_INTRA = -77, -5, 0xA5, -6


def _smooth(rng, H, W, dy, dx, noise):
    base = rng.integers(0, 256, size=(H + 40, W + 40)).astype(np.float64)
    k = np.ones(5) / 5
    base = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 1, base)
    base = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 0, base)
    ref = base[10:10 + H, 12:12 + W]
    src = base[10 + dy:10 + dy + H, 12 + dx:12 + dx + W] + rng.normal(0, noise, size=(H, W))
    return (np.ascontiguousarray(np.clip(src, 0, 255).astype(np.uint8)),
            np.ascontiguousarray(np.clip(ref, 0, 255).astype(np.uint8)))


_INPUTS = {}


def _inputs(B, wmb, hmb):
    """Pictures, vectors and AQ offsets of a shape, made once."""
    key = (B, wmb, hmb)
    if key not in _INPUTS:
        rng = np.random.default_rng(100 * wmb + hmb + B)
        nmb, W, H = wmb * hmb, wmb * 16, hmb * 16
        pics = [_smooth(rng, H, W, 3 - 2 * b, -2 + 3 * b, 2.0) for b in range(B)]
        _INPUTS[key] = dict(
            src=np.stack([p[0] for p in pics]), ref=np.stack([p[1] for p in pics]),
            pred=rng.integers(-24, 24, size=(B, nmb, 2)).astype(np.int16),
            cost_mv=rng.integers(-16, 16, size=(B, nmb, 2)).astype(np.int16),
            seed_mv=rng.integers(-40, 40, size=(B, nmb, 2)).astype(np.int16),
            aq=rng.integers(-6, 7, size=(B, nmb)).astype(np.int8),
            qp=np.array([27, 31][:B], dtype=np.int32))
    return _INPUTS[key]


def _pattern(name, nmb, slot):
    """True = the MB survives the gate (is searched)."""
    i = np.arange(nmb)
    if name == "all_gated":
        return np.zeros(nmb, dtype=bool)
    if name == "none_gated":
        return np.ones(nmb, dtype=bool)
    if name == "checker":
        return (i + slot) % 2 == 0
    if name == "first":
        return i == 0
    if name == "last":
        return i == nmb - 1
    if name == "run_then_empty":  # whole runs survive next to empty ones, for every run length up to 64
        return (i < 64) if nmb > 64 else (i < 8)
    if name == "empty_then_run":
        return (i >= 64) if nmb > 64 else (i >= 8)
    if name == "mixed":  # slot 0 and slot 1 differ: a run must not take the next slot's gate
        return (i % 3 == 0) if slot == 0 else (i % 5 != 0)
    raise AssertionError(name)


def _launch(hip, B, wmb, hmb, d, gate, gate_thresh, R, with_intra, early_sad, use_aq, use_cost_mv, use_seed,
            route=None, nbuf=0, role=0, want=0, ref_pool=None, hp_pool=None):
    import torch
    dev = torch.device("cuda")
    s = torch.cuda.current_stream().cuda_stream
    nmb = wmb * hmb
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items()}
    mv = torch.full((B, nmb, 2), S_MV, dtype=torch.int16, device=dev)
    cost = torch.full((B, nmb), S_COST, dtype=torch.int32, device=dev)
    pred = torch.full((B, nmb, 256), S_PRED, dtype=torch.uint8, device=dev)
    intra = torch.full((B, nmb), S_INTRA, dtype=torch.int32, device=dev)
    tg = torch.from_numpy(gate).to(dev) if gate is not None else None
    ref = ref_pool if ref_pool is not None else t["ref"]
    hip.me(B, wmb, hmb, t["src"].data_ptr(), ref.data_ptr(), t["pred"].data_ptr(), mv.data_ptr(), cost.data_ptr(),
           pred.data_ptr(), intra.data_ptr() if with_intra else 0, t["qp"].data_ptr(), R, 2, s,
           hp=hp_pool.data_ptr() if hp_pool is not None else 0, aq=t["aq"].data_ptr() if use_aq else 0,
           planes_ready=1 if hp_pool is not None else 0, early_sad=early_sad,
           gate_cost=tg.data_ptr() if tg is not None else 0, gate_thresh=gate_thresh,
           cost_mv=t["cost_mv"].data_ptr() if use_cost_mv else 0, route=route.data_ptr() if route is not None else 0,
           nbuf=nbuf, role=role, want=want, seed_mv=t["seed_mv"].data_ptr() if use_seed else 0)
    torch.cuda.synchronize()
    return mv.cpu().numpy(), cost.cpu().numpy(), pred.cpu().numpy(), intra.cpu().numpy()


def _gate_costs(host, d, surv, gate_thresh, use_aq):
    """Exactly the threshold for gated MBs, one above it for survivors."""
    lam = np.asarray(host.table("lambda")[0])
    qp = np.clip(d["qp"][:, None] + (d["aq"].astype(np.int32) if use_aq else 0), 0, 51)
    thr = np.full(surv.shape, gate_thresh, dtype=np.int64) if gate_thresh >= 0 else -gate_thresh * lam[qp].astype(np.int64)
    return np.ascontiguousarray((thr + surv).astype(np.int32))


_UNGATED = {}


def _check(host, B, wmb, hmb, pattern, gate_thresh=2400, R=8, with_intra=True, early_sad=0, use_aq=False,
           use_cost_mv=False, use_seed=False):
    from govideocompressor_amd.ops import native
    hip = native.hip()
    nmb = wmb * hmb
    d = _inputs(B, wmb, hmb)
    opts = (R, with_intra, early_sad, use_aq, use_cost_mv, use_seed)
    ukey = (B, wmb, hmb) + opts
    if ukey not in _UNGATED:  # the reference of every pattern at these options, computed once
        _UNGATED[ukey] = _launch(hip, B, wmb, hmb, d, None, 0, *opts)
    umv, ucost, upred, uintra = _UNGATED[ukey]
    assert (ucost != S_COST).all() and (ucost < KNO).all() and (umv != S_MV).any()
    surv = np.stack([_pattern(pattern, nmb, b) for b in range(B)])
    gate = _gate_costs(host, d, surv, gate_thresh, use_aq)
    mv, cost, pred, intra = _launch(hip, B, wmb, hmb, d, gate, gate_thresh, *opts)
    g = ~surv
    assert (cost[g] == KNO).all()
    assert (mv[g] == S_MV).all() and (pred[g] == S_PRED).all()
    assert (intra[g] == (KNO if with_intra else S_INTRA)).all()
    assert np.array_equal(cost[surv], ucost[surv])
    assert np.array_equal(mv[surv], umv[surv])
    assert np.array_equal(pred[surv], upred[surv])
    assert np.array_equal(intra[surv], uintra[surv])
    if not with_intra:
        assert (intra == S_INTRA).all()


_PATTERNS = ["all_gated", "none_gated", "checker", "first", "last", "run_then_empty", "empty_then_run"]


@pytest.mark.parametrize("pattern", _PATTERNS)
@pytest.mark.parametrize("shape", [(1, 5, 3), (1, 9, 8), (2, 9, 8)], ids=["5x3", "9x8", "2x9x8"])
def test_gated_search_equals_ungated(host, shape, pattern):
    _check(host, *shape, pattern)


@pytest.mark.parametrize("shape", [(2, 5, 3), (2, 9, 8)], ids=["2x5x3", "2x9x8"])
def test_gated_search_slots_keep_their_own_gate(host, shape):
    _check(host, *shape, "mixed")


@pytest.mark.parametrize("opts", [
    dict(gate_thresh=-150, use_aq=True),                       # lambdas of each MB's own QP inside a run
    dict(gate_thresh=-150, use_aq=True, R=4, with_intra=False),
    dict(gate_thresh=3000, R=4, early_sad=1024, use_seed=True),
    dict(gate_thresh=3000, R=4, use_cost_mv=True, with_intra=False, use_aq=True),
    dict(gate_thresh=2400, R=16),                              # the radius-16 instance
    dict(gate_thresh=-150, R=16, use_aq=True, with_intra=False, early_sad=1024, use_cost_mv=True, use_seed=True),
    dict(gate_thresh=2400, R=8, early_sad=1024, with_intra=False),
], ids=["neg-aq", "neg-aq-r4-nointra", "r4-early-seed", "r4-costmv-nointra-aq", "r16", "r16-all", "r8-early-nointra"])
@pytest.mark.parametrize("pattern", ["checker", "mixed"])
def test_gated_search_options(host, pattern, opts):
    _check(host, 2, 9, 8, pattern, **opts)


def test_negative_gate_uses_each_mbs_lambda(host):
    """The AQ offsets must change lambda inside a run, or the negative-threshold cases above
    would not tell a per-MB threshold from a per-slot one."""
    d = _inputs(2, 9, 8)
    lam = np.asarray(host.table("lambda")[0])
    qp = np.clip(d["qp"][:, None] + d["aq"].astype(np.int32), 0, 51)
    for b in range(2):
        assert np.unique(lam[qp[b, :8]]).size > 1 and (lam[qp[b]] != lam[d["qp"][b]]).any()


def _pools(hip, B, nbuf, wmb, hmb, seed):
    """Reference pool [B, nbuf, H, W] and its half-sample pool [B, nbuf, 3, H + 8, W + 8]."""
    import torch
    rng = np.random.default_rng(seed)
    W, H = wmb * 16, hmb * 16
    srcs, refs = [], []
    for b in range(B):
        s0, r0 = _smooth(rng, H, W, 2, -1, 2.0)
        _, r1 = _smooth(rng, H, W, 1, 1, 2.0)
        srcs.append(s0)
        refs.append(np.stack([r0, np.clip(s0.astype(np.int32) + 3, 0, 255).astype(np.uint8), r1][:nbuf]))
    dev = torch.device("cuda")
    pool = torch.from_numpy(np.ascontiguousarray(np.stack(refs))).to(dev)
    hp = torch.zeros((B, nbuf, 3, H + 8, W + 8), dtype=torch.uint8, device=dev)
    hip.me_halfpel(B * nbuf, W, H, pool.data_ptr(), hp.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return np.stack(srcs), pool, hp


def _route(kinds, n0, l0, l1):
    import torch
    from govideocompressor_amd.models.h264_gpu import ROUTE_DTYPE
    rt = np.zeros(len(kinds), dtype=ROUTE_DTYPE)
    rt["kind"], rt["n0"], rt["l1"], rt["w1"], rt["dcopy"], rt["disp"] = kinds, n0, l1, 32, 1, -1
    rt["l0"] = l0
    return torch.from_numpy(rt.view(np.uint8).reshape(len(kinds), 32).copy()).to("cuda")


@pytest.mark.parametrize("case", ["want_b", "role_ge_n0"])
def test_gated_search_routed_skips_slots(host, case):
    """Routed launches: a slot that codes another picture type, or whose list 0 has no entry
    `role`, keeps every sentinel; the other slot is gated / searched as above, on the pool
    buffer its route names."""
    from govideocompressor_amd.ops import native
    hip = native.hip()
    B, wmb, hmb, nbuf = 2, 9, 8, 3
    nmb = wmb * hmb
    d = dict(_inputs(B, wmb, hmb))
    d["src"], pool, hp = _pools(hip, B, nbuf, wmb, hmb, 7)
    if case == "want_b":  # slot 0 codes a P picture, slot 1 a B picture whose list-0[0] is buffer 2
        rt = _route([0, 1], [1, 1], [[0, -1, -1, -1], [2, -1, -1, -1]], [-1, 1])
        role, want, skipped, live = 0, 1, 0, 1
    else:                 # two P slots, list-0[1] searched: slot 0 has one active entry only
        rt = _route([0, 0], [1, 2], [[0, -1, -1, -1], [0, 2, -1, -1]], [-1, -1])
        role, want, skipped, live = 1, 0, 0, 1
    kw = dict(route=rt, nbuf=nbuf, role=role, want=want, ref_pool=pool, hp_pool=hp)
    opts = (4, True, 0, True, False, False)
    umv, ucost, upred, uintra = _launch(hip, B, wmb, hmb, d, None, 0, *opts, **kw)
    surv = np.stack([_pattern("mixed", nmb, b) for b in range(B)])
    gate = _gate_costs(host, d, surv, -150, True)
    mv, cost, pred, intra = _launch(hip, B, wmb, hmb, d, gate, -150, *opts, **kw)
    for out, sent in ((umv, S_MV), (ucost, S_COST), (upred, S_PRED), (uintra, S_INTRA),
                      (mv, S_MV), (cost, S_COST), (pred, S_PRED), (intra, S_INTRA)):
        assert (out[skipped] == sent).all()
    sv, g = surv[live], ~surv[live]
    assert (ucost[live] < KNO).all() and (ucost[live] != S_COST).all()
    assert (cost[live][g] == KNO).all() and (intra[live][g] == KNO).all()
    assert (mv[live][g] == S_MV).all() and (pred[live][g] == S_PRED).all()
    for a_, b_ in ((mv, umv), (cost, ucost), (pred, upred), (intra, uintra)):
        assert np.array_equal(a_[live][sv], b_[live][sv])
    # the routed search read buffer 2 of the live slot: an unrouted search of that picture agrees
    d1 = {k: v[live:live + 1] for k, v in d.items()}
    import torch
    ref1 = pool[live, 2:3].contiguous()
    r = _launch(hip, 1, wmb, hmb, d1, None, 0, *opts, ref_pool=ref1)
    assert np.array_equal(r[0][0], umv[live]) and np.array_equal(r[1][0], ucost[live])
    assert np.array_equal(r[2][0], upred[live])
    del torch


# ---------------------------------------------------------------- me_ref_select


def _ref_select_numpy(lam, qp, aq, n0, nref, mv, mv8, cost, pred, xmv, xcost, xpred, active):
    mv, cost, pred = mv.copy(), cost.copy(), pred.copy()
    mv8 = None if mv8 is None else mv8.copy()
    mref = np.full(cost.shape, 99, dtype=np.int8)
    for b in np.flatnonzero(active):
        for m in range(cost.shape[1]):
            L = int(lam[np.clip(qp[b] + (0 if aq is None else int(aq[b, m])), 0, 51)])
            best, bk = int(cost[b, m]) + L, 0
            for k in range(1, min(nref, n0[b])):
                c = int(xcost[k - 1, b, m])
                if c < KNO and c + L * (k + 2) < best:
                    best, bk = c + L * (k + 2), k
            mref[b, m] = bk
            if bk:
                mv[b, m], cost[b, m], pred[b, m] = xmv[bk - 1, b, m], xcost[bk - 1, b, m], xpred[bk - 1, b, m]
                if mv8 is not None:
                    mv8[b, m] = xmv[bk - 1, b, m]
    return mv, mv8, cost, pred, mref


@pytest.mark.parametrize("routed", [False, True], ids=["uniform", "routed"])
@pytest.mark.parametrize("with_mv8", [False, True], ids=["nomv8", "mv8"])
@pytest.mark.parametrize("nref", [2, 3])
@pytest.mark.parametrize("wmb,hmb", [(5, 3), (9, 8)])
def test_me_ref_select_matches_numpy(host, wmb, hmb, nref, with_mv8, routed):
    """Routed: slot 0 has one active list-0 entry (nothing of it may change but mref = 0), slot 1
    has them all, slot 2 codes a B picture (untouched, mref included)."""
    import torch
    from govideocompressor_amd.ops import native
    hip = native.hip()
    B, nmb = 3, wmb * hmb
    rng = np.random.default_rng(wmb * 10 + nref)
    lam = np.asarray(host.table("lambda")[0])
    qp = np.array([24, 30, 36], dtype=np.int32)
    aq = rng.integers(-5, 6, size=(B, nmb)).astype(np.int8)
    mv = rng.integers(-64, 64, size=(B, nmb, 2)).astype(np.int16)
    mv8 = rng.integers(-64, 64, size=(B, nmb, 4, 2)).astype(np.int16)
    cost = rng.integers(800, 1400, size=(B, nmb)).astype(np.int32)
    pred = rng.integers(0, 256, size=(B, nmb, 256)).astype(np.uint8)
    xmv = rng.integers(-64, 64, size=(nref - 1, B, nmb, 2)).astype(np.int16)
    xcost = rng.integers(600, 1600, size=(nref - 1, B, nmb)).astype(np.int32)
    xcost[rng.random(xcost.shape) < 0.4] = KNO
    xcost[:, :, 0] = cost[None, :, 0] - 300  # first and last MB of every slot: a farther picture wins
    xcost[:, :, -1] = cost[None, :, -1] - 300
    xpred = rng.integers(0, 256, size=(nref - 1, B, nmb, 256)).astype(np.uint8)
    n0 = np.array([1, 4, 4] if routed else [4, 4, 4])
    active = np.array([True, True, not routed])
    rt = _route([0, 0, 1], list(n0), [[0, 1, 2, 3]] * 3, [-1, -1, 0]) if routed else None
    dev = torch.device("cuda")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    t_mv, t_mv8, t_cost, t_pred = up(mv), up(mv8), up(cost), up(pred)
    t_xmv, t_xcost, t_xpred, t_qp, t_aq = up(xmv), up(xcost), up(xpred), up(qp), up(aq)
    t_mref = torch.full((B, nmb), 99, dtype=torch.int8, device=dev)
    hip.me_ref_select(B, wmb, hmb, nref, t_mv.data_ptr(), t_mv8.data_ptr() if with_mv8 else 0, t_cost.data_ptr(),
                      t_pred.data_ptr(), t_xmv.data_ptr(), t_xcost.data_ptr(), t_xpred.data_ptr(), t_mref.data_ptr(),
                      t_qp.data_ptr(), t_aq.data_ptr(), torch.cuda.current_stream().cuda_stream,
                      rt.data_ptr() if rt is not None else 0)
    torch.cuda.synchronize()
    e_mv, e_mv8, e_cost, e_pred, e_mref = _ref_select_numpy(lam, qp, aq, n0, nref, mv, mv8 if with_mv8 else None, cost,
                                                            pred, xmv, xcost, xpred, active)
    assert (e_mref[1] > 0).any() and (e_mref[1] == 0).any()
    if nref == 3:
        assert (e_mref[1] == 2).any() and (e_mref[1] == 1).any()
    if routed:
        assert (e_mref[0] == 0).all() and (e_mref[2] == 99).all()
    assert np.array_equal(t_mref.cpu().numpy(), e_mref)
    assert np.array_equal(t_mv.cpu().numpy(), e_mv)
    assert np.array_equal(t_cost.cpu().numpy(), e_cost)
    assert np.array_equal(t_pred.cpu().numpy(), e_pred)
    assert np.array_equal(t_mv8.cpu().numpy(), e_mv8 if with_mv8 else mv8)
