"""``p_mixed_refs`` (csrc/kernels/h264_p_mixed.hip) against its numpy definition
(tests/ref_models_h264_mixed.py): every output of every MB, exactly.

A launch has four slots: three P slots with 1, 2 and 3 active list-0 pictures, each with planes,
pool buffers, QP, AQ offsets and distance scales of its own, and an I slot.  The source of a P
slot is a chequer of 8x8 cells, each cut from one of the slot's reference pictures at a small
common shift plus noise, so quadrants of one MB are best predicted from different pictures.  The
I slot's poisoned outputs must come back untouched and the one-picture slot's as ``me_ref_select``
leaves them (reference 0, nothing else).  Vectors leave the picture on all four sides; the AQ
offsets change lambda inside a run of MBs; ``pattern`` says which MBs had a farther picture
searched (none, one, all, some).  Geometries 3x2 and 5x3 MBs (odd, a partial run of a wave), and
9x8 (72 MBs: a second wave per slot, with a partial run)."""
import numpy as np
import pytest

import ref_models_h264_mixed as mx

KNO = mx.KNO
B, NBUF = 4, 4
KINDS, N0 = [0, 0, 0, 2], [1, 2, 3, 1]
L0 = [[1, 0, 2, -1], [2, 0, 1, -1], [1, 3, 0, -1], [-1, -1, -1, -1]]
QP = np.array([26, 30, 34, 28], dtype=np.int32)
SCALE = np.array([[512, 384, 512, 256], [768, 640, 700, 256]], dtype=np.int16)
OVERHEAD, MIN_SATD = 8, 600

_CASES = {}


def _smooth(rng, H, W):
    base = rng.integers(0, 256, size=(H + 8, W + 8)).astype(np.float64)
    k = np.ones(3) / 3
    base = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 1, base)
    base = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 0, base)
    return np.clip(base[4:4 + H, 4:4 + W], 0, 255).astype(np.uint8)


def _inputs(wmb, hmb, pattern):
    """The planted buffers of a launch (numpy), made once per case."""
    key = (wmb, hmb, pattern)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(1000 * wmb + 10 * hmb + len(pattern))
    nmb, W, H = wmb * hmb, wmb * 16, hmb * 16
    pool = np.stack([np.stack([_smooth(rng, H, W) for _ in range(NBUF)]) for _ in range(B)])
    src = np.zeros((B, H, W), dtype=np.uint8)
    shift = [(1, -1), (-2, 1), (1, 2), (0, 0)]  # (dx, dy) samples per picture of distance: the source is the reference moved by it
    for b in range(B):
        ext = np.pad(pool[b], ((0, 0), (8, 8), (8, 8)), mode="edge")
        for cy in range(H // 8):
            for cx in range(W // 8):
                k = int(rng.integers(0, max(1, N0[b])))
                buf = max(0, L0[b][k])
                dx, dy = shift[b][0] * (k + 1), shift[b][1] * (k + 1)  # list entry k is k + 1 pictures away
                cell = ext[buf, 8 + cy * 8 + dy:16 + cy * 8 + dy, 8 + cx * 8 + dx:16 + cx * 8 + dx]
                src[b, cy * 8:cy * 8 + 8, cx * 8:cx * 8 + 8] = np.clip(cell + rng.normal(0, 1.5, (8, 8)), 0, 255)
    src0 = src.copy()
    src0[2] = np.clip(src[2].astype(np.int32) * 9 // 8 - 6, 0, 255)  # slot 2: an inverse-weighted source
    base = np.array([[4 * s[0], 4 * s[1]] for s in shift], dtype=np.int32)
    mv8 = (base[:, None, None, :] + rng.integers(-3, 4, size=(B, nmb, 4, 2))).astype(np.int16)
    mv = mv8[:, :, 0].copy()
    xmv = (base[None, :, None, :] * np.array([2, 3])[:, None, None, None]
           + rng.integers(-4, 5, size=(2, B, nmb, 2))).astype(np.int16)
    # vectors off the picture on every side (first / last MBs: the corners) and at the range's ends
    far = [(-300, -200), (300, 200), (-2048, -512), (2047, 511)]
    for i, v in enumerate(far):
        m = [0, nmb - 1, wmb - 1, nmb - wmb][i]
        mv8[1:3, m, i] = v
        xmv[:, 1:3, m] = (-v[0] // 2, -v[1] // 2) if i < 2 else v
    pm = (base[:, None, :] + rng.integers(-6, 7, size=(B, nmb, 2))).astype(np.int16)
    pm[2, nmb // 2] = (1900, -480)  # scales past the range
    # costs: every third MB keeps its list-0[0] decision cheap ((a) wins), every third has a cheap
    # 16x16 farther picture ((b)), the rest are dear either way, as MBs on an occlusion edge are ((c))
    i = np.arange(nmb)
    cost = (9000 + rng.integers(0, 500, size=(B, nmb))).astype(np.int32)
    xcost = (8000 + rng.integers(0, 500, size=(2, B, nmb))).astype(np.int32)
    cost[:, i % 3 == 0] = 300 + rng.integers(0, 200, size=(B, int((i % 3 == 0).sum())))
    for m in i[i % 3 == 1]:
        xcost[m % 2, :, m] = 300 + rng.integers(0, 200, size=B)
    if pattern == "none":
        xcost[:] = KNO
    elif pattern == "one":
        keep = xcost[0, :, nmb // 2].copy()
        xcost[:] = KNO
        xcost[0, :, nmb // 2] = keep
    elif pattern == "some":
        xcost[0][:, i % 5 == 3] = KNO
        xcost[1][:, i % 4 == 2] = KNO
    else:
        assert pattern == "all"
    d = dict(wmb=wmb, hmb=hmb, pool=pool, src=src, src0=src0, mv=mv, mv8=mv8, xmv=xmv, pm=pm, cost=cost, xcost=xcost,
             pred=rng.integers(0, 256, size=(B, nmb, 256)).astype(np.uint8),
             xpred=rng.integers(0, 256, size=(2, B, nmb, 256)).astype(np.uint8),
             aq=rng.integers(-6, 7, size=(B, nmb)).astype(np.int8),
             mref=np.full((B, nmb), 99, np.int8), mref4=np.full((B, nmb, 4), 99, np.int8))
    _CASES[key] = d
    return d


def _model(lam, d, min_satd=MIN_SATD, slots=slice(None)):
    s = slots
    return mx.p_mixed_refs(lam, d["wmb"], d["hmb"], 3, KINDS[s], N0[s], L0[s], QP[s], d["aq"][s], d["mv"][s], d["mv8"][s],
                           d["cost"][s], d["pred"][s], d["xmv"][:, s], d["xcost"][:, s], d["xpred"][:, s], d["mref"][s],
                           d["mref4"][s], d["src0"][s], d["src"][s], d["pool"][s], d["pm"][s], SCALE[:, s], OVERHEAD,
                           min_satd)


def _route(slots=slice(None)):
    import torch
    from govideocompressor_amd.models.h264_gpu import ROUTE_DTYPE
    kinds = KINDS[slots]
    rt = np.zeros(len(kinds), dtype=ROUTE_DTYPE)
    rt["kind"], rt["n0"], rt["l1"], rt["w1"], rt["dcopy"], rt["disp"] = kinds, N0[slots], -1, 32, 1, -1
    rt["l0"] = L0[slots]
    return torch.from_numpy(rt.view(np.uint8).reshape(len(kinds), 32).copy()).to("cuda")


def _launch(d, min_satd=MIN_SATD, slots=slice(None), select=False):
    """p_mixed_refs (or me_ref_select on the same inputs) -> dict of the outputs"""
    import torch
    from govideocompressor_amd.ops import native
    hip = native.hip()
    dev = torch.device("cuda")
    s = torch.cuda.current_stream().cuda_stream
    wmb, hmb = d["wmb"], d["hmb"]
    W, H = wmb * 16, hmb * 16
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    nb = len(KINDS[slots])
    t = {k: up(d[k][slots]) for k in ("pool", "src", "src0", "mv", "mv8", "pm", "cost", "pred", "aq", "mref", "mref4")}
    t.update({k: up(d[k][:, slots]) for k in ("xmv", "xcost", "xpred")})
    t["qp"], t["scale"] = up(QP[slots]), up(SCALE[:, slots])
    rt = _route(slots)
    hp = torch.zeros((nb, NBUF, 3, H + 8, W + 8), dtype=torch.uint8, device=dev)
    hip.me_halfpel(nb * NBUF, W, H, t["pool"].data_ptr(), hp.data_ptr(), s)
    P = lambda k: t[k].data_ptr()  # noqa: E731
    if select:
        hip.me_ref_select(nb, wmb, hmb, 3, P("mv"), P("mv8"), P("cost"), P("pred"), P("xmv"), P("xcost"), P("xpred"),
                          P("mref"), P("qp"), P("aq"), s, rt.data_ptr())
    else:
        hip.p_mixed_refs(nb, wmb, hmb, 3, P("mv"), P("mv8"), P("cost"), P("pred"), P("xmv"), P("xcost"), P("xpred"),
                         P("mref"), P("mref4"), P("qp"), P("aq"), P("src0"), P("src"), P("pool"), hp.data_ptr(), P("pm"),
                         P("scale"), OVERHEAD, min_satd, s, rt.data_ptr(), NBUF)
    torch.cuda.synchronize()
    return {k: t[k].cpu().numpy() for k in ("mv", "mv8", "cost", "pred", "mref", "mref4")}


def _lam(host):
    return np.asarray(host.table("lambda")[0])


def check_expectation(e, d, pattern):
    """What the planted case must exercise (also run on the CPU, tests/test_ref_models_h264_mixed.py
    has the rule itself): slots, winners and references."""
    w = e["winner"]
    assert (w[3] == 0).all() and (e["mref"][3] == 99).all() and (e["mref4"][3] == 99).all()  # the I slot
    assert (w[0] == 1).all() and (e["mref"][0] == 0).all() and (e["mref4"][0] == 0).all()    # one picture
    for k in ("mv", "mv8", "cost", "pred"):
        assert np.array_equal(e[k][0], d[k][0]) and np.array_equal(e[k][3], d[k][3])
    if pattern == "none":
        assert (w[:3] == 1).all()
    elif pattern == "one":
        assert (np.delete(w[:3], d["wmb"] * d["hmb"] // 2, axis=1) == 1).all()
    else:
        assert all((w == k).any() for k in (1, 2, 3))
        mixed = e["mref4"][w == 3]
        assert all((mixed == r).any() for r in (0, 1, 2))
        assert (w[1] == 3).any() and (w[2] == 3).any() and not (e["mref4"][1] == 2).any()


@pytest.mark.gpu
@pytest.mark.parametrize("wmb,hmb,pattern", [(w, h, p) for w, h in ((3, 2), (5, 3)) for p in ("some", "all", "one", "none")]
                         + [(9, 8, "some")])
def test_p_mixed_refs_matches_numpy(host, wmb, hmb, pattern):
    d = _inputs(wmb, hmb, pattern)
    e = _model(_lam(host), d)
    check_expectation(e, d, pattern)
    if wmb * hmb > 64:  # the second wave of a slot decides too, in every way
        assert all((e["winner"][1:3, 64:] == k).any() for k in (1, 2, 3))
    g = _launch(d)
    for k in ("mref", "mref4", "mv", "mv8", "cost", "pred"):
        assert np.array_equal(g[k], e[k]), k


@pytest.mark.gpu
def test_aq_changes_lambda_inside_a_run(host):
    """or the comparison above could not tell a lambda per MB from one per slot"""
    d, lam = _inputs(5, 3, "all"), _lam(host)
    for b in range(3):
        assert np.unique(lam[np.clip(QP[b] + d["aq"][b].astype(np.int32), 0, 51)]).size > 2


@pytest.mark.gpu
@pytest.mark.parametrize("wmb,hmb", [(3, 2), (5, 3)])
def test_nothing_eligible_is_me_ref_select(host, wmb, hmb):
    """min_satd beyond any SATD: no MB is priced per quadrant, and every buffer me_ref_select writes
    comes back byte for byte as me_ref_select leaves it on the same inputs"""
    d = _inputs(wmb, hmb, "all")
    g = _launch(d, min_satd=1 << 28)
    r = _launch(d, select=True)
    for k in ("mref", "mv", "mv8", "cost", "pred"):
        assert np.array_equal(g[k], r[k]), k
    assert np.array_equal(g["mref4"][:3], np.repeat(r["mref"][:3, :, None], 4, axis=2))
    assert (g["mref4"][3] == 99).all() and (g["mref"] > 0).any()
    e = _model(_lam(host), d, min_satd=1 << 28)
    assert np.array_equal(g["mref4"], e["mref4"]) and not (e["winner"] == 3).any()


@pytest.mark.gpu
def test_slot_alone_equals_slot_in_the_batch(host):
    d = _inputs(5, 3, "all")
    g = _launch(d)
    alone = _launch(d, slots=slice(2, 3))
    for k in ("mref", "mref4", "mv", "mv8", "cost", "pred"):
        assert np.array_equal(alone[k][0], g[k][2]), k
    assert (g["mref4"][2] != g["mref4"][2][:, :1]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("bad", ["nref", "route", "mv8_align", "null"])
def test_shim_refuses(bad):
    import torch
    from govideocompressor_amd.ops import native
    hip = native.hip()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    a = [1, 1, 1, 3] + [p] * 17 + [8, 600, 0, p, 4]
    if bad == "nref":
        a[3] = 5
    elif bad == "route":
        a[-2] = 0
    elif bad == "mv8_align":
        a[5] = p + 4
    else:
        a[12] = 0
    with pytest.raises(ValueError):
        hip.p_mixed_refs(*a)
