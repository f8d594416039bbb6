"""``hv::tskip_tu`` (csrc/kernels/hevc_tskip.h) through its stand-alone probe launch
(``hip.hevc_tskip_probe``) against the numpy model of tests/ref_models_hevc_tskip.py: levels,
reconstructed samples, transform_skip_flag, cbf, D_A, D_B, R_A and R_B of every block must be
equal, no tolerance, no block left out, on poisoned output buffers.

One case per kind of TU (intra luma with the DST, intra chroma and inter chroma with the DCT), bit
depth (8 / 10) and QpY in {12, 26, 40} (Qp' = QpY + 6 (bit depth - 8); lamq from the rd_cbf table at
tskip_lambda 1.0), plus, per kind and bit depth, the two ends of the Qp' range (Qp' 0 with the
table's entry 0, and Qp' 51 + 6 (bit depth - 8) with entry 51).  In each case every variant of
VARIANTS -- scanIdx 0 / 1 / 2, sign data hiding on / off, RDOQ level 0 / 1 / 2 at rdoq_lambda 0.5
-- is one launch on the same 256 + 6 blocks:

* 128 glyph blocks: a flat prediction, the source with about 40 % of its samples (each with
  probability 0.4, at least one) raised by one amplitude per block, 40 .. 120 at 8-bit scale
  (at the largest Qp', whose step is 228 samples at 8-bit scale and leaves such blocks without any
  level either way, 200 .. 249 on a prediction of 0 .. 5);
* 128 gradient blocks: a flat prediction, the source a plane whose corner-to-corner rise is
  8 .. 40 at 8-bit scale, with +-2 noise;
* a handful of full-range blocks: +-maxv everywhere, a full-range checkerboard both ways, and a
  single +-maxv sample.

Before the GPU is used each case asserts on the model alone that every variant picks B for 20 % to
80 % of its 256 glyph and gradient blocks: a kernel that never or always picks B cannot pass.
Measured on the model with these blocks: B wins 74 - 100 % of the glyph blocks and 0 - 20 % of the
gradient blocks (the latter only at Qp' 0, where both candidates are nearly lossless), 30 - 60 % of
the two together.

The hand cases of tests/test_ref_models_hevc_tskip.py run through the probe in a test of their
own (their lamq values are not a table's).
"""
import functools

import numpy as np
import pytest

import ref_models_hevc_rdcbf as rc
import ref_models_hevc_rdoq as rq
import ref_models_hevc_tskip as ts

pytestmark = pytest.mark.gpu

NGLYPH = NGRAD = 128
# (name, intra, dst)
KINDS = [("intra-luma-dst", True, True), ("intra-chroma-dct", True, False), ("inter-chroma-dct", False, False)]
QPYS = (12, 26, 40)
CASES = [(k, bd, qpy) for k in range(3) for bd in (8, 10) for qpy in QPYS]
END_CASES = [(k, bd, end) for k in range(3) for bd in (8, 10) for end in (0, 1)]
# (name, scanIdx, sdh, rdoq level)
VARIANTS = [("dz-s0", 0, False, 0), ("dz-s1", 1, False, 0), ("sdh-s2", 2, True, 0), ("sdh-s0", 0, True, 0),
            ("rdoq1-s2", 2, False, 1), ("rdoq2-s1", 1, False, 2), ("sdh-rdoq2-s0", 0, True, 2), ("sdh-rdoq1-s1", 1, True, 1)]
RDOQ_LAM = rq.lam_of(0.5)
POISON16, POISON32, POISON64 = -21846, -1431655766, -6148914691236517206


def _case_id(c):
    return f"{KINDS[c[0]][0]}-bd{c[1]}-qpy{c[2]}"


def _end_id(c):
    return f"{KINDS[c[0]][0]}-bd{c[1]}-{'qp-max' if c[2] else 'qp-0'}"


@functools.lru_cache(maxsize=1)
def _dct32():
    from govideocompressor_amd.ops import native
    return np.asarray(native.host().table("hevc_dct32"), dtype=np.int64).reshape(32, 32)


def _blocks(kind, bd, seed, coarse=False):
    """(src, pred) uint16 [262, 4, 4]: glyph blocks, gradient blocks, full-range blocks; coarse: the
    glyph amplitudes of the largest Qp'"""
    maxv, k = (1 << bd) - 1, 1 << (bd - 8)
    rng = np.random.default_rng(1000 * kind + 10 * bd + seed)
    src, pred = [], []
    yy, xx = np.mgrid[0:4, 0:4]
    for _ in range(NGLYPH):
        base = int(rng.integers(0, 6) if coarse else rng.integers(30, 120)) * k
        on = rng.random((4, 4)) < 0.4
        if not on.any():
            on[rng.integers(0, 4), rng.integers(0, 4)] = True
        amp = int(rng.integers(200, 250) if coarse else rng.integers(40, 121)) * k
        pred.append(np.full((4, 4), base))
        src.append(base + on * amp)
    for _ in range(NGRAD):
        base = int(rng.integers(60, 190)) * k
        gx, gy = rng.uniform(-1, 1, 2)
        rise = rng.uniform(8, 40) * k / 6.0 / max(abs(gx) + abs(gy), 0.25)
        plane = np.rint(rise * (gx * (xx - 1.5) + gy * (yy - 1.5))).astype(np.int64)
        pred.append(np.full((4, 4), base))
        src.append(np.clip(base + plane + rng.integers(-2, 3, (4, 4)), 0, maxv))
    full, zero = np.full((4, 4), maxv), np.zeros((4, 4), dtype=np.int64)
    chk = ((xx + yy) & 1) * maxv
    one = np.zeros((4, 4), dtype=np.int64)
    one[2, 1] = maxv
    for s, p in ((full, zero), (zero, full), (chk, maxv - chk), (maxv - chk, chk), (one, zero), (maxv - one, full)):
        src.append(s)
        pred.append(p)
    return np.stack(src).astype(np.uint16), np.stack(pred).astype(np.uint16)


def _model(src, pred, intra, dst, bd, qp, lamq, scan, sdh, rdoq):
    r = [ts.tskip_tu(s, p, _dct32(), bd, qp, lamq, intra, dst, scan, sdh, rdoq, RDOQ_LAM if rdoq else 0) for s, p in zip(src, pred)]
    return (np.stack([v[0] for v in r]), np.stack([v[1] for v in r]), np.array([v[2:4] for v in r], dtype=np.int32),
            np.array([v[4:8] for v in r], dtype=np.int64))


@functools.lru_cache(maxsize=2)
def expected(kind, bd, qp, lamq_q, seed):
    """(src, pred, {variant name: (levels, samples, flags [nblk, 2], terms [nblk, 4])})"""
    _, intra, dst = KINDS[kind]
    src, pred = _blocks(kind, bd, seed, coarse=qp >= 51)
    lamq = rc.lamq_table(1.0, bd)[lamq_q]
    return src, pred, {name: _model(src.astype(np.int64), pred.astype(np.int64), intra, dst, bd, qp, lamq, scan, sdh, rdoq)
                       for name, scan, sdh, rdoq in VARIANTS}


def b_share(out, name):
    """share of the glyph and gradient blocks for which the model picks B, and of each kind"""
    f = out[name][2][:NGLYPH + NGRAD, 0]
    return float(f.mean()), float(f[:NGLYPH].mean()), float(f[NGLYPH:].mean())


def _probe(src, pred, bd, qp, intra, dst, scan, sdh, rdoq, rdoq_lam, lamq):
    """the probe on blocks [nblk, 4, 4] with poisoned outputs: (levels, samples, flags, terms)"""
    import torch

    from govideocompressor_amd.ops import native
    nblk = len(src)
    dev = torch.device("cuda", torch.cuda.current_device())
    d_src = torch.from_numpy(np.asarray(src).astype(np.uint16).view(np.int16)).to(dev)
    d_pred = torch.from_numpy(np.asarray(pred).astype(np.uint16).view(np.int16)).to(dev)
    d_lev = torch.full((nblk, 4, 4), POISON16, dtype=torch.int16, device=dev)
    d_rec = torch.full((nblk, 4, 4), POISON16, dtype=torch.int16, device=dev)
    d_flag = torch.full((nblk, 2), POISON32, dtype=torch.int32, device=dev)
    d_terms = torch.full((nblk, 4), POISON64, dtype=torch.int64, device=dev)
    native.hip().hevc_tskip_probe(nblk, d_src.data_ptr(), d_pred.data_ptr(), d_lev.data_ptr(), d_rec.data_ptr(),
                                  d_flag.data_ptr(), d_terms.data_ptr(), bd, qp, int(intra), int(dst), scan, int(sdh), rdoq,
                                  rdoq_lam, lamq, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return (d_lev.cpu().numpy().astype(np.int64), d_rec.cpu().numpy().astype(np.int64) & 0xFFFF, d_flag.cpu().numpy(),
            d_terms.cpu().numpy())


def _compare(tag, got, want):
    lev, rec, flag, terms = got
    wl, wr, wf, wt = want
    for k, what in enumerate(("D_A", "D_B", "R_A", "R_B")):
        bad = np.flatnonzero(terms[:, k] != wt[:, k])
        assert bad.size == 0, (tag, what, bad[:8].tolist(), terms[bad[:4], k].tolist(), wt[bad[:4], k].tolist())
    for k, what in enumerate(("transform_skip_flag", "cbf")):
        assert np.array_equal(flag[:, k], wf[:, k]), (tag, what, np.flatnonzero(flag[:, k] != wf[:, k])[:8].tolist())
    bad = np.flatnonzero((lev != wl).any(axis=(1, 2)))
    assert bad.size == 0, (tag, "levels", bad[:8].tolist(), np.argwhere(lev[bad[0]] != wl[bad[0]])[:4].tolist())
    bad = np.flatnonzero((rec != wr).any(axis=(1, 2)))
    assert bad.size == 0, (tag, "samples", bad[:8].tolist())


def _run_case(kind, bd, qp, lamq_q, seed):
    _, intra, dst = KINDS[kind]
    src, pred, out = expected(kind, bd, qp, lamq_q, seed)
    assert len(src) == NGLYPH + NGRAD + 6
    for name, *_ in VARIANTS:
        share, glyph, grad = b_share(out, name)
        print(f"{KINDS[kind][0]} bd{bd} qp'{qp} {name}: B picked for {share:.3f} (glyph {glyph:.3f}, gradient {grad:.3f})")
        assert 0.2 <= share <= 0.8, (name, "share of glyph and gradient blocks with B", share, glyph, grad)
    lamq = rc.lamq_table(1.0, bd)[lamq_q]
    for name, scan, sdh, rdoq in VARIANTS:
        got = _probe(src, pred, bd, qp, intra, dst, scan, sdh, rdoq, RDOQ_LAM if rdoq else 0, lamq)
        _compare(name, got, out[name])


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_probe_equals_model(case):
    kind, bd, qpy = case
    _run_case(kind, bd, qpy + 6 * (bd - 8), qpy, qpy)


@pytest.mark.parametrize("case", END_CASES, ids=_end_id)
def test_probe_equals_model_at_the_qp_ends(case):
    kind, bd, end = case
    _run_case(kind, bd, (51 + 6 * (bd - 8)) if end else 0, 51 if end else 0, 90 + end)


def test_probe_on_the_hand_cases():
    """the cases of tests/test_ref_models_hevc_tskip.py: the tie and its neighbour, the CBF0 branch,
    the clips, the 10-bit shift, the three scans"""
    def imp(a, y=1, x=1, base=128):
        p = np.full((4, 4), base, dtype=np.int64)
        s = p.copy()
        s[y, x] += a
        return s, p

    runs = []  # (src, pred, bd, qp, dst, scan, lamq)
    for lamq in (2048, 2047):
        runs.append((*imp(33, 0, 1), 8, 34, True, 0, lamq))
    for a in (30, 31, 32, 38, 60, 3):
        runs.append((*imp(a), 8, 34, True, 0, 1471))
    runs.append((*imp(6, base=249), 8, 22, True, 0, 1))
    runs.append((*imp(-6, base=6), 8, 22, True, 0, 1))
    runs.append((*imp(24, base=999), 10, 34, True, 0, 1))
    runs.append((*imp(-24, base=24), 10, 34, True, 0, 1))
    runs.append((*imp(240, base=512), 10, 46, True, 0, 23533))
    for scan in (0, 1, 2):
        runs.append((*imp(64, 0, 1), 8, 34, False, scan, 1471))
    want_ts = [0, 1, 0, 0, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1]
    for (s, p, bd, qp, dst, scan, lamq), wts in zip(runs, want_ts):
        want = ts.tskip_tu(s, p, _dct32(), bd, qp, lamq, True, dst, scan)
        assert want[2] == wts
        lev, rec, flag, terms = _probe(s[None], p[None], bd, qp, True, dst, scan, False, 0, 0, lamq)
        assert np.array_equal(lev[0], want[0]) and np.array_equal(rec[0], want[1])
        assert flag[0].tolist() == list(want[2:4]) and terms[0].tolist() == list(want[4:8])


def test_probe_refuses_bad_parameters():
    import torch

    from govideocompressor_amd.ops import native
    hip = native.hip()
    dev = torch.device("cuda", torch.cuda.current_device())
    buf = torch.zeros((64,), dtype=torch.int64, device=dev)
    q = buf.data_ptr()
    ok = dict(nblk=1, src=q, pred=q, lev=q, rec=q, flag=q, terms=q, bd=8, qp=30, intra=1, dst=0, scan=0, sdh=0, rdoq=0,
              rdoq_lam=0, lamq=100, stream=torch.cuda.current_stream(dev).cuda_stream)
    for bad in (dict(bd=9), dict(qp=52), dict(qp=-1), dict(scan=3), dict(rdoq=3), dict(rdoq_lam=1473), dict(lamq=(1 << 23) + 1),
                dict(lamq=-1), dict(nblk=0), dict(intra=0, dst=1), dict(lev=0)):
        with pytest.raises(ValueError):
            hip.hevc_tskip_probe(**dict(ok, **bad))
    torch.cuda.synchronize(dev)
