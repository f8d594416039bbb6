"""encode_inter_mb / encode_inter_chroma (csrc/kernels/encode_inter.hip) against the numpy model of
tests/ref_models_h264_inter.py: the kernels are launched directly on small synthetic buffers (no
encoder object, no ME, no b_decide) and every output they own is compared -- the 408 levels of
each MB, nz, the record, intra_flag / intra_count, qp_flags, mask_pre and the reconstruction.

Exact at trellis 0.  With the trellis the kernels price in fp32 and the model in float64: an MB in
which the model made a choice with a relative margin under 1e-4 (``near_tie``) is exempt from the
comparisons that depend on its levels; at most 2 % of a test's MBs may be (the seeds are chosen
so, tests/test_ref_models_h264_inter.py holds that on the CPU).  Every output buffer is poisoned
first; what an MB handed to the intra kernels owns must still be poison afterwards.

Shapes: the smallest at which the four-MBs-per-wave luma layout and the eight-MBs-per-wave chroma
layout can go wrong (1x6: three row wraps inside a luma wave; 2x1: one partly filled wave of each;
3x3: one live MB in the last chroma wave; 5x3: waves straddle rows, three live MBs in the last
luma wave; 7x3: one live MB in the last luma wave, five in the last chroma wave), two slots at
different QPs.  The input families and what each is there for: ref_models_h264_inter.make_case.
"""
import numpy as np
import pytest
import torch

import ref_models_h264_inter as M

pytestmark = pytest.mark.gpu

POISON = 0xA5


def _launch(hip, c, t8, trellis):
    dev = torch.device("cuda")
    B, wmb, hmb = c["B"], c["wmb"], c["hmb"]
    nmb, H, W = wmb * hmb, hmb * 16, wmb * 16

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def poison(shape, dtype):
        size = torch.empty((), dtype=dtype).element_size()
        return torch.full(shape + (size,), POISON, dtype=torch.uint8, device=dev).view(dtype).reshape(shape)
    sy, su, sv, pred = t(c["src_y"]), t(c["src_u"]), t(c["src_v"]), t(c["pred_y"])
    ru, rv = [t(r) for r in c["refs_u"]], [t(r) for r in c["refs_v"]]
    fy = torch.zeros((B, H, W), dtype=torch.uint8, device=dev)  # the luma reference: not read
    mv, me, ic, qp = t(c["mv"]), t(c["me_cost"]), t(c["intra_cost"]), t(c["qp"])
    opt = {k: (None if c[k] is None else t(c[k])) for k in ("aq", "mv8", "mref", "wp", "ref1_u", "ref1_v")}
    hdr = t(M.case_hdr_in(c, POISON))
    out = dict(hdr=hdr, coef=poison((B, nmb, M.COEF_PER_MB), torch.int16), nz=poison((B, nmb, 16), torch.uint8),
               intra_flag=poison((B, nmb), torch.uint8), intra_count=torch.zeros(B, dtype=torch.int32, device=dev),
               rec_y=poison((B, H, W), torch.uint8), rec_u=poison((B, H // 2, W // 2), torch.uint8),
               rec_v=poison((B, H // 2, W // 2), torch.uint8), qp_flags=poison((B, nmb), torch.uint8),
               mask_pre=poison((B, nmb), torch.int32))

    def p(x):
        return 0 if x is None else x.data_ptr()
    hip.encode_inter(B, wmb, hmb, p(sy), p(su), p(sv), p(fy), p(ru[0]), p(rv[0]), p(out["rec_y"]), p(out["rec_u"]),
                     p(out["rec_v"]), p(pred), p(mv), p(me), p(ic), p(qp), int(c["cqo"]), p(hdr), p(out["coef"]),
                     p(out["nz"]), p(out["intra_flag"]), p(out["intra_count"]), torch.cuda.current_stream().cuda_stream,
                     aq=p(opt["aq"]), ref1_u=p(opt["ref1_u"]), ref1_v=p(opt["ref1_v"]), bmode=int(c["bmode"]), t8=int(t8),
                     mv8=p(opt["mv8"]), w1=[int(w) for w in c["w1"]], xref_u=[p(x) for x in ru[1:]],
                     xref_v=[p(x) for x in rv[1:]], mref=p(opt["mref"]), wp=p(opt["wp"]), trellis=int(trellis),
                     trellis_lambda=1.0, qp_flags=p(out["qp_flags"]), mask_pre=p(out["mask_pre"]))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _mb_view(plane, wmb, hmb, n):
    """[H, W] -> [nmb, n, n]"""
    return plane.reshape(hmb, n, wmb, n).transpose(0, 2, 1, 3).reshape(wmb * hmb, n, n)


def _compare(c, got, want, trellis, tag):
    wmb, hmb = c["wmb"], c["hmb"]
    pcoef = np.frombuffer(bytes([POISON, POISON]), np.int16)[0]
    for b, o in enumerate(want):
        where = "%s slot %d" % (tag, b)
        work, tie = o["work"], o["near_tie"]
        assert trellis or not tie.any()
        sure = work & ~tie          # every output compared
        intra = ~work
        # what never depends on a level
        np.testing.assert_array_equal(got["intra_flag"][b], o["intra_flag"], err_msg=where + " intra_flag")
        assert int(got["intra_count"][b]) == o["intra_count"], where + " intra_count"
        ghdr = got["hdr"][b].copy()
        whdr = o["hdr"].copy()
        ghdr[tie, M._FLAGS] = whdr[tie, M._FLAGS]
        bad = np.flatnonzero((ghdr != whdr).any(axis=1))
        assert bad.size == 0, "%s record of MB %s: got %s want %s" % (where, bad[:4], ghdr[bad[:1]], whdr[bad[:1]])
        # levels, nz, flags, masks
        gm = got["mask_pre"][b].view(np.uint32)
        for name, g, w in (("coef", got["coef"][b], o["coef"]), ("nz", got["nz"][b], o["nz"]),
                           ("qp_flags", got["qp_flags"][b], o["qp_flags"]), ("mask_pre", gm, o["mask_pre"])):
            g, w = g.reshape(len(work), -1), w.reshape(len(work), -1)
            bad = np.flatnonzero((g[sure] != w[sure]).any(axis=1))
            if bad.size:
                mb = np.flatnonzero(sure)[bad[0]]
                d = np.flatnonzero(g[mb] != w[mb])
                raise AssertionError("%s %s of %d MBs, first MB %d at %s: got %s want %s (trail %s)" % (
                    where, name, bad.size, mb, d[:8], g[mb][d[:8]], w[mb][d[:8]],
                    {k: v for k, v in o["trail"][mb]["luma"].items() if k in ("score4", "sa8d", "satd", "use8", "score8")}))
        np.testing.assert_array_equal(got["qp_flags"][b][intra], 2, err_msg=where)
        np.testing.assert_array_equal(gm[intra], M.BLOCK_MASK_INTRA, err_msg=where)
        # an MB handed to the intra kernels: its levels, nz and reconstruction are not touched
        assert (got["coef"][b][intra] == pcoef).all(), where + " levels of an intra MB written"
        assert (got["nz"][b][intra] == POISON).all(), where + " nz of an intra MB written"
        for name, n in (("rec_y", 16), ("rec_u", 8), ("rec_v", 8)):
            g, w = _mb_view(got[name][b], wmb, hmb, n), _mb_view(o[name], wmb, hmb, n)
            bad = np.flatnonzero((g[sure] != w[sure]).any(axis=(1, 2)))
            assert bad.size == 0, "%s %s of MBs %s" % (where, name, np.flatnonzero(sure)[bad][:6])
            assert (g[intra] == POISON).all(), where + " " + name + " of an intra MB written"


@pytest.mark.parametrize("wmb,hmb,bmode,t8,trellis,aq", M.grid())
def test_encode_inter_matches_model(wmb, hmb, bmode, t8, trellis, aq):
    from govideocompressor_amd.ops import native
    hip = native.hip()
    seed = M.SEEDS[(wmb, hmb, bmode, aq)]
    ties = work = 0
    for fam in M.families(bmode, trellis):
        c = M.cached_case(fam, wmb, hmb, bmode, seed, aq, trellis)
        want = M.cached_model(fam, wmb, hmb, bmode, seed, aq, t8, trellis, POISON)
        n = M.family_counts(c, want)
        assert M.missing_counts(fam, n, wmb * hmb, t8) == [], (fam, n)
        ties += n["tie"]
        work += n["work"]
        got = _launch(hip, c, t8, trellis)
        _compare(c, got, want, trellis, fam)
    assert ties <= (M.TIE_CAP * work if trellis else 0), (ties, work)
