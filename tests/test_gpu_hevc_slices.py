"""HEVC GPU encoder with several slices per picture (``HevcParams.slices``, x265 --slices).

* the GPU reconstruction is bit-exact against the independent CPU decoder's output of the
  written stream: intra pictures (the closed-loop intra kernel runs one workgroup per slice and
  takes no sample from another slice), P and B pictures with AQ (the QP predictor restarts per
  slice), several references, RDOQ;
* the GPU entropy coder writes the host writer's bytes, with one workgroup per picture and with
  a picture's rows spread over several workgroups;
* ``hevc_b_merge`` equals the numpy model once the model's availability adds "same slice";
* the GPU decoder reads the streams.
"""
import numpy as np
import pytest

import ref_models_hevc_merge as hm

pytestmark = pytest.mark.gpu


def _encode(w, h, F, B, bd=8, entropy=None, keep=True, seed=7, **kw):
    from govideocompressor_amd.models.h264_gpu import synth_clip
    from govideocompressor_amd.models.hevc_gpu import GpuHevcEncoder, HevcParams
    y, u, v = synth_clip(B, F, w, h, seed=seed, bit_depth=bd)
    enc = GpuHevcEncoder(HevcParams(width=w, height=h, bit_depth=bd, **kw), slots=B, entropy=entropy)
    res = enc.encode(y, u, v, keep_recon=keep, metrics=keep)
    rec = enc.last_recon if keep else None
    enc.close()
    return res, rec


def _compare(host, res, rec, skip_filters=False):
    for b, r in enumerate(res):
        pics = host.hevc_decode(r.bitstream, skip_filters)
        assert len(pics) == r.frames
        for t, p in enumerate(pics):
            for k, name in enumerate(("y", "u", "v")):
                g = rec[t][k][b].cpu().numpy().astype(np.uint16)
                d = p[name]
                if not np.array_equal(g, d):
                    diff = np.argwhere(g != d)
                    raise AssertionError(f"slot {b} pic {t} plane {name}: {len(diff)} samples differ, first "
                                         f"{diff[0].tolist()} gpu {g[tuple(diff[0])]} cpu {d[tuple(diff[0])]}")


def _slice_nals(stream):
    from govideocompressor_amd.segment import mp4_hevc
    return [n for n in mp4_hevc.split_nals(stream) if ((n[0] >> 1) & 0x3F) < 32]


# ---------------------------------------------------------------------------- intra pictures

@pytest.mark.parametrize("ctu64,S", [(False, 2), (False, 5), (True, 2), (True, 3)])
def test_gpu_hevc_slices_intra_matches_decoder(host, ctu64, S):
    res, rec = _encode(192, 160, 2, 2, intra_only=True, crf=None, qp=30, ctu64=ctu64, slices=S)
    _compare(host, res, rec)
    for r in res:
        assert len(_slice_nals(r.bitstream)) == 2 * S


def test_gpu_hevc_slices_intra_no_filters(host):
    """Both loop filters off: a mismatch here is in the prediction or the residual."""
    res, rec = _encode(192, 160, 2, 2, intra_only=True, crf=None, qp=30, ctu64=False, slices=3, deblock=False, sao=False)
    _compare(host, res, rec)


def test_gpu_hevc_slices_intra_main10(host):
    res, rec = _encode(192, 160, 2, 2, bd=10, intra_only=True, crf=None, qp=27, slices=2)
    _compare(host, res, rec)


def test_gpu_hevc_slices_change_the_intra_prediction(host):
    """The rows under a slice edge are predicted without the samples above it: the stream is
    not the one-slice stream cut in two."""
    one, _ = _encode(192, 160, 1, 1, intra_only=True, crf=None, qp=30, ctu64=False, slices=1)
    two, _ = _encode(192, 160, 1, 1, intra_only=True, crf=None, qp=30, ctu64=False, slices=2)
    a = host.hevc_decode(one[0].bitstream)[0]
    b = host.hevc_decode(two[0].bitstream)[0]
    # CTB rows 0-2 (slice 0 under the rule r * 2 // 5) carry the same levels, row 3 does not
    assert np.array_equal(a["coef_y"][:96], b["coef_y"][:96])
    assert not np.array_equal(a["coef_y"][96:128], b["coef_y"][96:128])


# ---------------------------------------------------------------------------- P and B pictures

_PB = dict(crf=None, qp=28, bframes=3)
_ONE = {}


def _one_slice_bits(key, **kw):
    """bits per picture of the one-slice encode of the same configuration (computed once)"""
    if key not in _ONE:
        res, _ = _encode(192, 160, 9, 2, keep=False, **_PB, **kw)
        _ONE[key] = [list(r.bits) for r in res]
    return _ONE[key]


@pytest.mark.parametrize("wpp", [True, False])
@pytest.mark.parametrize("ctu64", [True, False])
def test_gpu_hevc_slices_p_b_match_decoder(host, wpp, ctu64):
    """AQ on (the default): cu_qp_delta is coded and hevc_qp_fixup restarts the predictor per
    slice.  Rate sanity against a degenerate boundary: every picture costs more than nothing and
    less than 1.5x its one-slice size."""
    res, rec = _encode(192, 160, 9, 2, wpp=wpp, ctu64=ctu64, slices=2, **_PB)
    _compare(host, res, rec)
    base = _one_slice_bits((wpp, ctu64), wpp=wpp, ctu64=ctu64)
    for b, r in enumerate(res):
        assert len(_slice_nals(r.bitstream)) == 2 * r.frames
        print(f"slot {b} wpp {wpp} ctu64 {ctu64}: bits S=2 {list(r.bits)} S=1 {base[b]}")
        for t, (two, one) in enumerate(zip(r.bits, base[b])):
            assert 0 < two < 1.5 * one, (b, t, two, one)


def test_gpu_hevc_slices_refs3_match_decoder(host):
    res, rec = _encode(192, 160, 9, 2, slices=2, refs=3, crf=None, qp=28, bframes=0)
    _compare(host, res, rec)


def test_gpu_hevc_slices_rdoq_match_decoder(host):
    res, rec = _encode(192, 160, 9, 2, slices=2, rdoq_level=2, **_PB)
    _compare(host, res, rec)


def test_gpu_hevc_slices_merge_refine_approximation(host):
    """merge_exact off: P pictures take the neighbour-vector passes (hevc_merge_refine)."""
    res, rec = _encode(192, 160, 5, 2, slices=2, merge_exact=False, refs=1, crf=None, qp=28, bframes=0)
    _compare(host, res, rec)


# ---------------------------------------------------------------------------- GPU entropy

@pytest.mark.parametrize("wpp", [True, False])
@pytest.mark.parametrize("S", [2, 3])
def test_gpu_hevc_slices_entropy_one_workgroup(host, S, wpp):
    """64 slots of 8 CTU rows: 64 x 8 waves, so the launcher codes each picture in one workgroup
    (rows in barrier-separated rounds; without WPP a wave per slice)."""
    out = {}
    for ent in ("gpu", "host"):
        res, _ = _encode(64, 256, 2, 64, entropy=ent, keep=False, seed=11, ctu64=False, wpp=wpp, slices=S)
        out[ent] = [r.bitstream for r in res]
    assert out["gpu"] == out["host"]
    assert len(host.hevc_decode(out["gpu"][0], False)) == 2
    assert len(_slice_nals(out["gpu"][63])) == 2 * S


@pytest.mark.parametrize("wpp", [True, False])
@pytest.mark.parametrize("S", [2, 3])
def test_gpu_hevc_slices_entropy_several_workgroups(host, S, wpp):
    """One slot of 12 CTU rows: with WPP the rows go to two workgroups of 6 rows -- two slices
    meet on the block edge (row 6), three slices start rows 4 and 8 inside the blocks."""
    out = {}
    for ent in ("gpu", "host"):
        res, _ = _encode(128, 384, 3, 1, entropy=ent, keep=False, seed=12, ctu64=False, wpp=wpp, slices=S)
        out[ent] = [r.bitstream for r in res]
    assert out["gpu"] == out["host"]
    assert len(host.hevc_decode(out["gpu"][0], False)) == 3


# ---------------------------------------------------------------------------- hevc_b_merge vs the model

B_SLOTS = 2
PASSES = 3


def _sliced_model(host, monkeypatch, case, S):
    """the model's passes with "same slice" added to its availability rule"""
    import test_gpu_hevc_merge_model as tm
    (wmb, hmb), ctu64 = case[0], case[3]
    sh = 2 if ctu64 else 1
    hctu = -(-hmb >> sh)
    base = hm.available

    def slice_of(by):
        return host.hevc_slice_of_row(by >> sh, S, hctu)

    def available(order, nx, ny, mx, my):
        return base(order, nx, ny, mx, my) and slice_of(ny) == slice_of(my)
    lam = host.table("lambda")[0]
    plain = tm._build_merge(case, lam)
    monkeypatch.setattr(hm, "available", available)
    sliced = tm._build_merge(case, lam)
    monkeypatch.setattr(hm, "available", base)
    return tm, plain, sliced


@pytest.mark.parametrize("bslice", [1, 0], ids=["B", "P"])
@pytest.mark.parametrize("ctu64", [0, 1], ids=["ctu32", "ctu64"])
def test_hevc_b_merge_with_slices_matches_model(host, monkeypatch, ctu64, bslice):
    """6x5 blocks, two slices (the second starts at block row 4 for both CTU sizes): motions,
    directions, costs and bits of every block after each of three passes."""
    S = 2
    case = ((6, 5), bslice, 1, ctu64, 5, 1, 900 + 2 * ctu64 + bslice)
    tm, plain, m = _sliced_model(host, monkeypatch, case, S)
    # the slice edge matters in this case (asserted on the model alone): some block decides otherwise
    assert any(not np.array_equal(m["slots"][b][it][0][k], plain["slots"][b][it][0][k])
               for b in range(B_SLOTS) for it in range(PASSES) for k in ("mvb", "dir", "cost"))
    (wmb, hmb) = case[0]
    d = tm._Dev()
    nmb, W, H = wmb * hmb, wmb * 16, hmb * 16
    t_src = d.up(m["src"])
    t_ref0 = d.up(m["refs0"][0])
    t_hp0 = d.planes(t_ref0, W, H)
    t_ref1 = d.up(m["ref1"])
    t_hp1 = d.planes(t_ref1, W, H)
    t_qp, t_aq = d.up(np.asarray(tm.QP, dtype=np.int32)), d.up(m["aq"])
    t_tdir, t_tmv = d.up(m["tdir"]), d.up(m["tmv"])
    mvb = [d.up(m["mvs"]), d.full((B_SLOTS, nmb, 4), tm.P_MV, "int16")]
    dirb = [d.up(m["dirs"]), d.full((B_SLOTS, nmb), tm.P_DIR, "uint8")]
    cost, bits = d.up(m["cost"]), d.up(m["bits"])
    for it in range(PASSES):
        i_, o_ = it % 2, (it + 1) % 2
        mvb[o_].fill_(tm.P_MV)
        dirb[o_].fill_(tm.P_DIR)
        d.hip.hevc_b(1, B_SLOTS, wmb, hmb, t_src.data_ptr(), t_ref0.data_ptr(),
                     t_ref1.data_ptr() if bslice else t_ref0.data_ptr(), t_hp0.data_ptr(),
                     t_hp1.data_ptr() if bslice else t_hp0.data_ptr(), 0, 0, 0, 0, 0, 0, t_tmv.data_ptr(), t_tdir.data_ptr(),
                     mvb[i_].data_ptr(), dirb[i_].data_ptr(), mvb[o_].data_ptr(), dirb[o_].data_ptr(), cost.data_ptr(),
                     bits.data_ptr(), t_qp.data_ptr(), t_aq.data_ptr(), d.stream, bslice, 5, ctu64, slices=S)
        d.sync()
        g_mv, g_dir, g_cost, g_bits = tm._np(mvb[o_]), tm._np(dirb[o_]), tm._np(cost), tm._np(bits)
        for b in range(B_SLOTS):
            out, _ = m["slots"][b][it]
            bad = np.flatnonzero((g_mv[b] != out["mvb"]).any(axis=1) | (g_dir[b] != out["dir"]) | (g_cost[b] != out["cost"])
                                 | (g_bits[b] != out["bits"]))
            assert bad.size == 0, (f"pass {it} slot {b} blocks {bad[:6]}", g_mv[b][bad[:6]], out["mvb"][bad[:6]],
                                   g_dir[b][bad[:6]], out["dir"][bad[:6]], g_cost[b][bad[:6]], out["cost"][bad[:6]])


# ---------------------------------------------------------------------------- GPU decode

def test_gpu_hevc_decoder_reads_sliced_streams(host):
    from govideocompressor_amd.models.hevc_decode_gpu import GpuHevcDecoder
    res, _ = _encode(200, 168, 6, 2, keep=False, seed=21, crf=27.0, slices=3)
    streams = [r.bitstream for r in res]
    dec = GpuHevcDecoder().decode(streams)
    for i, (s, d) in enumerate(zip(streams, dec)):
        pics = host.hevc_decode_full(s, True, False)
        ref = sorted((p for p in pics if p["display"] >= 0), key=lambda p: p["display"])
        assert d.frames == len(ref) == 6
        for t, p in enumerate(ref):
            x0, y0, w, h = p["crop_x"], p["crop_y"], p["width"], p["height"]
            for name, g in (("y", d.y), ("u", d.u), ("v", d.v)):
                sc = 0 if name == "y" else 1
                want = p[name][y0 >> sc:(y0 + h) >> sc, x0 >> sc:(x0 + w) >> sc]
                got = g[t].cpu().numpy().astype(np.uint16)
                assert np.array_equal(got, want), (i, t, name, int((got != want).sum()))
