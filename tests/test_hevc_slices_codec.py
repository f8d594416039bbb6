"""HEVC host layer with several slices per picture (x265 --slices, ``HevcConfig.slices``).

A picture is ``slices`` independent slices of whole CTU rows (CTU row r lies in slice
r * slices // rows), one NAL each.  Nothing is predicted across a slice edge: the writer's
neighbour availability, the SAO merge-up candidate, the CABAC contexts and the QP predictor
all restart, and with WPP a slice's first row neither syncs from nor waits for the row above.
The independent decoder is the oracle: what it parses must be the records that were written.
"""
import numpy as np
import pytest

from govideocompressor_amd.segment import mp4_hevc
from govideocompressor_amd.utils.hevc_synth import expected_ctb_qps, random_gop_stream, random_records, random_stream


def _norm_sao(c):
    c = c.copy()
    for t in c:
        off = t[10:22].view(np.int8).reshape(3, 4).copy()
        for ci in range(3):
            typ = t[2 + (1 if ci else 0)]
            if typ != 1:
                t[6 + ci] = 0
            if typ == 0:
                off[ci] = 0
        for k in range(2):
            if t[2 + k] != 2:
                t[4 + k] = 0
        t[10:22] = off.reshape(-1).view(np.uint8)
    return c[:, 2:22]


def _check_records(pics, recs, ctu64=0, motion=True):
    assert len(pics) == len(recs)
    for p, (ctu, cu, cy, cb, cr) in zip(pics, recs):
        assert np.array_equal(p["coef_y"], cy) and np.array_equal(p["coef_cb"], cb) and np.array_equal(p["coef_cr"], cr)
        assert np.array_equal(p["ctu"][:, 0], ctu[:, 0])                       # CU tree
        # SAO: a 64x64 CTU codes the parameters of its first 32x32 record block
        wc = cy.shape[1] // 32
        first = np.array([not ctu64 or (i % wc) % 2 == 0 and (i // wc) % 2 == 0 for i in range(len(ctu))])
        assert np.array_equal(_norm_sao(p["ctu"])[first], _norm_sao(ctu)[first])
        assert np.array_equal(p["cu"][:, 0], cu[:, 0])                         # intra / inter
        assert np.array_equal(p["cu"][:, 1], np.where(cu[:, 0] == 0, cu[:, 1], 0))  # intra modes
        if motion:
            inter = cu[:, 0] == 1
            assert np.array_equal(p["cu"][inter, 4:8], cu[inter, 4:8])         # vectors


def _vcl(stream):
    return [n for n in mp4_hevc.split_nals(stream) if ((n[0] >> 1) & 0x3F) < 32]


def _ctu_rows(h, ctu64):
    return -(-h // (64 if ctu64 else 32))


# heights with unequal slices and a partial last CTU row (160 = 2.5 rows of 64)
@pytest.mark.parametrize("w,h", [(96, 160), (192, 160)])
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("ctu64", [0, 1])
@pytest.mark.parametrize("wpp", [0, 1])
@pytest.mark.parametrize("S", [2, 3])
def test_hevc_slices_roundtrip(host, S, wpp, ctu64, bd, w, h):
    cfg = dict(slices=S, wpp=wpp, ctu64=ctu64)
    s, recs = random_stream(host, w, h, 3, seed=11 * S + 3 * wpp + ctu64 + bd, bit_depth=bd, host_cfg=cfg,
                            mv_pool=3, uniform64=0.3 if ctu64 else 0.0)
    _check_records(host.hevc_decode(s), recs, ctu64)
    assert len(_vcl(s)) == 3 * S


@pytest.mark.parametrize("w,h,ctu64,wpp", [(96, 160, 0, 0), (96, 160, 0, 1), (128, 192, 1, 1), (32, 128, 0, 1),
                                           (32, 128, 0, 0), (64, 256, 1, 0), (64, 256, 1, 1)])
def test_hevc_one_slice_per_ctu_row(host, w, h, ctu64, wpp):
    """S equal to the CTU-row count (every row its own slice: no entry points, no sync), also
    on pictures one CTU wide."""
    S = _ctu_rows(h, ctu64)
    s, recs = random_stream(host, w, h, 2, seed=5 + S + wpp, host_cfg=dict(slices=S, wpp=wpp, ctu64=ctu64), mv_pool=2)
    _check_records(host.hevc_decode(s), recs, ctu64)
    assert len(_vcl(s)) == 2 * S
    with pytest.raises(RuntimeError, match="slices"):
        random_stream(host, w, h, 1, host_cfg=dict(slices=S + 1, wpp=wpp, ctu64=ctu64))


@pytest.mark.parametrize("wpp", [0, 1])
@pytest.mark.parametrize("S", [2, 3])
def test_hevc_slices_cu_qp_delta(host, S, wpp):
    """qPY_PREV restarts at the slice QP at each slice's first CTU (and, with WPP, every row)."""
    w, h = 96, 160
    s, recs = random_stream(host, w, h, 3, seed=23 + S + wpp, qp_spread=12, density=0.02,
                            host_cfg=dict(cu_qp_delta=1, wpp=wpp, slices=S))
    pics = host.hevc_decode(s, False)
    assert len(pics) == 3
    for p, (ctu, cu, cy, cb, cr) in zip(pics, recs):
        assert np.array_equal(p["coef_y"], cy) and np.array_equal(p["coef_cb"], cb) and np.array_equal(p["coef_cr"], cr)
        want = expected_ctb_qps(ctu, cy, cb, cr, p["qp"], bool(wpp), slices=S)
        assert np.array_equal(p["ctu"][:, 1].view(np.int8).astype(np.int32), want)


@pytest.mark.parametrize("S", [2, 3])
def test_hevc_slices_qp_predictor_restarts(host, S):
    """Without WPP: a slice whose first CTB has no coded level takes the slice QP there, not the
    QpY of the last CTB of the slice above (an intra picture with those CTBs' levels cleared)."""
    w, h, qp = 96, 160, 30
    rng = np.random.default_rng(90 + S)
    ctu, cu, cy, cb, cr = random_records(rng, w, h, pslice=False, ctb_qp=(qp, 12))
    hc, wc = h // 32, w // 32
    starts = [r for r in range(1, hc) if r * S // hc != (r - 1) * S // hc]
    assert len(starts) == S - 1
    for r in starts:
        cy[r * 32:r * 32 + 32, :32] = 0
        cb[r * 16:r * 16 + 16, :16] = 0
        cr[r * 16:r * 16 + 16, :16] = 0
    cfg = dict(width=w, height=h, cu_qp_delta=1, slices=S)
    nal, _ = host.hevc_write_slice(cfg, dict(idr=1, poc=0, qp=qp, slice_type=2), ctu, cu, cy, cb, cr)
    p = host.hevc_decode(host.hevc_parameter_sets(cfg) + nal, False)[0]
    got = p["ctu"][:, 1].view(np.int8).astype(np.int32)
    assert np.array_equal(got, expected_ctb_qps(ctu, cy, cb, cr, qp, False, slices=S))
    assert all(got[r * wc] == qp for r in starts)
    assert not np.array_equal(got, expected_ctb_qps(ctu, cy, cb, cr, qp, False))   # the one-slice rule differs


@pytest.mark.parametrize("ctu64,wpp", [(0, 0), (0, 1), (1, 1)])
def test_hevc_slices_b_gop(host, ctu64, wpp):
    """B GOP with TMVP, five merge candidates and several list-0 pictures, two slices: every
    direction, refIdx and vector comes back."""
    s, recs = random_gop_stream(host, 128, 160, 9, bframes=3, seed=3 + ctu64 + wpp, tmvp=True, mv_pool=3,
                                intra_in_p=0.05, density=0.02, pyramid=True, refs=3,
                                host_cfg=dict(max_merge=5, wpp=wpp, ctu64=ctu64, slices=2, threads=2))
    pics = host.hevc_decode(s)
    assert len(pics) == 9 and len(_vcl(s)) == 18
    for d, (p, (ctu, cu, cy, cb, cr)) in enumerate(zip(pics, recs)):
        assert p["poc"] == d
        assert np.array_equal(p["coef_y"], cy) and np.array_equal(p["coef_cb"], cb) and np.array_equal(p["coef_cr"], cr)
        assert np.array_equal(p["cu"][:, 0], cu[:, 0])
        inter = cu[:, 0] == 1
        dirs = np.where(cu[:, 12] == 0, 1, cu[:, 12])
        assert np.array_equal(p["cu"][inter, 12], dirs[inter])
        assert np.array_equal(p["cu"][inter, 4:12], cu[inter, 4:12])
        assert np.array_equal(p["cu"][inter, 13:15], cu[inter, 13:15])


@pytest.mark.parametrize("S,ctu64", [(2, 0), (3, 1), (5, 0)])
def test_hevc_slices_threaded_writer_same_bytes(host, S, ctu64):
    a, _ = random_stream(host, 160, 320, 3, seed=40, host_cfg=dict(wpp=1, threads=1, slices=S, ctu64=ctu64))
    b, _ = random_stream(host, 160, 320, 3, seed=40, host_cfg=dict(wpp=1, threads=4, slices=S, ctu64=ctu64))
    assert a == b


@pytest.mark.parametrize("wpp", [0, 1])
def test_hevc_one_slice_is_the_default_stream(host, wpp):
    a, _ = random_stream(host, 96, 160, 3, seed=41, host_cfg=dict(wpp=wpp))
    b, _ = random_stream(host, 96, 160, 3, seed=41, host_cfg=dict(wpp=wpp, slices=1))
    assert a == b


@pytest.mark.parametrize("S", [2, 3])
def test_hevc_slices_nal_structure(host, S):
    s1, _ = random_stream(host, 96, 160, 3, seed=42, host_cfg=dict(wpp=1))
    s, _ = random_stream(host, 96, 160, 3, seed=42, host_cfg=dict(wpp=1, slices=S))
    vcl = _vcl(s)
    assert len(vcl) == 3 * S and len(_vcl(s1)) == 3
    first = [bool(n[2] & 0x80) for n in vcl]          # first_slice_segment_in_pic_flag
    assert first == ([True] + [False] * (S - 1)) * 3
    pps = [n for n in mp4_hevc.split_nals(s) if ((n[0] >> 1) & 0x3F) == 34]
    pps1 = [n for n in mp4_hevc.split_nals(s1) if ((n[0] >> 1) & 0x3F) == 34]
    assert len(pps) == len(pps1) == 1 and pps[0] != pps1[0]   # pps_loop_filter_across_slices_enabled_flag
    # the filters off: no slice_loop_filter_across_slices_enabled_flag to carry, still decodable
    s, recs = random_stream(host, 96, 160, 2, seed=43, host_cfg=dict(slices=S, sao=0, deblock=0), sao=False)
    pics = host.hevc_decode(s)
    assert len(pics) == 2 and np.array_equal(pics[1]["coef_y"], recs[1][2])


@pytest.mark.parametrize("wpp,ctu64,w,h,S", [(1, 1, 192, 160, 2), (0, 1, 192, 160, 3), (1, 0, 160, 160, 3),
                                             (0, 0, 96, 160, 2), (1, 0, 96, 160, 5), (0, 0, 96, 160, 5)])
def test_hevc_assemble_slices_matches_writer_with_slices(host, wpp, ctu64, w, h, S):
    """The GPU entropy path's host half rebuilds the writer's slice NALs from the writer's own
    substreams: one per CTU row with WPP (each slice lists the entry points of its own rows),
    else one per slice."""
    rng = np.random.default_rng(50 + wpp + 2 * ctu64 + S)
    cfg = dict(width=w, height=h, wpp=wpp, ctu64=ctu64, cu_qp_delta=1, slices=S)
    frames = [dict(idr=1, poc=0, qp=30, slice_type=2), dict(idr=0, poc=1, qp=31, slice_type=1)]
    recs = [random_records(rng, w, h, pslice=False, ctb_qp=(30, 4)),
            random_records(rng, w, h, pslice=True, ctb_qp=(31, 4))]
    data, offs, sizes, want = bytearray(), [], [], []
    for fp, r in zip(frames, recs):
        want.append(host.hevc_write_slice(cfg, fp, *r)[0])
        subs = host.hevc_slice_substreams(cfg, fp, *r)
        assert len(subs) == (_ctu_rows(h, ctu64) if wpp else S)
        for sb in subs:
            offs.append(len(data))
            sizes.append(len(sb))
            data += sb + bytes(-len(sb) % 16)
    offs.append(len(data))
    got = host.hevc_assemble_slices(cfg, frames, np.frombuffer(bytes(data), np.uint8), np.array(offs, np.uint64),
                                    np.array(sizes, np.uint32), np.zeros(len(sizes), np.int32), 2)
    assert got == want
    assert all(len(_vcl(n)) == S for n in got)


def test_hevc_slices_packed_levels_and_stats(host):
    """The packed-level writer codes the same bytes, and the picture statistics are sums over
    the slices (as many CUs as the one-slice picture has)."""
    from govideocompressor_amd.utils.hevc_synth import pack_levels
    rng = np.random.default_rng(60)
    w, h = 96, 160
    fp = dict(idr=0, poc=1, qp=30, slice_type=1)
    r = random_records(rng, w, h, pslice=True)
    for wpp in (0, 1):
        cfg = dict(width=w, height=h, wpp=wpp, slices=3)
        nal, st = host.hevc_write_slice(cfg, fp, *r)
        nz, off, lv = pack_levels(*r[2:])
        nal2, st2 = host.hevc_write_slice_packed(cfg, fp, r[0], r[1], nz, off, lv)
        assert nal == nal2
        _, st1 = host.hevc_write_slice(dict(width=w, height=h, wpp=wpp), fp, *r)
        n1 = st1["intra_cus"] + st1["inter_cus"] + st1["skip_cus"]
        assert st["intra_cus"] + st["inter_cus"] + st["skip_cus"] == n1 > 0
        assert st["intra_cus"] == st1["intra_cus"] and st["bins"] == st2["bins"] and st["bytes"] == len(nal)


def test_hevc_slices_mp4_roundtrip(host):
    """One sample per picture (the slices of a picture stay together), the same display order
    as the one-slice stream, and demux returns the stream."""
    kw = dict(bframes=3, seed=8, tmvp=True, mv_pool=3, density=0.02, pyramid=True)
    s, _ = random_gop_stream(host, 128, 160, 9, host_cfg=dict(wpp=1, slices=2), **kw)
    s1, _ = random_gop_stream(host, 128, 160, 9, host_cfg=dict(wpp=1), **kw)
    m = mp4_hevc.mux(s, 25.0)
    i = m.index(b"stsz") + 4
    assert int.from_bytes(m[i + 8:i + 12], "big") == 9     # sample count
    assert mp4_hevc.display_order(s) == mp4_hevc.display_order(s1)
    back = mp4_hevc.demux(m)
    assert mp4_hevc.split_nals(back) == mp4_hevc.split_nals(s)
    a, b = host.hevc_decode(back), host.hevc_decode(s)
    assert len(a) == len(b) == 9
    for p, q in zip(a, b):
        assert np.array_equal(p["y"], q["y"]) and np.array_equal(p["u"], q["u"])


def test_hevc_slices_split_pieces_decode_like_the_whole(host):
    def disp(pics):
        return sorted(pics, key=lambda p: p["poc"])
    parts = [random_stream(host, 96, 160, 4, seed=70 + k, intra_in_p=0.2, mv_range=8,
                           host_cfg=dict(slices=3, wpp=k & 1))[0] for k in range(3)]
    whole = b"".join(parts)
    pieces = host.hevc_split_pieces(whole, 1)
    assert len(pieces) == 3
    got = [p for pc in pieces for p in disp(host.hevc_decode_full(pc, True, False))]
    ref = [p for pc in parts for p in disp(host.hevc_decode_full(pc, True, False))]
    assert len(got) == len(ref) == 12
    for p, q in zip(got, ref):
        assert np.array_equal(p["y"], q["y"])
    # the general decoder and the writer's own decoder agree on a sliced stream
    for p, q in zip(ref[:4], host.hevc_decode(parts[0])):
        assert np.array_equal(p["y"], q["y"])
