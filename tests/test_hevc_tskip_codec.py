"""HEVC host layer with transform skip (x265 --tskip, ``HevcConfig.tskip``).

The PPS carries transform_skip_enabled_flag and every 4x4 TU codes transform_skip_flag first in
its residual_coding, from the picture's transform skip map (laid out like the packed levels'
sub-block map).  Random records with the bits planted on coded 4x4 TUs -- the luma PUs of
PART_NxN intra CUs, the chroma blocks of 8x8 intra and inter CUs, the chroma quarter TUs of split
16x16 inter CUs -- go through the host writer to the independent decoder, which must parse the
planted map and the written levels, and reconstruct a planted block as the numpy model's inverse
(tests/ref_models_hevc_tskip.py ``ts_residual``) says, bit for bit: the block's prediction is read
from a second stream in which only that block has no levels (what precedes it is unchanged, so
its reconstruction there is its prediction).
"""
import hashlib

import numpy as np
import pytest

import ref_models_hevc_tskip as ts
from govideocompressor_amd.utils.hevc_synth import (coded_4x4_tus, hide_signs_diag, pack_levels, random_gop_stream,
                                                    random_records, random_stream, tsmap_of)

W, H = 64, 128
# bit depth, ctu64, wpp, slices, sdh
CONFIGS = [(8, 0, 0, 1, 0), (10, 1, 1, 2, 0), (8, 1, 0, 2, 1), (10, 0, 1, 1, 1), (8, 0, 1, 2, 0), (10, 1, 0, 1, 0)]
KW = dict(nxn=0.6, tu_split=0.5, mv_pool=3, density=0.06, intra_in_p=0.3, sao=False)


def _cfg(bd, ctu64, wpp, slices, sdh, tskip=1):
    return dict(ctu64=ctu64, wpp=wpp, slices=slices, sdh=sdh, tu_inter_depth=1, tskip=tskip, sao=0)


def _chroma_qp(qp):
    tab = {30: 29, 31: 30, 32: 31, 33: 32, 34: 33, 35: 33, 36: 34, 37: 34, 38: 35, 39: 35, 40: 36, 41: 36, 42: 37, 43: 37}
    return qp if qp < 30 else (tab[qp] if qp <= 43 else qp - 6)


class Planter:
    """the ``tsmaps`` callback of the stream generators: makes the records diagonal-scan and sign
    data hiding consistent when asked, plants bits on about half of the coded 4x4 TUs and keeps what
    it did; ``blank`` = (picture, component, x, y) empties that one TU first"""

    def __init__(self, seed, sdh, blank=None, plant=True):
        self.rng = np.random.default_rng(seed)
        self.sdh, self.blank, self.plant = sdh, blank, plant
        self.planted, self.maps = {}, {}

    def __call__(self, d, r):
        ctu, cu, cy, cb, cr = r
        if self.sdh:  # every intra mode DC: all TUs scan diagonally, then the parity of every 4x4 group
            intra = cu[:, 0] == 0
            cu[intra, 1] = 1
            nxn = intra & ((cu[:, 3] & 8) != 0)
            cu[nxn, 4:8] = 1
            for pl in (cy, cb, cr):
                for y in range(0, pl.shape[0], 4):
                    for x in range(0, pl.shape[1], 4):
                        pl[y:y + 4, x:x + 4] = hide_signs_diag(pl[y:y + 4, x:x + 4])
        tus = coded_4x4_tus(*r)
        pick = [t for t in tus if self.rng.random() < 0.5] if self.plant else []
        if self.blank is not None and self.blank[0] == d:
            _, c, x, y = self.blank
            (cy, cb, cr)[c][y:y + 4, x:x + 4] = 0
            pick = [t for t in pick if t != (c, x, y)]
        self.planted[d] = pick
        self.maps[d] = tsmap_of(pick, W, H)
        return self.maps[d]


def _gop(host, cfgt, seed, **pk):
    bd = cfgt[0]
    pl = Planter(seed, cfgt[4], **pk)
    s, recs = random_gop_stream(host, W, H, 3, bframes=1, seed=seed, bit_depth=bd, host_cfg=_cfg(*cfgt), tsmaps=pl, **KW)
    return s, recs, pl


@pytest.mark.parametrize("cfgt", CONFIGS, ids=lambda c: "bd{}-ctu64_{}-wpp{}-s{}-sdh{}".format(*c))
def test_tskip_bits_and_reconstruction(host, cfgt):
    """I, B, P (display order): the planted maps and the levels come back, and planted blocks of
    every picture and kind reconstruct as the model says"""
    bd = cfgt[0]
    seed = 100 + sum(v << i for i, v in enumerate(cfgt))
    s, recs, pl = _gop(host, cfgt, seed)
    pics = host.hevc_decode(s, True)
    assert [p["slice_type"] for p in pics] == [2, 0, 1]
    kinds = set()
    for d, (p, r) in enumerate(zip(pics, recs)):
        assert np.array_equal(p["coef_y"], r[2]) and np.array_equal(p["coef_cb"], r[3]) and np.array_equal(p["coef_cr"], r[4])
        assert np.array_equal(p["tsmap"], pl.maps[d]), d
        assert len(pl.planted[d]) >= 4, (d, len(pl.planted[d]))
        # up to two planted blocks of each component in this picture
        for c in range(3):
            for (_, x, y) in [t for t in pl.planted[d] if t[0] == c][:2]:
                s0, _, _ = _gop(host, cfgt, seed, blank=(d, c, x, y))
                pred = host.hevc_decode(s0, True)[d]["yuv"[c]][y:y + 4, x:x + 4].astype(np.int64)
                lev = r[2 + c][y:y + 4, x:x + 4].astype(np.int64)
                qp = p["qp"] if c == 0 else _chroma_qp(p["qp"])
                want = np.clip(pred + ts.ts_residual(lev, bd, qp + 6 * (bd - 8)), 0, (1 << bd) - 1)
                assert np.array_equal(p["yuv"[c]][y:y + 4, x:x + 4], want), (d, c, x, y)
                kinds.add((c > 0, int(p["slice_type"])))
    assert {(False, 2), (True, 2), (True, 0), (True, 1)} <= kinds   # intra luma; chroma in I, B and P pictures


@pytest.mark.parametrize("cfgt", CONFIGS[:3], ids=lambda c: "bd{}-ctu64_{}-wpp{}-s{}-sdh{}".format(*c))
def test_tskip_flag_changes_the_reconstruction(host, cfgt):
    """the same records without planted bits decode to other samples exactly where bits were"""
    seed = 300 + cfgt[0]
    s1, recs, pl = _gop(host, cfgt, seed)
    s0, _, _ = _gop(host, cfgt, seed, plant=False)
    a, b = host.hevc_decode(s1, True)[0], host.hevc_decode(s0, True)[0]
    assert not b["tsmap"].any() and a["tsmap"].any()
    assert np.array_equal(a["coef_y"], b["coef_y"]) and not np.array_equal(a["y"], b["y"])


def test_tskip_packed_levels_same_bytes(host):
    """the packed-level writer (one picture and batch form) takes the map and codes the same bytes"""
    rng = np.random.default_rng(5)
    fp = dict(idr=0, poc=1, qp=30, slice_type=1)
    r = random_records(rng, W, H, pslice=True, **{k: v for k, v in KW.items() if k != "mv_pool"})
    tsm = tsmap_of(coded_4x4_tus(*r)[::2], W, H)
    assert tsm.any()
    for wpp in (0, 1):
        cfg = dict(width=W, height=H, **_cfg(8, 1, wpp, 2, 0))
        nal, _ = host.hevc_write_slice(cfg, fp, *r, tsmap=tsm)
        nz, off, lv = pack_levels(*r[2:])
        nal2, _ = host.hevc_write_slice_packed(cfg, fp, r[0], r[1], nz, off, lv, tsmap=tsm)
        assert nal == nal2
        two = host.hevc_write_slices_packed(cfg, [fp, fp], np.stack([r[0], r[0]]), np.stack([r[1], r[1]]), np.stack([nz, nz]),
                                            np.stack([off, off]), np.stack([lv, lv]), 2,
                                            tsmap=np.stack([tsm, np.zeros_like(tsm)]))
        assert two[0] == nal and two[1] == host.hevc_write_slice(cfg, fp, *r)[0] != nal
        subs = host.hevc_slice_substreams(cfg, fp, *r, tsmap=tsm)
        assert b"".join(subs) != b"".join(host.hevc_slice_substreams(cfg, fp, *r))


def test_tskip_refusals(host):
    rng = np.random.default_rng(6)
    fp = dict(idr=1, poc=0, qp=30, slice_type=2)
    r = random_records(rng, W, H, pslice=False, nxn=0.6, sao=False)
    ctu, cu, cy, cb, cr = r
    cfg = dict(width=W, height=H, tskip=1, sao=0)
    tus = coded_4x4_tus(*r)
    assert host.hevc_write_slice(cfg, fp, *r, tsmap=tsmap_of(tus, W, H))[0]
    # a map with the flag off
    with pytest.raises(RuntimeError, match="tskip"):
        host.hevc_write_slice(dict(cfg, tskip=0), fp, *r, tsmap=tsmap_of(tus[:1], W, H))
    with pytest.raises(RuntimeError, match="tskip"):
        nz, off, lv = pack_levels(cy, cb, cr)
        host.hevc_write_slice_packed(dict(cfg, tskip=0), fp, ctu, cu, nz, off, lv, tsmap=tsmap_of([], W, H))
    # a bit on an empty 4x4 TU
    c, x, y = tus[0]
    planes = [cy.copy(), cb.copy(), cr.copy()]
    planes[c][y:y + 4, x:x + 4] = 0
    with pytest.raises(RuntimeError, match="transform skip bit"):
        host.hevc_write_slice(cfg, fp, ctu, cu, *planes, tsmap=tsmap_of([(c, x, y)], W, H))
    # a bit inside a TU that is not 4x4: every CTB one 32x32 CU
    r32 = random_records(rng, W, H, pslice=False, force_split=0, density=0.3, sao=False)
    assert r32[2][:4, :4].any() or r32[2][:32, :32].any()
    for t in ((0, 0, 0), (1, 4, 4), (2, 12, 0)):
        with pytest.raises(RuntimeError, match="transform skip bit"):
            host.hevc_write_slice(cfg, fp, *r32, tsmap=tsmap_of([t], W, H))
    # a wrong-sized map
    with pytest.raises(RuntimeError, match="tsmap"):
        host.hevc_write_slice(cfg, fp, *r, tsmap=np.zeros(3, np.uint64))


def test_tskip_enabled_without_bits(host):
    """the PPS flag alone: every 4x4 TU codes a zero flag (other bytes than the default stream's),
    and the decoder reconstructs what the default stream does"""
    a, recs = random_stream(host, W, H, 2, seed=11, host_cfg=dict(tskip=1), nxn=0.6)
    b, _ = random_stream(host, W, H, 2, seed=11, nxn=0.6)
    assert a != b
    for p, q in zip(host.hevc_decode(a), host.hevc_decode(b)):
        assert np.array_equal(p["y"], q["y"]) and np.array_equal(p["u"], q["u"]) and not p["tsmap"].any()


# sha256 (first 16 hex digits) of the streams below as the writer produced them before it knew
# transform skip
GOLDEN = {(8, 0, 0, 1): ("8d752c17e3f92074", "3628b7f2a75e6019"), (10, 1, 1, 2): ("21e8cb66a12100ba", "09b61c1b665d9db4")}


@pytest.mark.parametrize("key", list(GOLDEN), ids=lambda k: "bd{}-ctu64_{}-wpp{}-s{}".format(*k))
def test_tskip_off_is_the_earlier_stream(host, key):
    bd, ctu64, wpp, sl = key
    for extra in ({}, dict(tskip=0)):
        s, _ = random_stream(host, 64, 128, 2, seed=7, bit_depth=bd, host_cfg=dict(ctu64=ctu64, wpp=wpp, slices=sl, **extra),
                             nxn=0.5)
        g, _ = random_gop_stream(host, 64, 128, 3, bframes=1, seed=9, bit_depth=bd,
                                 host_cfg=dict(ctu64=ctu64, wpp=wpp, slices=sl, tu_inter_depth=1, **extra), nxn=0.5,
                                 tu_split=0.5, mv_pool=3)
        assert (hashlib.sha256(s).hexdigest()[:16], hashlib.sha256(g).hexdigest()[:16]) == GOLDEN[key]
