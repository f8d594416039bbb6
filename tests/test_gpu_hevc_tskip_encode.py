"""HevcParams.tskip (transform skip for 4x4 TUs, csrc/kernels/hevc_tskip.h) through whole encodes of
the screen generator (utils/screen_synth.py): 128x96 with 64x64 CTUs (partial CTUs on the bottom)
and 96x64 with 32x32 CTBs, 2 or 3 slots, 5 pictures (I, P, B) at a fixed QP, Main and Main 10, and
one run each with sign data hiding, RDOQ level 2, rd_cbf and two slices.  Every case keeps what
any encode keeps -- the GPU reconstruction is what the independent CPU decoder and the GPU decoder
decode, the GPU entropy coder writes the host writer's bytes, a second encode repeats the first --
and codes 4x4 TUs of all three kinds with the flag set (``enc.stats["tskip_tus"]``: intra luma,
intra chroma, inter chroma).  Then: the knob off is the default encoder; a gradient-only slot codes
the same beside a screen slot as alone; and a smooth clip after a screen clip on one encoder
gives a fresh encoder's bytes (no stale map).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = 5
# the 8x8 inter CUs (whose chroma TUs are 4x4) wherever they pay at all
BASE = dict(crf=None, qp=26, bframes=1, aq_strength=0.0, inter8=True, inter8_overhead=0, inter8_min_satd=0)
# (id, width, height, slots, bit depth, further parameters)
CASES = [
    ("ctu64-bd8", 128, 96, 2, 8, dict(ctu64=True)),
    ("ctu32-bd8", 96, 64, 3, 8, dict(ctu64=False)),
    ("ctu64-bd10", 128, 96, 3, 10, dict(ctu64=True)),
    ("ctu32-bd10", 96, 64, 2, 10, dict(ctu64=False)),
    ("sdh-ctu64-bd8", 128, 96, 2, 8, dict(ctu64=True, sdh=True)),
    ("rdoq2-ctu32-bd8", 96, 64, 2, 8, dict(ctu64=False, rdoq_level=2)),
    ("rdcbf-ctu64-bd10", 128, 96, 2, 10, dict(ctu64=True, rd_cbf=True)),
    ("slices2-ctu64-bd8", 128, 96, 2, 8, dict(ctu64=True, slices=2)),
    ("slices2-ctu32-bd10", 96, 64, 2, 10, dict(ctu64=False, slices=2, sdh=True)),
]


def _clip(w, h, slots, bd, seed=3, **kw):
    from govideocompressor_amd.utils.screen_synth import screen_clip
    return screen_clip(slots, F, w, h, seed=seed, bit_depth=bd, **kw)


def _params(w, h, bd, kw, **more):
    from govideocompressor_amd.models.hevc_gpu import HevcParams
    return HevcParams(width=w, height=h, bit_depth=bd, **{**BASE, **kw, **more})


def _streams(params, clip, entropy, twice=False):
    from govideocompressor_amd.models.hevc_gpu import GpuHevcEncoder
    enc = GpuHevcEncoder(params, slots=clip[0].shape[0], entropy=entropy)
    res = enc.encode(*clip, keep_recon=True)
    rec = [[pl.cpu().numpy().astype(np.uint16) for pl in pic] for pic in enc.last_recon]
    stats = dict(enc.stats)
    again = [r.bitstream for r in enc.encode(*clip)] if twice else None
    enc.close()
    return res, rec, again, stats


@pytest.mark.parametrize("name,w,h,slots,bd,kw", CASES, ids=[c[0] for c in CASES])
def test_tskip_encode(host, name, w, h, slots, bd, kw):
    from govideocompressor_amd.models.hevc_decode_gpu import GpuHevcDecoder
    clip = _clip(w, h, slots, bd)
    p = _params(w, h, bd, kw, tskip=True)
    res, rec, again, stats = _streams(p, clip, "gpu", twice=True)
    print(name, "tskip_tus (intra luma, intra chroma, inter chroma)", stats.get("tskip_tus"),
          "bytes", [len(r.bitstream) for r in res])
    streams = [r.bitstream for r in res]
    gdec = GpuHevcDecoder().decode(streams)
    for b, r in enumerate(res):  # the reconstruction is both decoders'
        pics = host.hevc_decode(r.bitstream, False)
        assert len(pics) == r.frames == F
        assert sorted(pic["slice_type"] for pic in pics) == [0, 0, 1, 1, 2]
        for t, pic in enumerate(pics):
            for k, plane in enumerate(("y", "u", "v")):
                assert np.array_equal(rec[t][k][b], pic[plane]), (name, b, t, plane)
                got = (gdec[b].y, gdec[b].u, gdec[b].v)[k][t].cpu().numpy().astype(np.uint16)
                assert np.array_equal(got, pic[plane][:h >> (k > 0), :w >> (k > 0)]), (name, "GPU decoder", b, t, plane)
        assert any(pic["tsmap"].any() for pic in pics)
    assert again == streams, "a second encode gives other bytes"
    hres, _, _, hstats = _streams(p, clip, "host")
    assert [r.bitstream for r in hres] == streams, "GPU entropy coder != host writer"
    ts = stats["tskip_tus"]
    assert len(ts) == 3 and all(v > 0 for v in ts), ts
    assert hstats["tskip_tus"] == ts


def test_tskip_off_is_the_default_encoder():
    for w, h, bd, kw in ((128, 96, 8, dict(ctu64=True)), (96, 64, 10, dict(ctu64=False, sdh=True))):
        clip = _clip(w, h, 2, bd)
        plain, _, _, stats = _streams(_params(w, h, bd, kw), clip, "gpu")
        assert "tskip_tus" not in stats
        for lam in (0.25, 4.0):
            named = _streams(_params(w, h, bd, kw, tskip=False, tskip_lambda=lam), clip, "gpu")[0]
            assert [r.bitstream for r in named] == [r.bitstream for r in plain]
        on = _streams(_params(w, h, bd, kw, tskip=True), clip, "gpu")[0]
        assert all(a.bitstream != b.bitstream for a, b in zip(on, plain))


def test_gradient_slot_is_isolated_from_a_screen_slot():
    """slot 1 shows panels only: its stream does not depend on slot 0 being screen content or not"""
    w, h = 128, 96
    p = _params(w, h, 8, dict(ctu64=True), tskip=True)
    beside = _streams(p, _clip(w, h, 2, 8, plain_slots=(1,)), "gpu")
    alone = _streams(p, _clip(w, h, 2, 8, plain_slots=(0, 1)), "gpu")
    assert beside[0][1].bitstream == alone[0][1].bitstream
    assert beside[0][0].bitstream != alone[0][0].bitstream
    assert all(v > 0 for v in beside[3]["tskip_tus"])


def test_no_stale_map_after_a_screen_clip():
    from govideocompressor_amd.models.hevc_gpu import GpuHevcEncoder
    w, h = 96, 64
    for entropy in ("gpu", "host"):
        p = _params(w, h, 8, dict(ctu64=False), tskip=True)
        screen, smooth = _clip(w, h, 2, 8), _clip(w, h, 2, 8, seed=4, plain_slots=(0, 1))
        enc = GpuHevcEncoder(p, slots=2, entropy=entropy)
        first = enc.encode(*screen)
        assert all(v > 0 for v in enc.stats["tskip_tus"])
        second = [r.bitstream for r in enc.encode(*smooth)]
        enc.close()
        fresh = [r.bitstream for r in _streams(p, smooth, entropy)[0]]
        assert second == fresh and [r.bitstream for r in first] != second
