"""HevcParams.rdoq_level 1 / 2 (x265 --rdoq-level) through whole encodes: 128x96, 2 slots, 5
pictures at fixed QP 22 and 30 -- intra-only, P and B pictures, Main and Main 10, 32x32 CTBs and
64x64 CTUs, the inter residual quadtree, sign data hiding and adaptive QP.  RDOQ has no syntax of
its own, so every case must keep what any encode keeps: the GPU reconstruction equals what the
independent CPU decoder decodes, the GPU entropy coder writes the host writer's bytes, and a
second encode repeats the first; and its bitstream differs from the one without RDOQ.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, F, B = 128, 96, 5, 2

_GOP = {"i": dict(intra_only=True), "p": dict(bframes=0), "b": dict(bframes=1), "b3": dict(bframes=3)}
# (id, rdoq_level, qp, bit depth, GOP, further parameters); aq_strength 0 = one QP per picture
CASES = [
    ("i-l1-qp22-bd8-ctu64", 1, 22, 8, "i", dict(ctu64=True, aq_strength=0.0)),
    ("i-l2-qp30-bd10-ctu32", 2, 30, 10, "i", dict(ctu64=False, aq_strength=0.0)),
    ("p-l2-qp22-bd8-ctu32", 2, 22, 8, "p", dict(ctu64=False, aq_strength=0.0)),
    ("p-l1-qp30-bd10-ctu64", 1, 30, 10, "p", dict(ctu64=True, aq_strength=0.0)),
    ("b-l2-qp30-bd8-ctu64", 2, 30, 8, "b", dict(ctu64=True, aq_strength=0.0)),
    ("b3-l1-qp22-bd10-ctu32", 1, 22, 10, "b3", dict(ctu64=False, aq_strength=0.0)),
    ("tu-l2-qp22-bd8-ctu64", 2, 22, 8, "b", dict(ctu64=True, aq_strength=0.0, tu_inter_depth=1)),
    ("tu-l1-qp30-bd10-ctu32", 1, 30, 10, "p", dict(ctu64=False, aq_strength=0.0, tu_inter_depth=1)),
    ("sdh-l1-qp22-bd8-ctu64", 1, 22, 8, "b", dict(ctu64=True, aq_strength=0.0, sdh=True)),
    ("sdh-l2-qp30-bd10-ctu32", 2, 30, 10, "i", dict(ctu64=False, aq_strength=0.0, sdh=True)),
    ("aq-l2-qp30-bd8-ctu64", 2, 30, 8, "b", dict(ctu64=True, aq_strength=1.0)),
    ("aq-sdh-tu-l1-qp22-bd10-ctu32", 1, 22, 10, "b", dict(ctu64=False, aq_strength=1.0, sdh=True, tu_inter_depth=1)),
]


def _clip(bd):
    from govideocompressor_amd.models.h264_gpu import synth_clip
    return synth_clip(B, F, W, H, seed=7, bit_depth=bd)


def _params(bd, qp, gop, kw, **rdoq):
    from govideocompressor_amd.models.hevc_gpu import HevcParams
    return HevcParams(width=W, height=H, bit_depth=bd, crf=None, qp=qp, **_GOP[gop], **kw, **rdoq)


def _streams(params, clip, entropy, twice=False):
    from govideocompressor_amd.models.hevc_gpu import GpuHevcEncoder
    enc = GpuHevcEncoder(params, slots=B, entropy=entropy)
    res = enc.encode(*clip, keep_recon=True)
    rec = [[pl.cpu().numpy().astype(np.uint16) for pl in pic] for pic in enc.last_recon]
    again = [r.bitstream for r in enc.encode(*clip)] if twice else None
    enc.close()
    return res, rec, again


@pytest.mark.parametrize("name,level,qp,bd,gop,kw", CASES, ids=[c[0] for c in CASES])
def test_rdoq_encode(host, name, level, qp, bd, gop, kw):
    clip = _clip(bd)
    p = _params(bd, qp, gop, kw, rdoq_level=level)
    assert p.adaptive_qp() == (kw["aq_strength"] > 0)
    res, rec, again = _streams(p, clip, "gpu", twice=True)
    for b, r in enumerate(res):  # the reconstruction is the decoder's
        pics = host.hevc_decode(r.bitstream, False)
        assert len(pics) == r.frames == F
        for t, pic in enumerate(pics):
            for k, plane in enumerate(("y", "u", "v")):
                assert np.array_equal(rec[t][k][b], pic[plane]), (name, b, t, plane)
    streams = [r.bitstream for r in res]
    assert again == streams, "a second encode gives other bytes"
    assert [r.bitstream for r in _streams(p, clip, "host")[0]] == streams, "GPU entropy coder != host writer"
    plain = [r.bitstream for r in _streams(_params(bd, qp, gop, kw), clip, "gpu")[0]]
    assert all(a != b for a, b in zip(plain, streams)), "RDOQ left a slot's bitstream unchanged"


def test_rdoq_level_0_is_the_encoder_without_the_field():
    clip = _clip(8)
    kw = dict(ctu64=True, aq_strength=1.0, sdh=True, tu_inter_depth=1)
    named = _streams(_params(8, 26, "b", kw, rdoq_level=0, rdoq_lambda=1.5), clip, "gpu")[0]
    plain = _streams(_params(8, 26, "b", kw), clip, "gpu")[0]
    assert [r.bitstream for r in named] == [r.bitstream for r in plain]


def test_rdoq_lambda_changes_the_stream():
    clip = _clip(8)
    kw = dict(ctu64=True, aq_strength=0.0)
    s = {lam: [r.bitstream for r in _streams(_params(8, 26, "p", kw, rdoq_level=2, rdoq_lambda=lam), clip, "gpu")[0]]
         for lam in (0.5, 1.5)}
    assert all(a != b for a, b in zip(s[0.5], s[1.5]))
    assert sum(map(len, s[1.5])) < sum(map(len, s[0.5]))  # a dearer bit buys fewer of them
