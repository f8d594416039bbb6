"""Auto-variance AQ (aq_mode 2 / 3) through both encoders on small pictures: the streams stay
bit-exact against the independent CPU decoders, the GPU entropy coders equal the host writers,
the per-block QPs vary and are the model's, two encodes of a clip give the same bytes, and
aq_mode 1 / 0 are the default encoder / aq_strength 0."""
import numpy as np
import pytest

import ref_models as rm
import ref_models_aq_auto as am

pytestmark = pytest.mark.gpu


class _Calls:
    """Stands in for the encoder's kernel module and counts the AQ launches by name."""

    _NAMES = ("aq_offsets", "prep_aq", "aq_terms", "prep_aq_terms", "aq_auto_finish", "hevc_aq", "hevc_aq_terms",
              "hevc_aq_auto_finish")

    def __init__(self, hip):
        self._hip = hip
        self.n = dict.fromkeys(self._NAMES, 0)
        self.took = 0   # fused term launches that ran

    def __getattr__(self, name):
        fn = getattr(self._hip, name)
        if name not in self._NAMES:
            return fn

        def counted(*a, **k):
            self.n[name] += 1
            r = fn(*a, **k)
            if name == "prep_aq_terms":
                self.took += bool(r)
            return r
        return counted


def _h264_roundtrip(host, enc, res):
    for b, r in enumerate(res):
        pics = host.decode(r.bitstream)
        assert len(pics) == r.frames
        for t, pic in enumerate(pics):
            ry, ru, rv = (x[b].cpu().numpy() for x in enc.last_recon[t])
            assert np.array_equal(pic["y_coded"], ry), f"slot {b} frame {t}: luma mismatch"
            assert np.array_equal(pic["u_coded"], ru) and np.array_equal(pic["v_coded"], rv), f"slot {b} frame {t}: chroma"


@pytest.mark.parametrize("w,mode,cabac", [(176, 2, True), (176, 3, True), (180, 2, True), (180, 3, True), (176, 3, False)],
                         ids=["176-mode2", "176-mode3", "180-mode2-unfused", "180-mode3-unfused", "176-mode3-cavlc"])
def test_h264_auto_variance_encode(host, w, mode, cabac):
    import torch
    from govideocompressor_amd.models.h264_gpu import GpuH264Encoder, H264Params, synth_clip

    h, B, F = 144, 2, 4
    y, u, v = synth_clip(B, F, w, h, seed=11)
    out = {}
    for ent in ("cpu", "gpu"):
        enc = GpuH264Encoder(H264Params(width=w, height=h, crf=None, qp=28, aq_mode=mode, cabac=cabac), slots=B, entropy=ent)
        calls = enc.hip = _Calls(enc.hip)
        res = enc.encode(y, u, v, keep_recon=(ent == "gpu"))
        torch.cuda.synchronize()
        out[ent] = [bytes(r.bitstream) for r in res]
        assert calls.n["aq_auto_finish"] == F and calls.n["aq_offsets"] == 0 and calls.n["prep_aq"] == 0
        # a display width off the coded width is not the fused launch's
        assert calls.n["prep_aq_terms"] == F and calls.took == (F if w % 16 == 0 else 0)
        assert calls.n["aq_terms"] == F - calls.took
        if ent == "gpu":
            _h264_roundtrip(host, enc, res)
            assert enc._mbtree is None   # (fixed QP: the offsets below are variance AQ alone)
            e = rm.aq_energy(*rm.mb_blocks(*(x.cpu().numpy() for x in enc.src)))
            adj = am.aq_auto_adj(e, mode, 1.0)
            am.check_band(enc.aq.cpu().numpy(), am.offset_h264(adj), adj, f"h264 encode {w}x{h} mode {mode}")
            assert enc.aq.float().std() > 0.5
        enc.close()
    assert out["gpu"] == out["cpu"]
    for b in range(B):
        pics = host.decode(out["gpu"][b])
        assert any(np.unique(np.asarray(p["mb_qp"])).size > 3 for p in pics)


def _hevc_compare(host, res, rec):
    for b, r in enumerate(res):
        pics = host.hevc_decode(r.bitstream, False)
        assert len(pics) == r.frames
        for t, p in enumerate(pics):
            for k, name in enumerate(("y", "u", "v")):
                assert np.array_equal(rec[t][k][b].cpu().numpy().astype(np.uint16), p[name]), f"slot {b} pic {t} plane {name}"


@pytest.mark.parametrize("wpp", [True, False], ids=["wpp", "nowpp"])
@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("bd", [8, 10], ids=["main", "main10"])
def test_hevc_auto_variance_encode(host, bd, mode, wpp):
    from govideocompressor_amd.models.h264_gpu import synth_clip
    from govideocompressor_amd.models.hevc_gpu import GpuHevcEncoder, HevcParams

    w, h, B, F = 160, 128, 2, 4
    y, u, v = synth_clip(B, F, w, h, seed=5, bit_depth=bd)
    enc = GpuHevcEncoder(HevcParams(width=w, height=h, bit_depth=bd, wpp=wpp, aq_mode=mode), slots=B)
    calls = enc.hip = _Calls(enc.hip)
    assert enc.p.host_cfg()["cu_qp_delta"] == 1
    res = enc.encode(y, u, v, keep_recon=True)
    rec = enc.last_recon
    ctu_last = enc.ctu.cpu().numpy()  # records of the last picture in coding order
    assert calls.n["hevc_aq_terms"] == F and calls.n["hevc_aq_auto_finish"] == F and calls.n["hevc_aq"] == 0
    enc.close()
    _hevc_compare(host, res, rec)
    qps = set()
    for b, r in enumerate(res):
        pics = host.hevc_decode(r.bitstream)
        q = pics[r.order[-1]]["ctu"][:, 1].view(np.int8)
        assert np.array_equal(q, ctu_last[b][:, 1].view(np.int8))
        for p in pics:
            qps |= set(p["ctu"][:, 1].view(np.int8).tolist())
    assert len(qps) > 3


def test_hevc_strength_0_with_cutree_is_mode_independent():
    """AQ strength 0 with cutree on: the per-CTB QPs are cutree's alone, whatever aq_mode says."""
    from govideocompressor_amd.models.h264_gpu import synth_clip
    from govideocompressor_amd.models.hevc_gpu import GpuHevcEncoder, HevcParams

    w, h, B, F = 160, 128, 2, 4
    y, u, v = synth_clip(B, F, w, h, seed=5)
    out = []
    for kw in (dict(aq_strength=0.0), dict(aq_strength=0.0, aq_mode=2), dict(aq_mode=0), dict(aq_mode=3, aq_strength=0.0)):
        enc = GpuHevcEncoder(HevcParams(width=w, height=h, **kw), slots=B)
        calls = enc.hip = _Calls(enc.hip)
        assert enc.p.adaptive_qp()
        out.append([bytes(r.bitstream) for r in enc.encode(y, u, v)])
        assert calls.n["hevc_aq"] == F and calls.n["hevc_aq_terms"] == 0
        enc.close()
    assert out[1:] == out[:1] * 3


def _h264_bytes(y, u, v, w, h, **kw):
    from govideocompressor_amd.models.h264_gpu import GpuH264Encoder, H264Params

    enc = GpuH264Encoder(H264Params(width=w, height=h, **kw), slots=y.shape[0])
    out = [bytes(r.bitstream) for r in enc.encode(y, u, v)]
    enc.close()
    return out


def _hevc_bytes(y, u, v, w, h, **kw):
    from govideocompressor_amd.models.hevc_gpu import GpuHevcEncoder, HevcParams

    enc = GpuHevcEncoder(HevcParams(width=w, height=h, **kw), slots=y.shape[0])
    out = [bytes(r.bitstream) for r in enc.encode(y, u, v)]
    enc.close()
    return out


def test_h264_auto_variance_is_deterministic():
    """The same clip twice (CRF, MB-tree and the routed table on): the same bytes."""
    from govideocompressor_amd.models.h264_gpu import synth_clip

    y, u, v = synth_clip(2, 3, 640, 368, seed=21)
    a = _h264_bytes(y, u, v, 640, 368, aq_mode=2)
    assert a == _h264_bytes(y, u, v, 640, 368, aq_mode=2)
    assert a != _h264_bytes(y, u, v, 640, 368)


def test_hevc_auto_variance_is_deterministic():
    from govideocompressor_amd.models.h264_gpu import synth_clip

    y, u, v = synth_clip(2, 3, 640, 352, seed=21)
    a = _hevc_bytes(y, u, v, 640, 352, aq_mode=2)
    assert a == _hevc_bytes(y, u, v, 640, 352, aq_mode=2)
    assert a != _hevc_bytes(y, u, v, 640, 352)


def test_modes_1_and_0_are_what_they_were():
    """aq_mode 1 gives the bytes of the default-constructed parameters, aq_mode 0 those of
    aq_strength 0; 2 and 3 give others."""
    from govideocompressor_amd.models.h264_gpu import synth_clip

    y, u, v = synth_clip(2, 4, 176, 144, seed=11)
    for fn, (w, h) in ((_h264_bytes, (176, 144)), (_hevc_bytes, (160, 128))):
        if fn is _hevc_bytes:
            y, u, v = synth_clip(2, 4, w, h, seed=5)
        default = fn(y, u, v, w, h)
        assert fn(y, u, v, w, h, aq_mode=1) == default
        off = fn(y, u, v, w, h, aq_strength=0.0)
        assert fn(y, u, v, w, h, aq_mode=0) == off and off != default
        m2, m3 = fn(y, u, v, w, h, aq_mode=2), fn(y, u, v, w, h, aq_mode=3)
        assert m2 != default and m3 != default and m2 != m3
