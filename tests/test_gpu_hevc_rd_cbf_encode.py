"""HevcParams.rd_cbf (inter TUs keep their levels only when they pay for themselves,
csrc/kernels/hevc_rdcbf.h) through whole encodes: 128x96, 2 slots, 5 pictures at fixed QP 22 and
30 -- P, 1 B and 3 B GOPs, Main and Main 10, 32x32 CTBs and 64x64 CTUs, the inter residual
quadtree, sign data hiding, adaptive QP (the table lookup per CTB), RDOQ levels 1 and 2, weighted
B prediction on a fade, three list-0 references and the 8x8 inter CUs with their 4x4 chroma TUs.
The check has no syntax of its own, so every case must keep what any encode keeps: the GPU
reconstruction equals what the independent CPU decoder decodes, the GPU entropy coder writes the
host writer's bytes, and a second encode repeats the first; and every slot's bitstream differs
from the one without the knob.  Then: the knob off is the default whatever the lambda; a static
clip under noise gets smaller, the more the larger the lambda, and keeps its slots apart; an
intra-only encode does not change.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, F, B = 128, 96, 5, 2

_GOP = {"i": dict(intra_only=True), "p": dict(bframes=0), "b": dict(bframes=1), "b3": dict(bframes=3)}
# (id, qp, bit depth, GOP, clip, further parameters); aq_strength 0 = one QP per picture
CASES = [
    ("p-qp22-bd8-ctu32", 22, 8, "p", "synth", dict(ctu64=False, aq_strength=0.0)),
    ("p-qp30-bd10-ctu64", 30, 10, "p", "synth", dict(ctu64=True, aq_strength=0.0)),
    ("b-qp30-bd8-ctu64", 30, 8, "b", "synth", dict(ctu64=True, aq_strength=0.0)),
    ("b3-qp22-bd10-ctu32", 22, 10, "b3", "synth", dict(ctu64=False, aq_strength=0.0)),
    ("tu-qp22-bd8-ctu64", 22, 8, "b", "synth", dict(ctu64=True, aq_strength=0.0, tu_inter_depth=1)),
    ("tu-qp30-bd10-ctu32", 30, 10, "p", "synth", dict(ctu64=False, aq_strength=0.0, tu_inter_depth=1)),
    ("sdh-qp22-bd8-ctu64", 22, 8, "b", "synth", dict(ctu64=True, aq_strength=0.0, sdh=True)),
    ("aq-qp30-bd8-ctu64", 30, 8, "b", "synth", dict(ctu64=True, aq_strength=1.0)),
    ("aq-sdh-tu-qp22-bd10-ctu32", 22, 10, "b", "synth", dict(ctu64=False, aq_strength=1.0, sdh=True, tu_inter_depth=1)),
    ("rdoq1-qp22-bd8-ctu64", 22, 8, "b", "synth", dict(ctu64=True, aq_strength=0.0, rdoq_level=1)),
    ("rdoq2-tu-qp30-bd10-ctu32", 30, 10, "p", "synth", dict(ctu64=False, aq_strength=0.0, rdoq_level=2, tu_inter_depth=1)),
    ("weightb-qp22-bd8-ctu64", 22, 8, "b3", "fade", dict(ctu64=True, aq_strength=0.0, weightb=True, pyramid=False)),
    ("weightb-tu-rdoq1-qp30-bd8-ctu32", 30, 8, "b", "fade",
     dict(ctu64=False, aq_strength=0.0, weightb=True, tu_inter_depth=1, rdoq_level=1)),
    ("refs3-inter8-qp22-bd8-ctu64", 22, 8, "p", "synth", dict(ctu64=True, aq_strength=0.0, refs=3, inter8=True)),
    ("refs3-inter8-qp30-bd10-ctu32", 30, 10, "p", "synth", dict(ctu64=False, aq_strength=1.0, refs=3, inter8=True)),
]


def _clip(bd, kind="synth"):
    import torch

    from govideocompressor_amd.models.h264_gpu import synth_clip
    clip = synth_clip(B, F, W, H, seed=7, bit_depth=bd)
    if kind == "fade":  # a steep linear fade: luma towards black, chroma towards grey
        a = torch.tensor([1.0 - 0.15 * t for t in range(F)], device=clip[0].device).view(1, -1, 1, 1)
        z = (16 << (bd - 8), 128 << (bd - 8), 128 << (bd - 8))
        clip = tuple((zz + (p.float() - zz) * a).round().clamp(0, (1 << bd) - 1).to(p.dtype) for p, zz in zip(clip, z))
    return clip


NOISE = 4


def _static_clip(swap=False, amp=NOISE):
    """one textured picture per slot (the slots' textures differ), repeated, under independent
    uniform noise of -amp .. amp levels per picture.  The test codes it at QP 22, a quantiser step
    of 2^((22 - 4) / 6) = 8: noise of -4 .. 4 has a deviation of 2.6, and a P picture's residual
    (its own noise minus what the reference kept of its noise) one of 2.6 .. 3.7 = 0.32 .. 0.46
    steps -- where the dead zone leaves lone +-1 levels, the levels the check is there to weigh"""
    import torch

    from govideocompressor_amd.models.h264_gpu import synth_clip
    base = synth_clip(B, 1, W, H, seed=21)
    g = torch.Generator(device="cpu").manual_seed(5)
    out = []
    for p in base:
        noise = torch.randint(-amp, amp + 1, (B, F) + tuple(p.shape[2:]), generator=g).to(p.device)
        q = (p.expand(-1, F, -1, -1).to(torch.int32) + noise).clamp(0, 255).to(p.dtype)
        out.append(q.flip(0).contiguous() if swap else q.contiguous())
    return tuple(out)


def _params(bd, qp, gop, kw, **rd):
    from govideocompressor_amd.models.hevc_gpu import HevcParams
    return HevcParams(width=W, height=H, bit_depth=bd, crf=None, qp=qp, **_GOP[gop], **kw, **rd)


def _streams(params, clip, entropy, twice=False):
    from govideocompressor_amd.models.hevc_gpu import GpuHevcEncoder
    enc = GpuHevcEncoder(params, slots=B, entropy=entropy)
    res = enc.encode(*clip, keep_recon=True)
    rec = [[pl.cpu().numpy().astype(np.uint16) for pl in pic] for pic in enc.last_recon]
    again = [r.bitstream for r in enc.encode(*clip)] if twice else None
    stats = dict(enc.stats)
    enc.close()
    return res, rec, again, stats


@pytest.mark.parametrize("name,qp,bd,gop,kind,kw", CASES, ids=[c[0] for c in CASES])
def test_rd_cbf_encode(host, name, qp, bd, gop, kind, kw):
    clip = _clip(bd, kind)
    p = _params(bd, qp, gop, kw, rd_cbf=True)
    assert p.adaptive_qp() == (kw["aq_strength"] > 0)
    res, rec, again, stats = _streams(p, clip, "gpu", twice=True)
    if kw.get("weightb"):
        assert stats.get("weightb_pictures", 0) > 0, "the fade left every B picture unweighted"
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
    assert all(a != b for a, b in zip(plain, streams)), "the check left a slot's bitstream unchanged"


def test_rd_cbf_off_is_the_encoder_without_the_field():
    clip = _clip(8)
    kw = dict(ctu64=True, aq_strength=1.0, sdh=True, tu_inter_depth=1)
    plain = [r.bitstream for r in _streams(_params(8, 26, "b", kw), clip, "gpu")[0]]
    for lam in (0.25, 4.0):
        named = _streams(_params(8, 26, "b", kw, rd_cbf=False, rd_cbf_lambda=lam), clip, "gpu")[0]
        assert [r.bitstream for r in named] == plain


def test_static_clip_under_noise_gets_smaller_and_keeps_its_slots_apart():
    clip = _static_clip()
    kw = dict(ctu64=True, aq_strength=0.0)

    def enc(c, **rd):
        return [r.bitstream for r in _streams(_params(8, 22, "p", kw, **rd), c, "gpu")[0]]

    off, on = enc(clip), enc(clip, rd_cbf=True)
    print("static clip bytes per slot: off", [len(s) for s in off], "on", [len(s) for s in on])
    assert all(len(a) < len(b) for a, b in zip(on, off)), ([len(s) for s in on], [len(s) for s in off])
    lo, hi = enc(clip, rd_cbf=True, rd_cbf_lambda=0.5), enc(clip, rd_cbf=True, rd_cbf_lambda=2.0)
    print("lambda 0.5", [len(s) for s in lo], "lambda 2.0", [len(s) for s in hi])
    assert sum(map(len, hi)) <= sum(map(len, lo))
    assert lo != hi, "the lambda changes nothing"
    swapped = enc(_static_clip(swap=True), rd_cbf=True)
    assert on[0] != on[1] and swapped == on[::-1], "a slot's stream depends on its neighbour"


def test_intra_only_is_untouched():
    clip = _clip(8)
    kw = dict(ctu64=True, aq_strength=0.0)
    plain = [r.bitstream for r in _streams(_params(8, 26, "i", kw), clip, "gpu")[0]]
    assert [r.bitstream for r in _streams(_params(8, 26, "i", kw, rd_cbf=True, rd_cbf_lambda=2.0), clip, "gpu")[0]] == plain
