"""Lane layout of encode_inter_mb (four macroblocks per wave, one 16-lane row each): small
shapes at which it can go wrong -- a last wave with one, two or three live MBs, waves that
straddle MB rows, waves mixing intra-flagged and inter MBs, waves where only some MBs take the
8x8 transform, four different QPs in a wave -- across B pictures, the 8x8 transform, trellis,
adaptive quantisation, partitions, several references and weighted prediction.

Every case is checked two ways: the CPU decoder's reconstruction of the emitted stream equals
the encoder's, bit for bit, and the SHA-256 of every slot's bitstream equals the value that the
parent commit's kernels (two MBs per wave) emitted for the same arguments, recorded on the GPU
by tools/record_inter_layout.py into tests/golden/inter_layout_parent.json."""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inter_layout_parent.json")
with open(_GOLDEN) as _f:
    _DOC = json.load(_f)
_CASES = _DOC["cases"]

# what the decoded records of a case must show (counts from record_stats), so that the case
# exercises what it is there for and cannot pass vacuously
_EXPECT = {
    "80x48-b-t8-trellis0-part": ("split",),
    "176x144-p-part": ("split",),
    "96x48-b-t8-trellis2-aq": ("qps",),
    "80x48-p-t8-trellis2-aq": ("qps",),
    "80x48-p-noise-lowqp": ("mixed_t8",),
    "176x144-b-noise-lowqp": ("mixed_intra", "mixed_t8"),
}


def _stats(host, bitstreams):
    """Waves = four consecutive MBs of a P / B picture: split partition MBs, waves with intra and
    inter MBs, waves with inter MBs on and off the 8x8 transform, most MB QPs in a picture."""
    out = dict(split=0, mixed_intra=0, mixed_t8=0, qps=0)
    for seg in host.parse(list(bitstreams), 1):
        for hdr in np.asarray(seg["hdr"]):
            kind, flags, qp = hdr[:, 0], hdr[:, 5], hdr[:, 2]
            intra = np.isin(kind, (0, 1, 4, 8))
            if intra.all():
                continue
            out["split"] += int(np.isin(kind, (5, 6, 7, 10, 11, 12)).sum())
            out["qps"] = max(out["qps"], int(np.unique(qp[~intra]).size))
            t8 = (flags & 2) != 0
            for w0 in range(0, kind.size, 4):
                i, t = intra[w0:w0 + 4], t8[w0:w0 + 4]
                out["mixed_intra"] += int(i.any() and not i.all())
                out["mixed_t8"] += int((t & ~i).any() and (~t & ~i).any())
    return out


def test_inter_layout_cases_cover_the_tails():
    """The recorded cases have last waves with one, two and three live MBs, and a width whose
    rows are no multiple of four MBs."""
    nmb = {(c["width"] // 16) * (c["height"] // 16) for c in _CASES}
    assert {n % 4 for n in nmb} >= {1, 2, 3}
    assert any((c["width"] // 16) % 4 for c in _CASES)
    assert set(_EXPECT) <= {c["id"] for c in _CASES}


@pytest.mark.parametrize("case", _CASES, ids=[c["id"] for c in _CASES])
def test_inter_layout_roundtrip_and_parent_bytes(host, case):
    import torch
    from govideocompressor_amd.models.h264_gpu import GpuH264Encoder, H264Params, synth_clip

    w, h, slots = case["width"], case["height"], _DOC["slots"]
    enc = GpuH264Encoder(H264Params(width=w, height=h, **case["params"]), slots=slots)
    y, u, v = synth_clip(slots, case["frames"], w, h, seed=case["seed"], kind=case["kind"])
    res = enc.encode(y, u, v, keep_recon=True)
    torch.cuda.synchronize()
    streams = [bytes(r.bitstream) for r in res]
    # (a) the CPU decoder reconstructs what the kernels reconstructed
    for b, r in enumerate(res):
        pics = host.decode(r.bitstream)
        assert len(pics) == r.frames == case["frames"]
        for t, pic in enumerate(pics):
            ry, ru, rv = (x[b].cpu().numpy() for x in enc.last_recon[t])
            assert np.array_equal(pic["y_coded"], ry), f"slot {b} frame {t}: luma mismatch"
            assert np.array_equal(pic["u_coded"], ru), f"slot {b} frame {t}: Cb mismatch"
            assert np.array_equal(pic["v_coded"], rv), f"slot {b} frame {t}: Cr mismatch"
    enc.close()
    # the case exercises what it is there for
    st = _stats(host, streams)
    print(case["id"], [len(s) for s in streams], st)
    for key in _EXPECT.get(case["id"], ()):
        assert st[key] > (3 if key == "qps" else 0), (key, st)
    # (b) the bytes of the parent commit
    assert [hashlib.sha256(s).hexdigest() for s in streams] == case["sha256"]
