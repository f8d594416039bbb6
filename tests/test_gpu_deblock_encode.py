"""Whole H.264 encodes through the deblocking pre-pass (deblock_bs) and the wavefront that skips
what its strengths switch off (csrc/kernels/deblock.hip), two slots each.

Per case:
* the SHA-256 of every slot's bitstream and of the kept reconstruction (every picture is kept, so
  B pictures are filtered too) equal what the parent's kernels gave
  (tests/golden/deblock_bs_parent.json, written by ``tools/record_inter_layout.py deblock`` with a
  kernel library built from the parent commit);
* the CPU decoder's output equals the kept reconstruction, picture for picture;
* for every P picture, the strengths the pre-pass wrote equal the parser's ``bs`` of the stream
  just written (B pictures: the parser compares reference pictures, the records (list, ref_idx)).

Sizes: 48x32 (3 x 2 MBs), 80x48 (5 MBs per row), 176x144, 48x560 (35 MB rows: the second band of
the 16 waves).
"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deblock_bs_parent.json")
SLOTS = 2
_Q = dict(crf=None, qp=26)
_B3 = dict(bframes=3, lookahead=False)
CASES = [
    dict(id="48x32-p-cabac-t8-aq", width=48, height=32, frames=5, seed=201, kind="default",
         params=dict(bframes=0, t8x8=True, aq_strength=1.0, **_Q)),
    dict(id="48x32-p-cavlc-not8", width=48, height=32, frames=5, seed=202, kind="default",
         params=dict(bframes=0, cabac=False, t8x8=False, aq_strength=0.0, **_Q)),
    dict(id="80x48-p-refs3-weightp-fade", width=80, height=48, frames=7, seed=203, kind="fade",
         params=dict(bframes=0, refs=3, weightp=True, **_Q)),
    dict(id="80x48-b3-cavlc", width=80, height=48, frames=9, seed=204, kind="default",
         params=dict(cabac=False, aq_strength=1.0, **_B3, **_Q)),
    dict(id="176x144-b3-pyramid", width=176, height=144, frames=9, seed=205, kind="default",
         params=dict(pyramid=True, refs=2, **_B3, **_Q)),
    dict(id="176x144-p-slices2-not8", width=176, height=144, frames=5, seed=206, kind="pan-fast",
         params=dict(bframes=0, slices=2, t8x8=False, **_Q)),
    dict(id="176x144-p-scenecut", width=176, height=144, frames=6, seed=207, kind="default", cut=3,
         params=dict(bframes=0, crf=None, qp=30)),
    dict(id="48x560-p-t8-aq", width=48, height=560, frames=5, seed=208, kind="default",
         params=dict(bframes=0, t8x8=True, aq_strength=1.0, crf=None, qp=22)),
    dict(id="48x560-b3", width=48, height=560, frames=5, seed=209, kind="zoom",
         params=dict(crf=None, qp=30, **_B3)),
]


class _Spy:
    """Stands in for the encoder's kernel module: keeps the strengths of every deblock launch."""

    def __init__(self, enc):
        self._enc, self._hip = enc, enc.hip
        self.bs = []

    def __getattr__(self, name):
        return getattr(self._hip, name)

    def deblock(self, *a, **kw):
        if self._enc.dbk_bs is not None:
            self.bs.append(self._enc.dbk_bs.clone())
        return self._hip.deblock(*a, **kw)


def encode(case):
    """-> (bitstreams, kept reconstruction [F][3] of [B, h, w] uint8 arrays, strengths per launch)"""
    from govideocompressor_amd.models.h264_gpu import GpuH264Encoder, H264Params, synth_clip

    p = H264Params(width=case["width"], height=case["height"], **case["params"])
    enc = GpuH264Encoder(p, slots=SLOTS)
    spy = _Spy(enc)
    enc.hip = spy
    y, u, v = synth_clip(SLOTS, case["frames"], case["width"], case["height"], seed=case["seed"], kind=case["kind"])
    if case.get("cut"):  # other content from display frame `cut` on
        y2, u2, v2 = synth_clip(SLOTS, case["frames"], case["width"], case["height"], seed=case["seed"] + 50, kind="noise")
        c = case["cut"]
        y[:, c:], u[:, c:], v[:, c:] = y2[:, c:], u2[:, c:], v2[:, c:]
    res = enc.encode(y, u, v, keep_recon=True)
    torch.cuda.synchronize()
    assert int(enc.err.item()) == 0
    recon = [[pl.cpu().numpy() for pl in pic] for pic in enc.last_recon]
    enc.close()
    return [bytes(r.bitstream) for r in res], recon, [b.cpu().numpy() for b in spy.bs]


def hashes(streams, recon):
    out = dict(sha256=[hashlib.sha256(s).hexdigest() for s in streams], recon_sha256=[])
    for b in range(len(streams)):
        h = hashlib.sha256()
        for pic in recon:
            for pl in pic:
                h.update(np.ascontiguousarray(pl[b]).tobytes())
        out["recon_sha256"].append(h.hexdigest())
    return out


def _golden():
    with open(GOLDEN) as f:
        return {c["id"]: c for c in json.load(f)["cases"]}


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_encode_through_prepass(host, case):
    want = _golden()[case["id"]]
    assert {k: want[k] for k in case} == json.loads(json.dumps(case)), "the golden file is of other cases"
    streams, recon, bs = encode(case)
    got = hashes(streams, recon)
    assert got["sha256"] == want["sha256"], "bitstreams differ from the parent's"
    assert got["recon_sha256"] == want["recon_sha256"], "reconstruction differs from the parent's"
    segs = host.parse(streams, 1)
    n_p = 0
    for b, s in enumerate(streams):
        pics = host.decode(s)
        assert len(pics) == case["frames"]
        for t, p in enumerate(pics):
            for pl, k in zip(recon[t], ("y_coded", "u_coded", "v_coded")):
                assert np.array_equal(pl[b], p[k]), "slot %d picture %d %s: decoder != reconstruction" % (b, t, k)
        seg = segs[b]
        assert seg["error"] is None and seg["n"] == len(bs), "one deblock launch per coded picture"
        for i in range(seg["n"]):  # decode order = coding steps
            if int(seg["meta"][i][4]) % 5 == 0:
                np.testing.assert_array_equal(bs[i][b], seg["bs"][i], err_msg="slot %d P picture %d (decode order)" % (b, i))
                n_p += 1
    assert n_p >= 2
