"""The 16x16 motion search in whole encodes.  Its wave-uniform work (predictors, candidate costs,
centres, the inside tests of every phase) runs on the scalar unit, and a phase that reads only
inside the picture takes a path without clamps (csrc/kernels/me_search.h); no search decision may
change.  A decoder round trip cannot see a changed decision, so every case is checked two ways:
the CPU decoder's reconstruction of the emitted stream equals the encoder's, bit for bit, and the
SHA-256 of every slot's bitstream equals the value that the parent commit's kernels emitted for the
same arguments, recorded on the GPU by ``tools/record_inter_layout.py me`` into
tests/golden/me_uniform_parent.json."""
import hashlib
import json
import os

import numpy as np
import pytest

from tools.record_inter_layout import encode_decide_case

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "me_uniform_parent.json")
with open(_GOLDEN) as _f:
    _DOC = json.load(_f)
_CASES = _DOC["cases"]


def test_me_uniform_cases_cover_the_callers():
    """Every caller of the search has a case: P only, three B pictures with temporal direct, three
    references with weighted P, b-pyramid, CAVLC and HEVC, at 80x48, 112x112 and 176x144."""
    assert _DOC["slots"] == 2
    h264 = [c for c in _CASES if c["codec"] == "h264"]
    assert {(c["width"], c["height"]) for c in h264} == {(80, 48), (176, 144), (112, 112)}
    assert all(5 <= c["frames"] <= 9 for c in h264)
    par = [c["params"] for c in h264]
    assert any(p["bframes"] == 0 and p.get("refs") == 1 for p in par)
    assert any(p["bframes"] == 3 and p.get("direct") == "temporal" for p in par)
    assert any(p.get("refs") == 3 and p.get("weightp") for p in par)
    assert any(p.get("pyramid") for p in par)
    assert any(p.get("cabac") is False for p in par)
    assert any(c["codec"] == "hevc" and (c["width"], c["height"]) == (176, 144) for c in _CASES)
    assert len(_CASES) == 10  # the recorder drops a case the parent rejects: none was


@pytest.mark.parametrize("case", _CASES, ids=[c["id"] for c in _CASES])
def test_me_uniform_roundtrip_and_parent_bytes(host, case):
    enc, res = encode_decide_case(case)
    rec = enc.last_recon
    streams = [bytes(r.bitstream) for r in res]
    # (a) the CPU decoder reconstructs what the kernels reconstructed
    for b, r in enumerate(res):
        pics = host.decode(r.bitstream) if case["codec"] == "h264" else host.hevc_decode(r.bitstream)
        assert len(pics) == r.frames == case["frames"]
        names = ("y_coded", "u_coded", "v_coded") if case["codec"] == "h264" else ("y", "u", "v")
        for t, pic in enumerate(pics):
            for k, name in enumerate(names):
                assert np.array_equal(pic[name], rec[t][k][b].cpu().numpy()), f"slot {b} frame {t} plane {name}"
    enc.close()
    # (b) the bytes of the parent commit
    assert [hashlib.sha256(s).hexdigest() for s in streams] == case["sha256"]
