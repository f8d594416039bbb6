"""Decision kernels that no other golden reaches: the HEVC merge passes (hevc_b_init_p +
hevc_b_merge, hevc_merge_refine, hevc_b_choose) and H.264 spatial direct (b_spatial_exact /
b_spatial_fixup, b_spatial_decide).  A decoder round trip cannot see a changed decision, so
every case is checked two ways: the CPU decoder's reconstruction of the emitted stream equals
the encoder's, bit for bit, and the SHA-256 of every slot's bitstream equals the value that the
parent commit's kernels emitted for the same arguments, recorded on the GPU by
``tools/record_inter_layout.py decide`` into tests/golden/decide_layout_parent.json.  Whether the
HEVC decisions are the right ones is checked elsewhere: tests/test_gpu_hevc_merge_model.py holds
every output of the merge kernels against the numpy model of tests/ref_models_hevc_merge.py.
(The two ``merge_exact=False`` cases were re-recorded when that comparison found
``hevc_merge_refine`` keeping a neighbour's vector at the searched vector's merge price.)

HEVC sizes are padded to the CTB, so every wave of four 16x16 blocks is full; the shapes make
waves straddle block rows (6 and 10 blocks per row) and put blocks on CTU edges of both CTU
sizes (z-scan availability of the merge neighbours)."""
import hashlib
import json
import os

import numpy as np
import pytest

from tools.record_inter_layout import decide_stats, encode_decide_case

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decide_layout_parent.json")
with open(_GOLDEN) as _f:
    _DOC = json.load(_f)
_CASES = _DOC["cases"]


def _expect(case):
    """Counts (decide_stats) that must be > 0, so that the case cannot pass vacuously."""
    if case["codec"] == "h264":
        return ("direct",)
    return ("merge", "bi") if case["params"]["bframes"] else ("merge",)


def test_decide_layout_cases_cover_the_paths():
    """Every kernel path the suite is there for has a case at each CTU size / picture size."""
    hevc = [c for c in _CASES if c["codec"] == "hevc"]
    h264 = [c for c in _CASES if c["codec"] == "h264"]
    assert _DOC["slots"] == 2
    for ctu64 in (False, True):
        sel = [c["params"] for c in hevc if c["params"]["ctu64"] == ctu64]
        assert any(p["bframes"] == 0 and p.get("merge_exact") is True for p in sel)    # hevc_b_init_p + hevc_b_merge
        assert any(p["bframes"] == 0 and p.get("merge_exact") is False for p in sel)   # hevc_merge_refine
        assert any(p["bframes"] == 1 and p.get("tmvp") for p in sel)                   # hevc_b_choose + hevc_b_merge
    assert {(c["width"], c["height"]) for c in hevc} == {(96, 64), (160, 96), (192, 128)}
    assert any(c["params"].get("refs") == 3 and c["params"].get("ref_gate") == 0 for c in hevc)
    for size in ((80, 48), (176, 144)):
        sel = [c["params"] for c in h264 if (c["width"], c["height"]) == size]
        assert all(p["direct"] == "spatial" and p["bframes"] == 3 for p in sel)
        assert {bool(p.get("spatial_wavefront")) for p in sel} == {False, True}
    assert any(c["params"].get("pyramid") for c in h264)


@pytest.mark.parametrize("case", _CASES, ids=[c["id"] for c in _CASES])
def test_decide_layout_roundtrip_and_parent_bytes(host, case):
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
    st = decide_stats(host, case, enc, streams)
    enc.close()
    # the case exercises what it is there for
    print(case["id"], [len(s) for s in streams], st)
    for key in _expect(case):
        assert st[key] > 0, (key, st)
    # (b) the bytes of the parent commit
    assert [hashlib.sha256(s).hexdigest() for s in streams] == case["sha256"]
