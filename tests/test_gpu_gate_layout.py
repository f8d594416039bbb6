"""Gated motion searches in whole encodes: the B pictures' two list searches behind ``b_gate``
and the farther list-0 pictures' behind ``ref_gate`` run one wave per run of consecutive MBs
(me.hip), and ``me_ref_select`` a lane per MB.  A decoder round trip cannot see a changed
decision, so every case is checked two ways: the CPU decoder's reconstruction of the emitted
stream equals the encoder's, bit for bit, and the SHA-256 of every slot's bitstream equals the
value that the parent commit's kernels (a workgroup per MB) emitted for the same arguments,
recorded on the GPU by ``tools/record_inter_layout.py gate`` into
tests/golden/gate_layout_parent.json.

The golden file also holds, per case, how many MBs the gates stopped and let through under the
parent's kernels (counted from the encoder's cost buffers after each gated launch).  A case with
a non-zero gate must show both, or it would pass without a wave ever searching a survivor next
to a gated MB; the counts of the build under test must equal the parent's."""
import hashlib
import json
import os

import numpy as np
import pytest

from tools.record_inter_layout import encode_gate_case, gate_expect

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gate_layout_parent.json")
with open(_GOLDEN) as _f:
    _DOC = json.load(_f)
_CASES = _DOC["cases"]


def test_gate_layout_cases_cover_the_gates():
    assert _DOC["slots"] == 2
    for size in ((80, 48), (176, 144)):
        sel = [c for c in _CASES if (c["width"], c["height"]) == size]
        assert {c["params"]["b_gate"] for c in sel} == {2400, -150, 0}
        assert all(c["params"]["bframes"] == 3 and 5 <= c["frames"] <= 9 for c in sel)
        assert any(c["params"].get("refs") == 3 and c["params"]["ref_gate"] == 3000 for c in sel)
    assert any(c["params"].get("refs") == 3 and c["params"]["ref_gate"] == 0 for c in _CASES)
    assert any(c["params"]["weightb"] and c["params"]["aq_strength"] > 0 and c["params"]["b_gate"] < 0 for c in _CASES)
    for c in _CASES:  # the recorded (parent) counts are not vacuous
        for key in gate_expect(c):
            assert c["counts"][key] > 0, (c["id"], key)
    assert any(gate_expect(c) == ["b_gated", "b_searched", "far_gated", "far_searched"] for c in _CASES)


@pytest.mark.parametrize("case", _CASES, ids=[c["id"] for c in _CASES])
def test_gate_layout_roundtrip_and_parent_bytes(host, case):
    enc, res, counts = encode_gate_case(case)
    rec = enc.last_recon
    streams = [bytes(r.bitstream) for r in res]
    # (a) the CPU decoder reconstructs what the kernels reconstructed
    for b, r in enumerate(res):
        pics = host.decode(r.bitstream)
        assert len(pics) == r.frames == case["frames"]
        for t, pic in enumerate(pics):
            for k, name in enumerate(("y_coded", "u_coded", "v_coded")):
                assert np.array_equal(pic[name], rec[t][k][b].cpu().numpy()), f"slot {b} frame {t} plane {name}"
    enc.close()
    # the case exercises both sides of its gates, as it did under the parent's kernels
    print(case["id"], [len(s) for s in streams], counts)
    for key in gate_expect(case):
        assert counts[key] > 0, (key, counts)
    assert counts == case["counts"]
    # (b) the bytes of the parent commit
    assert [hashlib.sha256(s).hexdigest() for s in streams] == case["sha256"]
