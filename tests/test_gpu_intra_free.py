"""Intra MBs of P / B pictures (encode_intra.hip): an intra MB none of whose left / top-left /
top / top-right neighbours is intra is *free* and coded by encode_intra_free, one wave per run
of consecutive MBs; the rest are *chained* and coded by the wavefront kernel, which waits on
the row above only below an MB it codes itself (encode_intra_free also takes a chained MB whose
only intra neighbour is the left one when the same wave codes that one: the horizontal pairs
and the top rows of the groups below).  The class only changes the schedule, never a byte.

Small shapes at which that can go wrong: isolated MBs at every picture edge, one chained MB
through each single dependency (left, top, top-left, top-right; the last also with the I4x4
trial, which really predicts from the top-right samples), groups whose chains turn through
every direction, runs that straddle MB rows (5 and 11 MBs per row) with a wave coding MBs
whose raster indices do not follow each other, a free MB one column right of the wave's
previous one (the left-edge cache of the body; (k + 1, y + 1) itself would be chained through
its top-left neighbour, so the nearest row is y + 2), a last partial run, a slot without intra
MBs beside one with many, slots with free MBs only, a scene-cut P picture (everything chained
but MB 0), B pictures, two slices (an intra MB in the first row of the second slice under one
of the first: independent), and the two noisy cases of the inter-layout suite.

Every case is checked two ways: the CPU decoder's reconstruction equals the encoder's, bit for
bit, and the SHA-256 of every slot's bitstream equals what the parent commit's kernels emitted,
recorded by tools/record_inter_layout.py (suite ``intra``) into
tests/golden/intra_free_parent.json together with the free / chained counts of the decoded
pictures, which this test recomputes itself from the decoded ``mb_kind`` maps."""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "intra_free_parent.json")
with open(_GOLDEN) as _f:
    _DOC = json.load(_f)
_CASES = _DOC["cases"]

_INTRA = (0, 1, 4, 8)
_B_KINDS = (9, 10, 11, 12, 13)


def _classify(intra, slice_rows):
    """[hmb, wmb] bool intra map -> (free, chained) maps.  A row that starts a slice has no
    neighbours above (slice_rows MB rows per slice, 0: one slice)."""
    hmb, wmb = intra.shape
    top = np.arange(hmb) > 0
    if slice_rows > 0:
        top &= np.arange(hmb) % slice_rows != 0
    p = np.zeros((hmb + 1, wmb + 2), dtype=bool)
    p[1:, 1:-1] = intra
    dep = p[1:, :-2] | ((p[:-1, :-2] | p[:-1, 1:-1] | p[:-1, 2:]) & top[:, None])
    return intra & ~dep, intra & dep


def _planted_clip(case, slots):
    """Static noise; in display frame ``plant_t`` the MBs of ``spots[slot]`` (raster order) repeat
    the sample left of the MB along their rows (Intra16x16 horizontal predicts them, the
    reference does not); in column 0 they repeat the sample above along their columns."""
    import torch

    w, h, F = case["width"], case["height"], case["frames"]
    rng = np.random.default_rng(case["seed"])
    planes = []
    for ph, pw in ((h, w), (h // 2, w // 2), (h // 2, w // 2)):
        bg = rng.integers(0, 256, (slots, 1, ph, pw), dtype=np.uint8)
        planes.append(np.repeat(bg, F, axis=1))
    for b in range(slots):
        yt = planes[0][b, case["plant_t"]]
        for mx, my in sorted((tuple(s) for s in case["spots"][b]), key=lambda s: (s[1], s[0])):
            rows, cols = slice(my * 16, my * 16 + 16), slice(mx * 16, mx * 16 + 16)
            if mx > 0:
                yt[rows, cols] = yt[rows, mx * 16 - 1:mx * 16]
            else:
                yt[rows, cols] = yt[my * 16 - 1:my * 16, cols]
    return [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in planes]


def _cut_clip(case, slots):
    """The headline content, then from frame ``cut`` uniform noise panning by whole pixels: the
    old scene predicts none of the cut frame, the frames after it predict each other."""
    import torch
    from govideocompressor_amd.models.h264_gpu import synth_clip

    w, h, F, cut = case["width"], case["height"], case["frames"], case["cut"]
    rng = np.random.default_rng(case["seed"])
    out = []
    for c, pa in enumerate(synth_clip(slots, F, w, h, seed=case["seed"])):
        ph, pw, sh = pa.shape[2], pa.shape[3], 1 if c == 0 else 2
        canvas = rng.integers(0, 256, (slots, ph + 2 * F, pw + 4 * F), dtype=np.uint8)
        new = np.stack([canvas[:, t // sh:t // sh + ph, (2 * t) // sh:(2 * t) // sh + pw] for t in range(F)], axis=1)
        new = torch.from_numpy(np.ascontiguousarray(new)).to(pa.device)
        out.append(torch.cat([pa[:, :cut], new[:, cut:]], dim=1).contiguous())
    return out


def _clip(case, slots):
    from govideocompressor_amd.models.h264_gpu import synth_clip

    if case["clip"] == "spots":
        return _planted_clip(case, slots)
    if case["clip"] == "cut":
        return _cut_clip(case, slots)
    return synth_clip(slots, case["frames"], case["width"], case["height"], seed=case["seed"], kind=case["kind"])


def _counts(case, pics_by_slot, slice_rows):
    """Free / chained intra MBs of the case's P / B pictures (``pics``: display indices; None:
    every picture with an inter MB), summed over slots, and the maps of the planted picture."""
    hmb, wmb = case["height"] // 16, case["width"] // 16
    out, planted = dict(free=0, chained=0), []
    for pics in pics_by_slot:
        for t, pic in enumerate(pics):
            kinds = np.asarray(pic["mb_kind"]).reshape(hmb, wmb)
            intra = np.isin(kinds, _INTRA)
            if case["pics"] is None and intra.all():
                continue
            if case["pics"] is not None and t not in case["pics"]:
                continue
            free, chained = _classify(intra, slice_rows)
            out["free"] += int(free.sum())
            out["chained"] += int(chained.sum())
            if case["clip"] == "spots" and t == case["plant_t"]:
                planted.append((kinds, intra, free, chained))
    return out, planted


def test_intra_free_classification():
    """The test's own classifier on a map with every dependency, and across a slice edge."""
    m = np.zeros((4, 6), dtype=bool)
    for x, y in ((0, 0), (1, 0), (3, 0), (3, 1), (5, 1), (4, 2), (0, 2), (1, 3), (5, 3)):
        m[y, x] = True
    free, chained = _classify(m, 0)
    assert sorted(zip(*np.nonzero(free)[::-1])) == [(0, 0), (0, 2), (3, 0), (5, 1)]
    assert sorted(zip(*np.nonzero(chained)[::-1])) == [(1, 0), (1, 3), (3, 1), (4, 2), (5, 3)]
    free2, chained2 = _classify(m, 2)  # rows 0-1 and 2-3: (4, 2) no longer sees (5, 1) above it
    assert free2[2, 4] and not chained2[2, 4] and chained2[3, 1] and chained2[1, 3]


def test_intra_free_cases_cover_the_shapes():
    """Rows of 5 and of 11 MBs (a run of 16, 32 or 64 MBs straddles rows), pictures of 15 and
    99 MBs (a last partial run), and every case names the classes it is there for."""
    assert {c["width"] // 16 for c in _CASES} >= {5, 11}
    assert {(c["width"] // 16) * (c["height"] // 16) for c in _CASES} >= {15, 99}
    assert all(set(c["need"]) <= {"free", "chained"} for c in _CASES)
    assert {"free", "chained"} <= {k for c in _CASES for k in c["need"]}


@pytest.mark.parametrize("case", _CASES, ids=[c["id"] for c in _CASES])
def test_intra_free_roundtrip_and_parent_bytes(host, case):
    import torch
    from govideocompressor_amd.models.h264_gpu import GpuH264Encoder, H264Params

    w, h, slots = case["width"], case["height"], _DOC["slots"]
    enc = GpuH264Encoder(H264Params(width=w, height=h, **case["params"]), slots=slots)
    y, u, v = _clip(case, slots)
    res = enc.encode(y, u, v, keep_recon=True)
    torch.cuda.synchronize()
    slice_rows = int(enc.slice_rows)
    streams = [bytes(r.bitstream) for r in res]
    # (a) the CPU decoder reconstructs what the kernels reconstructed
    decoded = []
    for b, r in enumerate(res):
        pics = host.decode(r.bitstream)
        decoded.append(pics)
        assert len(pics) == r.frames == case["frames"]
        for t, pic in enumerate(pics):
            ry, ru, rv = (x[b].cpu().numpy() for x in enc.last_recon[t])
            assert np.array_equal(pic["y_coded"], ry), f"slot {b} frame {t}: luma mismatch"
            assert np.array_equal(pic["u_coded"], ru), f"slot {b} frame {t}: Cb mismatch"
            assert np.array_equal(pic["v_coded"], rv), f"slot {b} frame {t}: Cr mismatch"
    enc.close()
    # the case exercises what it is there for: the planted MBs are intra, the picture is of the
    # kind asked for, and each class the case names is present -- in the counts of the parent run
    counts, planted = _counts(case, decoded, slice_rows)
    print(case["id"], [len(s) for s in streams], counts)
    for b, (kinds, intra, free, chained) in enumerate(planted):
        assert all(intra[my, mx] for mx, my in case["spots"][b]), (b, kinds)
        if case.get("b_picture"):
            assert np.isin(kinds, _B_KINDS).any(), (b, kinds)
        if case.get("free_only"):
            assert not chained.any(), (b, kinds)
        for mx, my in case.get("free_spots", [[], []])[b]:
            assert free[my, mx], (b, mx, my, kinds)
        for mx, my in case.get("chained_spots", [[], []])[b]:
            assert chained[my, mx], (b, mx, my, kinds)
    if case["clip"] == "spots":
        assert len(planted) == slots
    if case["clip"] == "cut":
        nmb = (w // 16) * (h // 16)
        assert counts == dict(free=slots, chained=slots * (nmb - 1))
    for key in case["need"]:
        assert counts[key] > 0, (key, counts)
    assert counts == case["counts"]
    # (b) the bytes of the parent commit
    assert [hashlib.sha256(s).hexdigest() for s in streams] == case["sha256"]
