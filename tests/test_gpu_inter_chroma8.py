"""Chroma of the H.264 inter residual as its own launch (encode_inter_chroma: eight macroblocks
per wave, eight lanes each) with the motion compensation on pairs of 16-bit samples.

Small encodes at the sizes where that layout can go wrong -- 6 MBs (one partly filled wave), 9
(one live MB in the second wave), 12 (four), 15 (seven, 5 MBs per row), 18 (two), 21 (7 MBs per
row: every wave straddles MB rows), 99 -- across P pictures with free partition splits
(per-quadrant chroma vectors), several references with weighted prediction on fades, B pictures
with implicit weights other than 32 and quadrants that mix one and two lists, the 8x8 transform
on and off, trellis 0 and 2, adaptive quantisation, a chroma QP offset and noise at a low QP.
At these sizes many vectors point outside the picture (the edge-clamped path of the chroma MC).

The clips are the synthetic content with three macroblocks planted per slot and frame: one that
no reference predicts and Intra16x16 predicts exactly (it is handed to the intra kernels), one
whose Cb / Cr get noise and one whose Cb / Cr get a small flat offset, luma untouched.

Every case is checked three ways: the CPU decoder's reconstruction of the emitted stream equals
the encoder's, bit for bit; the SHA-256 of every slot's bitstream equals what the parent commit's
kernel library (chroma on lanes 0-31 of encode_inter_mb) emitted for the same arguments, recorded
by ``tools/record_inter_layout.py chroma8`` into tests/golden/inter_chroma8_parent.json; and with
adaptive quantisation on, after every coding step ``qp_fixup`` runs on copies of the records with
the bytes the two launches left in ``qp_flags`` and without them (it then reads the levels): the
flags and the records must be equal.  Per family of cases the decoded records must show what the
family is there for (``_NEED``)."""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inter_chroma8_parent.json")
with open(_GOLDEN) as _f:
    _DOC = json.load(_f)
_CASES = _DOC["cases"]

# size -> MBs per picture (nmb % 8 = live MBs in the last wave of eight)
_SIZES = {(48, 32): 6, (48, 48): 9, (64, 48): 12, (80, 48): 15, (96, 48): 18, (112, 48): 21, (176, 144): 99}

# what the decoded records of a family's cases must show, summed over the family (chroma_stats)
_COMMON = ("mixed8", "chroma_only", "chroma_dc_only")
_NEED = {
    "p-part": _COMMON + ("split",),
    "p-refs": _COMMON + ("mref",),
    "b-weightb": _COMMON + ("bi", "uni_bi"),
}

_INTRA = (0, 1, 4, 8)


def clip(case, slots):
    """The synthetic clip of the case with, per slot and frame t >= 1, three planted MBs at
    places that move from frame to frame: rows of random values that continue the sample to
    their left (Intra16x16 horizontal predicts them, no reference does), Cb / Cr noise, and a
    flat Cb / Cr offset."""
    import torch
    from govideocompressor_amd.models.h264_gpu import synth_clip

    w, h = case["width"], case["height"]
    y, u, v = (p.cpu().numpy().copy() for p in synth_clip(slots, case["frames"], w, h, seed=case["seed"], kind=case["kind"]))
    rng = np.random.default_rng(1000 + case["seed"])
    wmb, hmb = w // 16, h // 16
    nmb = wmb * hmb
    right = [my * wmb + mx for my in range(hmb) for mx in range(1, wmb)]
    for b in range(slots):
        for t in range(1, case["frames"]):
            imb = right[(5 * t + 3 * b) % len(right)]
            others = [m for m in range(nmb) if m != imb]
            nmbi = others[(7 * t + b) % len(others)]
            dmb = [m for m in others if m != nmbi][(11 * t + 2 * b) % (len(others) - 1)]
            mx, my = imb % wmb, imb // wmb
            rows = rng.integers(16, 240, (16, 1), dtype=np.uint8)
            y[b, t, my * 16:my * 16 + 16, mx * 16 - 1:mx * 16 + 16] = rows
            mx, my = nmbi % wmb, nmbi // wmb
            for p in (u, v):
                blk = p[b, t, my * 8:my * 8 + 8, mx * 8:mx * 8 + 8].astype(np.int16)
                p[b, t, my * 8:my * 8 + 8, mx * 8:mx * 8 + 8] = np.clip(blk + rng.integers(-40, 41, blk.shape), 0, 255).astype(np.uint8)
            mx, my = dmb % wmb, dmb // wmb
            for p, off in ((u, 6), (v, -6)):
                blk = p[b, t, my * 8:my * 8 + 8, mx * 8:mx * 8 + 8].astype(np.int16)
                p[b, t, my * 8:my * 8 + 8, mx * 8:mx * 8 + 8] = np.clip(blk + off, 0, 255).astype(np.uint8)
    return [torch.from_numpy(p).cuda() for p in (y, u, v)]


def chroma_stats(host, bitstreams):
    """From the decoded records of the P / B pictures: waves of eight consecutive MBs with intra
    and inter MBs (mixed8); inter MBs with chroma levels and no luma level (chroma_only: their
    mb_qp_delta flag comes from the chroma launch alone), with chroma DC levels only
    (chroma_dc_only); MBs with a quadrant on both lists (bi), with quadrants on one and on two
    lists (uni_bi); P MBs on a farther reference (mref); split partitions; most QPs in a picture."""
    out = dict(mixed8=0, chroma_only=0, chroma_dc_only=0, bi=0, uni_bi=0, mref=0, split=0, qps=0)
    for seg in host.parse(list(bitstreams), 1):
        for hdr in np.asarray(seg["hdr"]):
            kind, cbp, qp = hdr[:, 0], hdr[:, 1], hdr[:, 2]
            intra = np.isin(kind, _INTRA)
            if intra.all():
                continue
            inter = ~intra
            ref = hdr[:, 8:16].view(np.int8).reshape(-1, 2, 4)
            two = (ref[:, 0] >= 0) & (ref[:, 1] >= 0)
            out["chroma_only"] += int((inter & ((cbp & 15) == 0) & ((cbp >> 4) > 0)).sum())
            out["chroma_dc_only"] += int((inter & ((cbp >> 4) == 1)).sum())
            out["bi"] += int((inter & two.any(axis=1)).sum())
            out["uni_bi"] += int((inter & two.any(axis=1) & ~two.all(axis=1)).sum())
            out["mref"] += int((np.isin(kind, (2, 5, 6, 7)) & (ref[:, 0, 0] > 0)).sum())
            out["split"] += int(np.isin(kind, (5, 6, 7, 10, 11, 12)).sum())
            out["qps"] = max(out["qps"], int(np.unique(qp[inter]).size))
            for w0 in range(0, kind.size, 8):
                i = intra[w0:w0 + 8]
                out["mixed8"] += int(i.any() and not i.all())
    return out


class _FixupSpy:
    """Stands in for the encoder's kernel module.  Every ``qp_fixup`` that gets the bytes of the
    two inter launches runs twice more on copies of the records, with them and without: the
    flags and the records must come out equal.  Counts the bytes (0 / 1 / 2)."""

    def __init__(self, enc):
        self._enc, self._hip = enc, enc.hip
        self.counts = {0: 0, 1: 0, 2: 0}
        self.calls = 0

    def __getattr__(self, name):
        return getattr(self._hip, name)

    def qp_fixup(self, *a, **kw):
        import torch

        if kw.get("pre"):
            enc = self._enc
            hdr = next(t for t in enc.hdr if t.data_ptr() == a[3])  # (positional as h264_gpu.py calls it)
            assert a[6] == enc.qp_flags.data_ptr() and kw["pre"] == enc.qp_pre.data_ptr()
            outs = []
            for extra in (kw, {}):
                h2, f2 = hdr.clone(), torch.full_like(enc.qp_flags, 7)
                args = list(a)
                args[3], args[6] = h2.data_ptr(), f2.data_ptr()
                self._hip.qp_fixup(*args, **extra)
                outs.append((h2, f2))
            torch.cuda.synchronize()
            assert torch.equal(outs[0][1], outs[1][1]), "qp_flags differ with the inter launches' bytes"
            assert torch.equal(outs[0][0], outs[1][0]), "records (hdr.qp) differ with the inter launches' bytes"
            pre = enc.qp_pre.cpu().numpy()
            for k in self.counts:
                self.counts[k] += int((pre == k).sum())
            self.calls += 1
        return self._hip.qp_fixup(*a, **kw)


def encode(case, slots):
    """-> (encoder, results, spy); the caller closes the encoder."""
    import torch
    from govideocompressor_amd.models.h264_gpu import GpuH264Encoder, H264Params

    enc = GpuH264Encoder(H264Params(width=case["width"], height=case["height"], **case["params"]), slots=slots)
    spy = _FixupSpy(enc)
    enc.hip = spy
    y, u, v = clip(case, slots)
    res = enc.encode(y, u, v, keep_recon=True)
    torch.cuda.synchronize()
    return enc, res, spy


def test_cases_cover_the_sizes_and_families():
    sizes = {(c["width"], c["height"]) for c in _CASES}
    assert sizes == set(_SIZES)
    assert {n % 8 for n in _SIZES.values()} == {6, 1, 4, 7, 2, 5, 3}
    assert {c["family"] for c in _CASES} == set(_NEED)
    assert _DOC["slots"] == 2 and all(5 <= c["frames"] <= 9 for c in _CASES)
    par = [c["params"] for c in _CASES]
    assert {p["t8x8"] for p in par} == {True, False} and {p["trellis"] for p in par} == {0, 2}
    assert all(p["aq_strength"] > 0 for p in par)
    assert sum(c["kind"] == "noise" and c["params"]["qp"] <= 18 for c in _CASES) >= 2


@pytest.mark.parametrize("case", _CASES, ids=[c["id"] for c in _CASES])
def test_chroma8_roundtrip_flags_and_parent_bytes(host, case):
    slots = _DOC["slots"]
    enc, res, spy = encode(case, slots)
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
    st = chroma_stats(host, streams)
    print(case["id"], [len(s) for s in streams], st, "flag bytes", spy.counts, "steps", spy.calls)
    # (b) the flags of every coding step (adaptive quantisation is on in every case)
    assert spy.calls > 0, "no step handed the inter launches' bytes to qp_fixup"
    assert spy.counts[1] > 0 and spy.counts[2] > 0, spy.counts
    assert st["qps"] > 1, st
    # the records and the flag bytes say what the parent's said when the golden file was recorded
    assert st == case["stats"]
    assert spy.counts == {int(k): n for k, n in case["flag_bytes"].items()}
    # (c) the bytes of the parent commit
    assert [hashlib.sha256(s).hexdigest() for s in streams] == case["sha256"]


@pytest.mark.parametrize("family", sorted(_NEED))
def test_family_is_not_vacuous(family):
    """From the stats recorded with the parent's bytes (the case test asserts that the streams
    under test decode to the same stats, and that the flag bytes are the same)."""
    tot = {}
    for c in _CASES:
        if c["family"] == family:
            for k, n in list(c["stats"].items()) + [("flag" + k, n) for k, n in c["flag_bytes"].items()]:
                tot[k] = tot.get(k, 0) + n
    print(family, tot)
    for key in _NEED[family] + ("flag0", "flag1", "flag2"):
        assert tot[key] > 0, (family, key, tot)
