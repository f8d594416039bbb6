"""The H.264 inter kernels hand the GPU CABAC path every MB's non-zero block mask
(``encode_inter``'s ``mask_pre`` -> ``cabac_bin``'s ``pre``), so ``cabac_mask`` no longer reads every
level back to learn which blocks are zero.

Small encodes, 2 slots, 5-9 frames, at 6 MBs (a partly filled luma and chroma wave), 9 (one live
MB in the last chroma wave), 15 (waves straddle rows), 21 and 99, across P pictures with
partitions, ``refs=3`` with ``weightp`` on fades, B pictures with ``weightb``, the 8x8 transform
on / off, trellis 0 / 2, a chroma QP offset, noise at QP 16-18 (most blocks coded), flat content
at a high QP (no block coded), AQ on and off, two slices per picture, one slot at a scene cut
(every MB handed to the intra kernels) and the planted Intra16x16-only MBs of
tests/test_gpu_inter_chroma8.py (waves mix handed-over and coded MBs).

Every encode runs with ``_poison_levels``: the level buffer is filled with a non-zero pattern
before each step's kernels, so a level nobody wrote this step cannot be zero by luck.  Per case:
the stream equals the SHA-256 the parent commit's kernel library emitted
(``tools/record_inter_layout.py mask`` -> tests/golden/inter_block_mask_parent.json); it decodes to
the encoder's reconstruction on the CPU; after every coding step ``cab_mask`` equals what
``cabac_mask`` computes without ``pre`` from the levels; the records show what the case is there
for (``_NEED``).  One CAVLC and one host-entropy case show that those paths take no masks and
emit the same bytes."""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inter_block_mask_parent.json")
with open(_GOLDEN) as _f:
    _DOC = json.load(_f)
_CASES = _DOC["cases"]
SLOTS = 2

_INTRA = (0, 1, 4, 8)
_P = dict(crf=None, bframes=0)
_B = dict(crf=None, bframes=3, weightb=True, lookahead=False)
_PART = dict(partitions=True, part_overhead=0, part_min_satd=0)


def _case(id_, w, h, frames, seed, kind, clip="planted", entropy="gpu", **params):
    return dict(id=id_, width=w, height=h, frames=frames, seed=seed, kind=kind, clip=clip, entropy=entropy, params=params)


# (the recorder runs these; the test runs what the golden file holds)
CASES = [
    _case("48x32-p-part-t8-trellis2-aq", 48, 32, 6, 71, "default", qp=26, t8x8=True, trellis=2, chroma_qp_offset=-4,
          aq_strength=1.0, **_P, **_PART),
    _case("48x48-p-part-t8-trellis2", 48, 48, 6, 72, "default", qp=24, t8x8=True, trellis=2, aq_strength=0.0, **_P, **_PART),
    _case("112x48-p-part-not8-trellis0", 112, 48, 6, 73, "zoom", qp=24, t8x8=False, trellis=0, aq_strength=0.0,
          chroma_qp_offset=-4, **_P, **_PART),
    _case("80x48-p-refs3-weightp-t8-trellis0", 80, 48, 7, 75, "fade", qp=28, t8x8=True, trellis=0, refs=3, weightp=True,
          chroma_qp_offset=-6, aq_strength=0.0, **_P),
    _case("176x144-p-refs3-weightp-trellis2-aq", 176, 144, 6, 76, "fade", qp=26, t8x8=True, trellis=2, refs=3,
          weightp=True, ref_gate=0, aq_strength=1.0, **_P),
    _case("48x48-b-not8-trellis0", 48, 48, 9, 77, "default", qp=26, t8x8=False, trellis=0, chroma_qp_offset=-4,
          aq_strength=0.0, **_B),
    _case("80x48-b-t8-trellis2-aq", 80, 48, 9, 78, "pan-fast", qp=28, t8x8=True, trellis=2, chroma_qp_offset=-6,
          aq_strength=1.0, **_B),
    _case("112x48-b-t8-trellis2", 112, 48, 9, 79, "default", qp=24, t8x8=True, trellis=2, aq_strength=0.0, **_B),
    _case("176x144-b-t8-trellis0", 176, 144, 9, 80, "zoom", qp=28, t8x8=True, trellis=0, aq_strength=0.0, **_B),
    _case("80x48-p-noise-qp18", 80, 48, 6, 81, "noise", qp=18, t8x8=True, trellis=2, aq_strength=0.0, **_P),
    _case("176x144-b-noise-qp16-aq", 176, 144, 9, 82, "noise", qp=16, t8x8=True, trellis=2, aq_strength=1.0, **_B),
    _case("80x48-b-flat-qp44", 80, 48, 9, 83, "default", clip="flat", qp=44, t8x8=True, trellis=2, aq_strength=0.0, **_B),
    _case("176x128-p-slices2", 176, 128, 6, 84, "default", qp=26, t8x8=True, trellis=2, aq_strength=0.0, slices=2, **_P),
    _case("176x144-b-slices2-aq", 176, 144, 9, 85, "default", qp=26, t8x8=True, trellis=2, aq_strength=1.0, slices=2, **_B),
    _case("112x48-scenecut-slot0", 112, 48, 9, 86, "default", clip="cut", t8x8=True, trellis=2, bframes=0),
    _case("80x48-p-cavlc", 80, 48, 6, 87, "default", qp=26, t8x8=True, trellis=2, aq_strength=0.0, cabac=False, **_P),
    _case("80x48-b-host-entropy", 80, 48, 9, 88, "default", entropy="cpu", qp=26, t8x8=True, trellis=2, aq_strength=0.0, **_B),
]

# what a case's decoded records must show (record_stats), so that it cannot pass vacuously
_LUMA0 = ("chroma_only", "chroma_dc_only", "zero_mbs", "mixed_intra")
_ALL5 = ("t8_zero_chunk",) + _LUMA0
_NEED = {
    "48x32-p-part-t8-trellis2-aq": ("t8_zero_chunk", "mixed_intra"),
    "48x48-p-part-t8-trellis2": _ALL5,
    "112x48-p-part-not8-trellis0": _LUMA0,
    "80x48-p-refs3-weightp-t8-trellis0": _ALL5,
    "176x144-p-refs3-weightp-trellis2-aq": _ALL5,
    "48x48-b-not8-trellis0": _LUMA0,
    "80x48-b-t8-trellis2-aq": ("t8_zero_chunk", "chroma_only", "zero_mbs", "mixed_intra"),
    "112x48-b-t8-trellis2": _ALL5,
    "176x144-b-t8-trellis0": _ALL5,
    "80x48-p-noise-qp18": ("full_mbs", "mixed_intra"),
    "176x144-b-noise-qp16-aq": ("full_mbs", "mixed_intra"),
    "80x48-b-flat-qp44": ("zero_mbs",),
    "176x128-p-slices2": _ALL5,
    "176x144-b-slices2-aq": _ALL5,
    "112x48-scenecut-slot0": ("all_intra_pics", "mixed_intra"),
}
# ... and what the cases together must show
_NEED_ALL = ("t8_zero_chunk", "chroma_only", "chroma_dc_only", "zero_mbs", "mixed_intra", "full_mbs", "all_intra_pics")


def clip(case):
    """planted: the clip of tests/test_gpu_inter_chroma8.py (per slot and frame one MB that only
    Intra16x16 predicts, one with Cb / Cr noise, one with a flat Cb / Cr offset); flat: one grey
    level per frame; cut: slot 0 switches to panning noise at frame 5, slot 1 goes on."""
    import torch
    from govideocompressor_amd.models.h264_gpu import synth_clip

    w, h, F = case["width"], case["height"], case["frames"]
    if case["clip"] == "planted":
        try:
            import test_gpu_inter_chroma8 as C8
        except ImportError:  # (run from the recorder: tests/ is not on the path)
            from tests import test_gpu_inter_chroma8 as C8

        return C8.clip(case, SLOTS)
    if case["clip"] == "flat":
        lv = torch.arange(F, dtype=torch.uint8, device="cuda").view(1, F, 1, 1)
        return [(base + lv).expand(SLOTS, F, h // s, w // s).contiguous() for base, s in ((100, 1), (128, 2), (128, 2))]
    assert case["clip"] == "cut"
    rng = np.random.default_rng(case["seed"])
    out = []
    for c, pa in enumerate(synth_clip(SLOTS, F, w, h, seed=case["seed"], kind=case["kind"])):
        ph, pw, sh = pa.shape[2], pa.shape[3], 1 if c == 0 else 2
        canvas = rng.integers(0, 256, (ph + 2 * F, pw + 4 * F), dtype=np.uint8)
        new = np.stack([canvas[t // sh:t // sh + ph, (2 * t) // sh:(2 * t) // sh + pw] for t in range(F)])
        pa = pa.clone()
        pa[0, 5:] = torch.from_numpy(np.ascontiguousarray(new[5:])).to(pa.device)
        out.append(pa)
    return out


class _Spy:
    """Stands in for the encoder's kernel module.  Notes what every ``encode_inter`` is asked
    for; before every ``cabac_bin`` that gets the inter kernels' masks, runs it once more without
    them into scratch buffers (it then reads the levels) and compares the two mask buffers."""

    def __init__(self, enc):
        self._enc, self._hip = enc, enc.hip
        self.mask_pre, self.bins, self.pre_words = set(), 0, 0

    def __getattr__(self, name):
        return getattr(self._hip, name)

    def encode_inter(self, *a, **kw):
        self.mask_pre.add(bool(kw.get("mask_pre")))
        return self._hip.encode_inter(*a, **kw)

    def cabac_bin(self, *a, **kw):
        import torch

        enc = self._enc
        if not kw.get("pre"):
            return self._hip.cabac_bin(*a, **kw)
        # positional as h264_gpu.py calls it: 5 mask, 6 nb, 7 cnt, 8 off, 9 tot, 10 pool, 12 pool_used, 13 base, 14 total
        assert a[5] == enc.cab_mask.data_ptr()
        pool = next(p for p in enc.cab_pool if p.data_ptr() == a[10])
        scratch = [torch.zeros_like(enc.cab_mask), torch.zeros_like(enc.cab_nb), torch.zeros_like(enc.cab_cnt),
                   torch.zeros_like(enc.cab_off), torch.zeros_like(enc.cab_tot), torch.empty_like(pool),
                   torch.zeros(1, dtype=torch.int64, device=pool.device),
                   torch.zeros(enc.B * enc.S, dtype=torch.int64, device=pool.device),
                   torch.zeros(enc.B * enc.S, dtype=torch.int32, device=pool.device)]
        args = list(a)
        for i, t in zip((5, 6, 7, 8, 9, 10, 12, 13, 14), scratch):
            args[i] = t.data_ptr()
        self._hip.cabac_bin(*args, **{k: v for k, v in kw.items() if k != "pre"})
        out = self._hip.cabac_bin(*a, **kw)
        torch.cuda.synchronize()
        assert torch.equal(scratch[0], enc.cab_mask), "cab_mask from the inter kernels' words != from the levels"
        self.bins += 1
        pre = next(m for m in enc.mask_pre if m.data_ptr() == kw["pre"])
        self.pre_words += int((pre >= 0).sum())  # (int32 view: the handed-over marker is negative)
        return out


def encode(case, poison=True):
    """-> (encoder, results, spy); the caller closes the encoder."""
    import torch
    from govideocompressor_amd.models.h264_gpu import GpuH264Encoder, H264Params

    enc = GpuH264Encoder(H264Params(width=case["width"], height=case["height"], **case["params"]), slots=SLOTS,
                         entropy=case["entropy"])
    enc._poison_levels = poison
    spy = _Spy(enc)
    enc.hip = spy
    y, u, v = clip(case)
    res = enc.encode(y, u, v, keep_recon=True)
    torch.cuda.synchronize()
    return enc, res, spy


def record_stats(host, bitstreams):
    """From the decoded records and levels of the P / B pictures (masks by cabac_block_mask):
    inter MBs on the 8x8 transform with a coded 8x8 block that has an all-zero chunk, with chroma
    levels and no luma level, with chroma DC levels only, with no level, with every luma block
    coded; waves of four consecutive MBs with intra and inter MBs; pictures after the first whose
    MBs are all intra."""
    from govideocompressor_amd.utils.h264_synth import unpack_levels

    out = dict(t8_zero_chunk=0, chroma_only=0, chroma_dc_only=0, zero_mbs=0, full_mbs=0, mixed_intra=0, all_intra_pics=0)
    for seg in host.parse(list(bitstreams), 1):
        for t, hdr in enumerate(np.asarray(seg["hdr"])):
            kind, flags = hdr[:, 0], hdr[:, 5]
            intra = np.isin(kind, _INTRA)
            if intra.all():
                out["all_intra_pics"] += int(t > 0)
                continue
            inter = ~intra
            m = np.asarray(host.cabac_block_masks(np.ascontiguousarray(hdr), np.ascontiguousarray(unpack_levels(seg, t))))
            luma, chroma = m & 0xFFFF, m >> 17
            nib = np.stack([(luma >> (4 * b)) & 15 for b in range(4)], axis=1)
            out["t8_zero_chunk"] += int((inter & ((flags & 2) != 0) & ((nib != 0) & (nib != 15)).any(axis=1)).sum())
            out["chroma_only"] += int((inter & (luma == 0) & (chroma != 0)).sum())
            out["chroma_dc_only"] += int((inter & (luma == 0) & (chroma != 0) & ((chroma >> 2) == 0)).sum())
            out["zero_mbs"] += int((inter & (m == 0)).sum())
            out["full_mbs"] += int((inter & (luma == 0xFFFF)).sum())
            for w0 in range(0, kind.size, 4):
                i = intra[w0:w0 + 4]
                out["mixed_intra"] += int(i.any() and not i.all())
    return out


def test_cases_cover_the_sizes_and_families():
    assert {c["id"] for c in _CASES} == {c["id"] for c in CASES}
    nmb = {(c["width"] // 16) * (c["height"] // 16) for c in _CASES}
    assert nmb >= {6, 9, 15, 21, 99}
    assert all(5 <= c["frames"] <= 9 for c in _CASES) and _DOC["slots"] == SLOTS
    par = [c["params"] for c in _CASES if c["entropy"] == "gpu" and c["params"].get("cabac", True)]
    assert {p["t8x8"] for p in par} == {True, False} and {p["trellis"] for p in par} == {0, 2}
    assert {p.get("aq_strength", 1.0) > 0 for p in par} == {True, False}
    assert any(p.get("slices") == 2 for p in par) and any(p.get("chroma_qp_offset") for p in par)
    assert any(p.get("refs") == 3 and p.get("weightp") for p in par) and any(p.get("weightb") for p in par)
    assert any(p.get("partitions") for p in par)
    assert sum(c["kind"] == "noise" and 16 <= c["params"]["qp"] <= 18 for c in _CASES) >= 2
    assert {c["clip"] for c in _CASES} == {"planted", "flat", "cut"}
    tot = {k: sum(c["stats"][k] for c in _CASES) for k in _NEED_ALL}
    print(tot)
    assert all(tot[k] > 0 for k in _NEED_ALL), tot
    for c in _CASES:
        for k in _NEED.get(c["id"], ()):
            assert c["stats"][k] > 0, (c["id"], k, c["stats"])
        if c["clip"] == "flat":
            assert c["stats"]["full_mbs"] == c["stats"]["chroma_only"] == 0


@pytest.mark.parametrize("case", _CASES, ids=[c["id"] for c in _CASES])
def test_block_mask_bytes_masks_and_roundtrip(host, case):
    cabac_gpu = case["entropy"] == "gpu" and case["params"].get("cabac", True)
    enc, res, spy = encode(case)  # (the spy checks every step's cab_mask against the levels')
    streams = [bytes(r.bitstream) for r in res]
    if cabac_gpu:
        assert spy.mask_pre == {True}, spy.mask_pre
        # (a batch whose symbol pool runs out is coded again with a larger one: the noise cases)
        assert spy.bins >= case["frames"] and spy.bins % case["frames"] == 0
        assert spy.pre_words > 0, "no MB's mask came from the inter kernels"
    else:
        # the CAVLC kernels and the host writers count every block's levels themselves
        assert enc.mask_pre is None and spy.mask_pre == {False} and spy.bins == 0, (spy.mask_pre, spy.bins)
    for b, r in enumerate(res):
        pics = host.decode(r.bitstream)
        assert len(pics) == r.frames == case["frames"]
        for t, pic in enumerate(pics):
            ry, ru, rv = (x[b].cpu().numpy() for x in enc.last_recon[t])
            assert np.array_equal(pic["y_coded"], ry), f"slot {b} frame {t}: luma mismatch"
            assert np.array_equal(pic["u_coded"], ru), f"slot {b} frame {t}: Cb mismatch"
            assert np.array_equal(pic["v_coded"], rv), f"slot {b} frame {t}: Cr mismatch"
    enc.close()
    st = record_stats(host, streams)
    print(case["id"], [len(s) for s in streams], st)
    assert st == case["stats"]
    assert [hashlib.sha256(s).hexdigest() for s in streams] == case["sha256"]
