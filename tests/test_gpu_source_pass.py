"""The source pass of the H.264 encoder in one launch (``prep_aq``: padding + AQ offsets) and the
mb_qp_delta flags that ``encode_inter`` hands to ``qp_fixup``.

* planes and offsets: the fused launch against ``np.pad(mode="edge")`` (exactly) and against the
  unchanged ``prep`` + ``aq_offsets`` kernels of the same library (the ``int8`` offsets, exactly:
  the float rounding is the device's), at the shapes where its layout can go wrong -- no
  padding, 8 / 14 replicated luma rows, chroma 9 -> 16 rows, one MB column, 65 MB columns (one
  past a wave of MB columns) -- and at a width that is no multiple of 16, which must be refused
  (the caller then makes the two old calls);
* flags: after every coding step ``qp_fixup`` runs twice on copies of the records, with the
  bytes of ``encode_inter`` and without: the flags and the records must be equal; a third run
  tells the kernel that slot 0 codes an I picture and gives it wrong bytes, which it must not read;
* bytes: the same clips through ``encode``, decoded by the CPU decoder and equal to the SHA-256
  values of the parent commit's kernel library (tools/record_inter_layout.py source).
"""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "source_pass_parent.json")
with open(_GOLDEN) as _f:
    _DOC = json.load(_f)
_CASES = _DOC["cases"]

# (width, height): see the module text; all but the last take the fused launch
_SHAPES = [(48, 32), (48, 24), (48, 18), (16, 24), (1040, 24), (40, 24)]
_SLOTS, _FRAMES = 3, 4


def _random_planes(w, h, slots, frames, seed):
    """Random bytes; MB 0 of slot 0 all zero (energy 0: e = 1), the last MB of row 0 of slot 1
    all 255 (the unsigned squares), in every frame."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 256, (slots, frames, h, w), dtype=np.uint8)
    u, v = (rng.integers(0, 256, (slots, frames, h // 2, w // 2), dtype=np.uint8) for _ in range(2))
    x1 = max(0, (w // 16 - 1) * 16)
    for p, sh in ((y, 0), (u, 1), (v, 1)):
        p[0, :, :16 >> sh, :16 >> sh] = 0
        p[1 % slots, :, :16 >> sh, x1 >> sh:(x1 + 16) >> sh] = 255
    return y, u, v


def _flag_planes(w, h, slots, frames, seed):
    """Static noise (MBs without a level); per frame t >= 1 two MBs with a small change (inter
    MBs with levels) and one MB that repeats the sample to its left along its rows (Intra16x16
    predicts it, no reference does), at places that differ from frame to frame.  The last MB
    of the picture takes part: it sits in the last, partly filled wave of four MBs."""
    rng = np.random.default_rng(seed)
    wmb, hmb = w // 16, h // 16
    planes = [np.repeat(rng.integers(0, 256, (slots, 1, ph, pw), dtype=np.uint8), frames, axis=1)
              for ph, pw in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
    y = planes[0]
    right = [(mx, my) for my in range(hmb) for mx in range(1, wmb)]
    for t in range(1, frames):
        imx, imy = right[(3 * t) % len(right)]
        rmb = (wmb * hmb - 1 - 2 * t) % (wmb * hmb) if t > 1 else wmb * hmb - 1
        for b in range(slots):
            for mb in (rmb, (rmb + wmb * hmb // 2) % (wmb * hmb)):
                rmx, rmy = mb % wmb, mb // wmb
                if (rmx, rmy) == (imx, imy):
                    continue
                blk = y[b, t, rmy * 16:rmy * 16 + 16, rmx * 16:rmx * 16 + 16].astype(np.int16)
                blk += rng.integers(-48, 49, blk.shape, dtype=np.int16)
                y[b, t, rmy * 16:rmy * 16 + 16, rmx * 16:rmx * 16 + 16] = np.clip(blk, 0, 255).astype(np.uint8)
            rows, cols = slice(imy * 16, imy * 16 + 16), slice(imx * 16, imx * 16 + 16)
            y[b, t, rows, cols] = y[b, t, rows, imx * 16 - 1:imx * 16]
    return planes


def _clip(case):
    import torch

    fn = _random_planes if case["clip"] == "random" else _flag_planes
    planes = fn(case["width"], case["height"], case["slots"], case["frames"], case["seed"])
    return [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in planes]


class _FixupSpy:
    """Stands in for the encoder's kernel module.  Every ``qp_fixup`` that gets encode_inter's
    bytes runs twice more on copies of the records, with and without them: the flags and the
    records must come out equal.  A third run says through the route that slot 0 codes an I
    picture this step and holds wrong bytes for it (a stale buffer): the encoder's own plans put
    every slot's I picture at step 0, so no encode has a step with I and P slots; where slot 0
    and another slot code P / B pictures, this is such a step at the kernel's interface
    (``mixed``).  Counts the bytes (0 / 1 / 2) of the slots coding a P or B picture."""

    def __init__(self, enc):
        self._enc, self._hip = enc, enc.hip
        self.counts = {0: 0, 1: 0, 2: 0}
        self.calls = self.mixed = 0
        self.kinds = None

    def __getattr__(self, name):
        return getattr(self._hip, name)

    def qp_fixup(self, *a, **kw):
        import torch

        if kw.get("pre"):
            enc = self._enc
            hdr = next(t for t in enc.hdr if t.data_ptr() == a[3])  # (positional as h264_gpu.py calls it)
            assert a[6] == enc.qp_flags.data_ptr()
            outs = []
            for extra in (kw, {}):
                h2, f2 = hdr.clone(), torch.full_like(enc.qp_flags, 7)
                args = list(a)
                args[3], args[6] = h2.data_ptr(), f2.data_ptr()
                self._hip.qp_fixup(*args, **extra)
                outs.append((h2, f2))
            row = next(r for r in enc._route_dev if r.data_ptr() == kw["route"]).clone()
            row[0] = 2  # SlotRoute.kind of slot 0: SK_I
            stale = enc.qp_pre.clone()
            stale[0] = torch.where(stale[0] < 2, 1 - stale[0], stale[0])
            h2, f2 = hdr.clone(), torch.full_like(enc.qp_flags, 7)
            args = list(a)
            args[3], args[6] = h2.data_ptr(), f2.data_ptr()
            self._hip.qp_fixup(*args, pre=stale.data_ptr(), route=row.data_ptr())
            torch.cuda.synchronize()
            assert torch.equal(f2, outs[1][1]) and torch.equal(h2, outs[1][0]), "a stale byte of an I slot was read"
            assert torch.equal(outs[0][1], outs[1][1]), "qp_flags differ with encode_inter's bytes"
            assert int(outs[0][1].max()) <= 1
            assert torch.equal(outs[0][0], outs[1][0]), "records (hdr.qp) differ with encode_inter's bytes"
            inter = np.isin(self.kinds, (0, 1))
            pre = enc.qp_pre.cpu().numpy()[inter]
            for k in self.counts:
                self.counts[k] += int((pre == k).sum())
            self.calls += 1
            self.mixed += int(inter[0] and inter[1:].any() and bool((enc.qp_pre[0] < 2).any()))
        return self._hip.qp_fixup(*a, **kw)


def _encode(case):
    """-> (encoder, results, spy); the caller closes the encoder."""
    import torch
    from govideocompressor_amd.models.h264_gpu import GpuH264Encoder, H264Params

    enc = GpuH264Encoder(H264Params(width=case["width"], height=case["height"], **case["params"]), slots=case["slots"])
    spy = _FixupSpy(enc)
    enc.hip = spy
    step = enc._encode_step

    def spy_step(st, *a, **k):
        spy.kinds = np.asarray(st["kinds"])
        return step(st, *a, **k)

    enc._encode_step = spy_step
    y, u, v = _clip(case)
    res = enc.encode(y, u, v, keep_recon=True, anchors_at=case.get("anchors_at") or ())
    torch.cuda.synchronize()
    return enc, res, spy


def _route(slots):
    """One slot codes a reference picture (display index 1), one a non-reference picture, one is
    inactive: only the first takes a row of the MB-tree table."""
    from govideocompressor_amd.models.h264_gpu import ROUTE_DTYPE, SF_REF

    rt = np.zeros(slots, dtype=ROUTE_DTYPE)
    rt["kind"] = [0, 1, -1][:slots]
    rt["flags"] = [SF_REF, 0, 0][:slots]
    rt["disp"] = [1, 2, -1][:slots]
    return rt


@pytest.mark.parametrize("use_extra", [False, True], ids=["noextra", "extra"])
@pytest.mark.parametrize("use_fsel", [False, True], ids=["frame", "fsel"])
@pytest.mark.parametrize("shape", _SHAPES, ids=[f"{w}x{h}" for w, h in _SHAPES])
def test_fused_planes_and_offsets(shape, use_fsel, use_extra):
    import torch
    from govideocompressor_amd.ops import native

    hip = native.hip()
    w, h = shape
    B, F = _SLOTS, _FRAMES
    W, H = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    wmb, hmb = W // 16, H // 16
    nmb = wmb * hmb
    planes = _random_planes(w, h, B, F, seed=w * 100 + h)
    y, u, v = (torch.from_numpy(p).cuda() for p in planes)
    s = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()  # noqa: E731
    cs = (w // 2) * (h // 2)
    pick = [2, 0, 3] if use_fsel else [2, 2, 2]
    fsel = torch.tensor(pick, dtype=torch.int32).cuda() if use_fsel else None
    iy, iu, iv = (y, u, v) if use_fsel else (y[:, 2], u[:, 2], v[:, 2])
    extra, stride, rt = 0, 0, 0
    if use_extra:
        table = torch.from_numpy(np.random.default_rng(7).uniform(-8, 8, (B, F, nmb)).astype(np.float32)).cuda()
        rt_d = torch.from_numpy(_route(B).view(np.uint8).reshape(B, 32).copy()).cuda()
        extra, stride, rt = P(table), F * nmb, P(rt_d)

    def buffers():
        return (torch.full((B, H, W), 99, dtype=torch.uint8).cuda(), torch.full((B, H // 2, W // 2), 99, dtype=torch.uint8).cuda(),
                torch.full((B, H // 2, W // 2), 99, dtype=torch.uint8).cuda(), torch.full((B, nmb), 99, dtype=torch.int8).cuda())

    def old(oy, ou, ov, aq):
        hip.prep(P(iy), P(iu), P(iv), w, h, F * h * w, F * cs, B, P(oy), P(ou), P(ov), w, h, W, H, s, P(fsel) if use_fsel else 0)
        hip.aq_offsets(B, wmb, hmb, P(oy), P(ou), P(ov), 1.0, P(aq), s, extra, stride, rt)

    ref = buffers()
    old(*ref)
    new = buffers()
    took = hip.prep_aq(P(iy), P(iu), P(iv), w, h, F * h * w, F * cs, B, P(new[0]), P(new[1]), P(new[2]), W, H, 1.0, P(new[3]),
                       s, P(fsel) if use_fsel else 0, extra, stride, rt)
    assert took == (w % 16 == 0), "the fused launch takes widths that are a multiple of 16, and only those"
    if not took:
        assert all(int((t != 99).sum()) == 0 for t in new), "a refused launch writes nothing"
        old(*new)  # what the encoder does then
    torch.cuda.synchronize()
    for c, (plane, got) in enumerate(zip(planes, new[:3])):
        sh = 1 if c else 0
        for b in range(B):
            src = plane[b, pick[b]]
            want = np.pad(src, ((0, (H >> sh) - src.shape[0]), (0, (W >> sh) - src.shape[1])), mode="edge")
            assert np.array_equal(got[b].cpu().numpy(), want), f"plane {c} slot {b}"
    a_new, a_old = new[3].cpu().numpy(), ref[3].cpu().numpy()
    print(shape, "offsets", np.unique(a_old).tolist())
    assert np.array_equal(a_new, a_old)
    # the all-zero MB: energy 0 -> e = 1 -> round(1.0397 * -14.427) = -15 (before the MB-tree term)
    if not use_extra:
        assert a_old[0, 0] == -15 and np.unique(a_old).size > 1


def test_cases_cover_the_issue():
    ids = {c["id"] for c in _CASES}
    assert {f"planes-{w}x{h}" for w, h in _SHAPES} <= ids
    assert {"flags-48x48-trellis0", "flags-48x48-trellis2", "flags-80x48-trellis0", "flags-80x48-trellis2",
            "flags-80x48-per-slot-plans"} <= ids


@pytest.mark.parametrize("case", _CASES, ids=[c["id"] for c in _CASES])
def test_flags_roundtrip_and_parent_bytes(host, case):
    enc, res, spy = _encode(case)
    streams = [bytes(r.bitstream) for r in res]
    for b, r in enumerate(res):
        pics = host.decode(r.bitstream)
        assert len(pics) == r.frames == case["frames"]
        for t, pic in enumerate(pics):
            ry, ru, rv = (x[b].cpu().numpy() for x in enc.last_recon[t])
            assert np.array_equal(pic["y_coded"], ry), f"slot {b} frame {t}: luma mismatch"
            assert np.array_equal(pic["u_coded"], ru), f"slot {b} frame {t}: Cb mismatch"
            assert np.array_equal(pic["v_coded"], rv), f"slot {b} frame {t}: Cr mismatch"
    enc.close()
    print(case["id"], [len(s) for s in streams], spy.counts, "steps", spy.calls, "mixed", spy.mixed)
    assert spy.calls > 0, "no step handed encode_inter's bytes to qp_fixup"
    if case.get("need_flags"):
        assert all(spy.counts[k] > 0 for k in (0, 1, 2)), spy.counts
    assert spy.mixed > 0, "no step with slot 0 and another slot coding P / B pictures"
    assert [hashlib.sha256(s).hexdigest() for s in streams] == case["sha256"]
