"""x265 --weightb in the GPU HEVC encoder: whole encodes (192x128, 9 pictures, CRF 27) whose
GPU reconstruction must equal what the independent CPU decoder makes of the stream -- the B
pictures' explicit uni / bi prediction (hevc_inter_cu's weightb instances), the two-list
pred_weight_table, host and GPU entropy stage, the GPU decoder on the first encoder-made
weighted-bipred streams, slot isolation, Main 10, one-list weights and the no-op on static content.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

W, H, F = 192, 128, 9


def _compare(host, res, rec, skip_filters=False):
    for b, r in enumerate(res):
        pics = host.hevc_decode(r.bitstream, skip_filters)
        assert len(pics) == r.frames
        for t, p in enumerate(pics):
            for k, name in enumerate(("y", "u", "v")):
                g = rec[t][k][b].cpu().numpy().astype(np.uint16)
                d = p[name]
                if not np.array_equal(g, d):
                    diff = np.argwhere(g != d)
                    raise AssertionError(f"slot {b} pic {t} plane {name}: {len(diff)} samples differ, first "
                                         f"{diff[0].tolist()} gpu {g[tuple(diff[0])]} cpu {d[tuple(diff[0])]}")


def _gain(clip, a, bd=8):
    """Luma black + (y - black) * a, chroma mid + (c - mid) * a; ``a``: [F] or [B, F] gains."""
    y, u, v = clip
    a = torch.as_tensor(a, dtype=torch.float32, device=y.device)
    a = a.view(1, -1, 1, 1) if a.dim() == 1 else a.view(a.shape[0], a.shape[1], 1, 1)
    blk, mid, mx = 16 << (bd - 8), 128 << (bd - 8), (1 << bd) - 1
    f = lambda p, z: (z + (p.float() - z) * a).round().clamp(0, mx).to(p.dtype)  # noqa: E731
    return f(y, blk), f(u, mid), f(v, mid)


def _fade_clip(B=2, seed=11, bd=8):
    from govideocompressor_amd.models.h264_gpu import synth_clip
    return _gain(synth_clip(B, F, W, H, seed=seed, bit_depth=bd), [1.0 - 0.1 * t for t in range(F)], bd)


def _encode(clip, keep=True, entropy="host", bd=8, **kw):
    from govideocompressor_amd.models.hevc_gpu import GpuHevcEncoder, HevcParams
    enc = GpuHevcEncoder(HevcParams(width=W, height=H, crf=27.0, bit_depth=bd, **kw), slots=clip[0].shape[0], entropy=entropy)
    res = enc.encode(*clip, keep_recon=keep)
    out = (res, enc.last_recon if keep else None, dict(enc.stats), dict(getattr(enc, "last_weightb", {})))
    enc.close()
    return out


def _check_gpu_decoder(host, streams):
    from govideocompressor_amd.models.hevc_decode_gpu import GpuHevcDecoder
    dec = GpuHevcDecoder().decode(streams)
    for i, (s, d) in enumerate(zip(streams, dec)):
        pics = host.hevc_decode_full(s, True, False)
        ref = sorted((p for p in pics if p["display"] >= 0), key=lambda p: p["display"])
        assert d.frames == len(ref)
        for t, p in enumerate(ref):
            x0, y0, w, h = p["crop_x"], p["crop_y"], p["width"], p["height"]
            for name, g in (("y", d.y), ("u", d.u), ("v", d.v)):
                sc = 0 if name == "y" else 1
                want = p[name][y0 >> sc:(y0 + h) >> sc, x0 >> sc:(x0 + w) >> sc]
                assert np.array_equal(g[t].cpu().numpy().astype(np.uint16), want), (i, t, name)


@pytest.mark.parametrize("bframes,pyramid", [(3, True), (3, False), (1, True)])
def test_gpu_hevc_weightb_fade_matches_decoders(host, bframes, pyramid):
    """Steep linear fade (gain 1.0 - 0.1 t): bit-exact with the CPU decoder, weighted B pictures
    counted, deterministic, the GPU entropy stage writes the host writer's bytes, the GPU decoder
    reproduces the CPU decoder's pictures; with three B pictures the stream is strictly smaller
    than the unweighted one (an off-centre B between anchors whose gains differ by 0.4 is otherwise
    predicted about 10 % of the luma range wrong)."""
    clip = _fade_clip()
    kw = dict(bframes=bframes, pyramid=pyramid, weightb=True)
    res, rec, stats, wmap = _encode(clip, **kw)
    assert stats.get("weightb_pictures", 0) > 0 and wmap
    _compare(host, res, rec)
    streams = [r.bitstream for r in res]
    assert [r.bitstream for r in _encode(clip, keep=False, **kw)[0]] == streams
    assert [r.bitstream for r in _encode(clip, keep=False, entropy="gpu", **kw)[0]] == streams
    _check_gpu_decoder(host, streams)
    if bframes == 3:
        off = sum(len(r.bitstream) for r in _encode(clip, keep=False, **dict(kw, weightb=False))[0])
        on = sum(len(s) for s in streams)
        print(f"weightb bytes {on} / unweighted {off} = {on / off:.4f} (bframes 3, pyramid {pyramid})")
        assert on < off, (on, off)


def _strip_clip(B, seed):
    """The fade over a clip built for the three directions: rows 0..31 change scene right after
    each anchor (noise panning by whole pixels that only the later anchor shows: list 1), rows
    96..127 change scene at each later anchor (only the earlier anchor shows it: list 0), ordinary
    content between.  Anchors at 0, 4, 8 (bframes 3, no pyramid)."""
    from govideocompressor_amd.models.h264_gpu import synth_clip
    base = synth_clip(B, F, W, H, seed=seed)
    rng = np.random.default_rng(seed)
    out = []
    for c, pa in enumerate(base):
        sh = 1 if c == 0 else 2
        ph, pw, rows = pa.shape[2], pa.shape[3], 32 // sh
        pa = pa.clone()
        for (r0, scenes) in ((0, ((0, 1), (1, 5), (5, 9))), (ph - rows, ((0, 4), (4, 8), (8, 9)))):
            for (t0, t1) in scenes:
                canvas = rng.integers(0, 256, (B, rows + 2 * F, pw + 4 * F), dtype=np.uint8)
                for t in range(t0, t1):
                    s = canvas[:, t // sh:t // sh + rows, (2 * t) // sh:(2 * t) // sh + pw]
                    pa[:, t, r0:r0 + rows] = torch.from_numpy(np.ascontiguousarray(s)).to(pa.device)
        out.append(pa.contiguous())
    return _gain(out, [1.0 - 0.1 * t for t in range(F)])


def test_gpu_hevc_weightb_covers_all_three_directions(host):
    """Coverage guard: every weighted B picture of every slot holds list-0-only, list-1-only and
    bi-predicted CUs (the decoder's CU records).  The unweighted encode of the clip shows all three
    directions in every slot too, so the guard does not depend on the tool (per encode, not per
    picture: without weights a B picture midway between the anchors' gains may bi-predict the strip
    only one anchor shows, because the average of both has the right mean)."""
    clip = _strip_clip(2, 5)
    for wb in (True, False):
        res, rec, stats, wmap = _encode(clip, bframes=3, pyramid=False, weightb=wb, scenecut=0)
        _compare(host, res, rec)
        if wb:
            assert sorted(wmap) == [1, 2, 3, 5, 6, 7] and all(any(s) for v in wmap.values() for s in v), wmap
        for b, r in enumerate(res):
            seen = {}
            for p in host.hevc_decode(r.bitstream):
                if p["slice_type"] == 0:
                    cu = p["cu"]
                    seen[p["poc"]] = set(np.unique(np.where(cu[:, 12] == 0, 1, cu[:, 12])[cu[:, 0] == 1]).tolist())
            print(f"weightb {wb} slot {b}: directions per B picture {seen}")
            assert sorted(seen) == [1, 2, 3, 5, 6, 7]
            if wb:
                assert all(d == {1, 2, 3} for d in seen.values()), (b, seen)
            else:
                assert set().union(*seen.values()) == {1, 2, 3}, (b, seen)


def test_gpu_hevc_weightb_slot_isolation(host):
    """Fade-out, the same content unfaded, fade-in: the unfaded slot is reconstructed exactly as
    without the tool and counts no weighted picture."""
    from govideocompressor_amd.models.h264_gpu import synth_clip
    one = synth_clip(1, F, W, H, seed=13)
    base = tuple(p.repeat(3, 1, 1, 1).contiguous() for p in one)
    down = [1.0 - 0.1 * t for t in range(F)]
    clip = _gain(base, [down, [1.0] * F, down[::-1]])
    on, rec_on, stats, wmap = _encode(clip, bframes=3, weightb=True)
    off, rec_off, _, _ = _encode(clip, bframes=3, weightb=False)
    _compare(host, on, rec_on)
    assert wmap and all(v[0] != (False, False) and v[2] != (False, False) for v in wmap.values()), wmap
    assert all(v[1] == (False, False) for v in wmap.values()), wmap
    assert stats["weightb_pictures"] == sum(any(s) for v in wmap.values() for s in v)
    for t in range(F):
        for k in range(3):
            assert torch.equal(rec_on[t][k][1], rec_off[t][k][1]), (t, k)


def test_gpu_hevc_weightb_main10_fade_matches_decoder(host):
    """Main 10: offsets coded in 8-bit units and scaled by 4 in the prediction."""
    clip = _fade_clip(bd=10)
    res, rec, stats, _ = _encode(clip, bd=10, bframes=3, weightb=True)
    assert stats.get("weightb_pictures", 0) > 0
    _compare(host, res, rec)


def test_gpu_hevc_weightb_one_list_only(host):
    """Only the later anchor differs in gain: list 0 stays under the thresholds, so the B pictures
    before it are weighted on list 1 alone."""
    from govideocompressor_amd.models.h264_gpu import synth_clip
    clip = _gain(synth_clip(2, F, W, H, seed=17), [1.0] * 4 + [0.6] * 5)
    res, rec, stats, wmap = _encode(clip, bframes=3, weightb=True)
    assert any(s == (False, True) for v in wmap.values() for s in v), wmap
    assert not any(s[0] for d in (1, 2, 3) for s in wmap.get(d, [])), wmap
    _compare(host, res, rec)


def test_gpu_hevc_weightb_static_content_is_untouched(host):
    """Nothing weighted: no extra launch changes anything -- the reconstruction equals the
    unweighted encode's and the streams differ only by headers (the PPS flag, and per B slice the
    empty table: two denominators and four flags, at most 2 bytes)."""
    from govideocompressor_amd.models.h264_gpu import synth_clip
    clip = synth_clip(2, F, W, H, seed=19, kind="static")
    on, rec_on, stats, wmap = _encode(clip, bframes=3, weightb=True)
    off, rec_off, _, _ = _encode(clip, bframes=3, weightb=False)
    assert stats["weightb_pictures"] == 0 and not wmap
    for t in range(F):
        for k in range(3):
            assert torch.equal(rec_on[t][k], rec_off[t][k]), (t, k)
    for a, b in zip(on, off):
        assert a.order == b.order
        pa, pb = host.hevc_decode(a.bitstream), host.hevc_decode(b.bitstream)
        for x, y in zip(pa, pb):
            assert all(np.array_equal(x[k], y[k]) for k in ("cu", "ctu", "coef_y", "coef_cb", "coef_cr"))
        kinds = {p["poc"]: p["slice_type"] for p in pa}
        for na, nb, d in zip(a.nals, b.nals, a.order):
            if kinds[d] == 0:
                assert 0 <= len(na) - len(nb) <= 2, (d, len(na), len(nb))
            else:
                assert na == nb, d
