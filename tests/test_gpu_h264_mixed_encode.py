"""Whole encodes with ``H264Params.mixed_refs`` (x264 --mixed-refs) at a fixed QP.

The planted clip (96x64): pictures 0 and 1 are two unrelated smooth textures A and B (no scene
cut detection), pictures 2, 3 and 4 are chequers of A and B -- 8x8 cells, then cells 16 wide and
8 tall, then 8 wide and 16 tall -- every cell of a picture moved by the same two samples (each
picture in a direction of its own, so an earlier chequer is no clean reference for a later one),
plus mild noise.  Four reference pictures, so A and B stay in the list up to the last chequer.
A macroblock of a chequer is half in one reference picture and half in another: with one
reference per MB it pays for a bad prediction or goes intra, with one per 8x8 quadrant it is
P_8x8 / P_16x8 / P_8x16 with alternating references at one vector.  ``test_model_picks_mixed``
shows on the CPU, with the model alone, that the decision rule takes the quadrant-wise candidate
on such a picture; the GPU tests then hold the encoder to what follows from it.
"""
import numpy as np
import pytest

import ref_models_h264_mixed as mx

W, H, QP = 96, 64, 30
WMB, HMB = W // 16, H // 16
SHIFT = 2  # samples
SHIFTS = {2: (SHIFT, SHIFT), 3: (-SHIFT, SHIFT), 4: (SHIFT, -SHIFT)}  # (dx, dy) of pictures 2, 3, 4
HDR = np.dtype([("kind", "u1"), ("cbp", "u1"), ("qp", "i1"), ("i16", "u1"), ("chroma", "u1"), ("flags", "u1"),
                ("sub_direct", "u1"), ("pad", "u1"), ("ref", "i1", (2, 4)), ("mv", "<i2", (2, 4, 2)),
                ("i4", "u1", (16,))])
P16x16, P16x8, P8x16, P8x8, BDIRECT = 2, 5, 6, 7, 13
BASE = dict(crf=None, qp=QP, bframes=0, scenecut=0, refs=4, weightp=False)


def _texture(rng, h, w, scale):
    """smooth, strong contrast: box-filtered noise stretched to the full range"""
    t = rng.normal(0, 1, size=(h + 16, w + 16))
    k = np.ones(scale) / scale
    for ax in (0, 1):
        t = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), ax, t)
    t = t[8:8 + h, 8:8 + w]
    return (t - t.min()) / (t.max() - t.min()) * 200 + 28


def _chequer(rng, a, b, cw, ch, s, noise):
    """cells cw x ch alternating a / b, each texture moved by s = (dx, dy) samples (windows of the padded textures)"""
    h, w = a.shape[0] - 16, a.shape[1] - 16
    wa, wb = (t[8 + s[1]:8 + s[1] + h, 8 + s[0]:8 + s[0] + w] for t in (a, b))
    yy, xx = np.mgrid[0:h, 0:w]
    pick = ((yy // ch + xx // cw) % 2) == 0
    return np.clip(np.where(pick, wa, wb) + rng.normal(0, noise, size=(h, w)), 0, 255)


_CLIP = {}


def _clip(fade=False):
    """[1, 6, H, W] luma and [1, 6, H/2, W/2] chroma planes (numpy uint8)"""
    if fade in _CLIP:
        return _CLIP[fade]
    rng = np.random.default_rng(41)
    planes = []
    for (h, w, sc) in ((H, W, 7), (H // 2, W // 2, 5), (H // 2, W // 2, 5)):
        a, b = _texture(rng, h + 16, w + 16, sc), _texture(rng, h + 16, w + 16, sc)
        d = 16 // (H // h)  # cell unit: 16 luma samples
        sh = {t: (v[0] * h // H, v[1] * h // H) for t, v in SHIFTS.items()}
        pics = [a[8:8 + h, 8:8 + w], b[8:8 + h, 8:8 + w], _chequer(rng, a, b, d // 2, d // 2, sh[2], 1.0),
                _chequer(rng, a, b, d, d // 2, sh[3], 1.0), _chequer(rng, a, b, d // 2, d, sh[4], 1.0)]
        if fade:  # pictures 2.. fade towards grey: RefPicList0[0] gets explicit weights
            for t in range(2, 5):
                pics[t] = (pics[t] - 128) * (1 - 0.12 * (t - 1)) + 128 + 4 * (t - 1)
        # picture 5: the 8x8 chequer without a shift (its own noise stream), for the B-picture test
        pics.append(_chequer(np.random.default_rng(43 + len(planes)), a, b, d // 2, d // 2, (0, 0), 1.0))
        planes.append(np.clip(np.stack(pics), 0, 255).astype(np.uint8)[None])
    _CLIP[fade] = planes
    return planes


_RUNS = {}


def _encode(slots=1, entropy="gpu", fade=False, reps=None, frames=5, **kw):
    """One encode of the planted clip in every slot (``reps``: per-slot picture orders, to tell
    slots apart) -> dict(streams, recon, records, stats); cached per configuration."""
    import torch
    from govideocompressor_amd.models.h264_gpu import GpuH264Encoder, H264Params
    key = (slots, entropy, fade, reps, frames, tuple(sorted(kw.items())))
    if key in _RUNS:
        return _RUNS[key]
    planes = _clip(fade)
    order = reps if reps is not None else [tuple(range(frames))] * slots
    y, u, v = (torch.from_numpy(np.ascontiguousarray(np.stack([p[0][list(o)] for o in order]))).cuda() for p in planes)
    enc = GpuH264Encoder(H264Params(width=W, height=H, **{**BASE, **kw}), slots=slots, entropy=entropy)
    enc.keep_records = True
    res = enc.encode(y, u, v, keep_recon=True, idr_ids=[3] * slots)  # (idr_pic_id would tell the slots apart)
    torch.cuda.synchronize()
    out = dict(streams=[r.bitstream for r in res], psnr=[r.psnr_y for r in res], stats=dict(enc.stats),
               recon=[[x.cpu().numpy() for x in t] for t in enc.last_recon],
               records=[r[0].cpu().numpy().view(HDR).reshape(slots, WMB * HMB) for r in enc.last_records])
    enc.close()
    _RUNS[key] = out
    return out


def _check_roundtrip(host, run):
    for b, s in enumerate(run["streams"]):
        pics = host.decode(s)
        assert len(pics) == len(run["recon"])
        for t, pic in enumerate(pics):
            ry, ru, rv = (p[b] for p in run["recon"][t])
            assert np.array_equal(pic["y_coded"], ry), f"slot {b} picture {t}: luma differs"
            assert np.array_equal(pic["u_coded"], ru), f"slot {b} picture {t}: Cb differs"
            assert np.array_equal(pic["v_coded"], rv), f"slot {b} picture {t}: Cr differs"


def _check_gpu_decoder(host, streams):
    from govideocompressor_amd.models.h264_decode_gpu import GpuH264Decoder
    for s, d in zip(streams, GpuH264Decoder().decode(streams)):
        ref = host.decode(s)
        assert d.frames == len(ref) and d.path == "gpu"
        y, u, v = d.y.cpu().numpy(), d.u.cpu().numpy(), d.v.cpu().numpy()
        for t, p in enumerate(ref):
            h, w = y[t].shape
            for name, a, b in (("y", y[t], p["y_coded"][:h, :w]), ("u", u[t], p["u_coded"][:h // 2, :w // 2]),
                               ("v", v[t], p["v_coded"][:h // 2, :w // 2])):
                assert np.array_equal(a, b), f"GPU decoder, picture {t} plane {name}"


# ---------------------------------------------------------------- the rule on the planted pictures (CPU)
def _planted_model(host, t, refs):
    """Picture t against the source pictures ``refs`` as its list 0, integer search results planted
    from the known shifts (a vector is the picture's shift less its reference's) -> model outputs,
    the planted list-0[0] costs"""
    luma = _clip()[0][0]
    nmb, K = WMB * HMB, len(refs) - 1
    lam = np.asarray(host.table("lambda")[0])
    L = int(lam[QP])
    vec = [(4 * (SHIFTS[t][0] - SHIFTS.get(r, (0, 0))[0]), 4 * (SHIFTS[t][1] - SHIFTS.get(r, (0, 0))[1])) for r in refs]
    pool = np.stack([luma[r] for r in refs])[None]
    pics = [mx.Pic(pool[0, k]) for k in range(len(refs))]
    mv = np.tile(np.array(vec[0], np.int16), (1, nmb, 1))
    xmv = np.stack([np.tile(np.array(v, np.int16), (1, nmb, 1)) for v in vec[1:]])
    cost = np.zeros((1, nmb), np.int32)
    xcost = np.zeros((K, 1, nmb), np.int32)
    for m in range(nmb):
        X, Y = (m % WMB) * 16, (m // WMB) * 16
        s = luma[t][Y:Y + 16, X:X + 16]
        for k in range(K + 1):
            c = sum(mx.satd8(s[y:y + 8, x:x + 8], pics[k].block(X + x, Y + y, *vec[k])) for y in (0, 8) for x in (0, 8)) + 2 * L
            if k == 0:
                cost[0, m] = c
            else:
                xcost[k - 1, 0, m] = c
    assert cost.min() > 3000  # every MB passes the default ref_gate
    scale = np.array([[256 * (t - r) // (t - refs[0])] for r in refs[1:]], np.int16)
    e = mx.p_mixed_refs(lam, WMB, HMB, 4, [0], [K + 1], [list(range(K + 1)) + [-1] * (3 - K)], np.array([QP]), None, mv,
                        np.repeat(mv[:, :, None], 4, 2), cost, np.zeros((1, nmb, 256), np.uint8), xmv, xcost,
                        np.zeros((K, 1, nmb, 256), np.uint8), np.zeros((1, nmb), np.int8), np.zeros((1, nmb, 4), np.int8),
                        luma[t][None], luma[t][None], pool, mv, scale, 8, 2000)
    return e, cost, vec


_INTERIOR = np.array([0 < m % WMB < WMB - 1 and 0 < m // WMB < HMB - 1 for m in range(WMB * HMB)])


def test_model_picks_mixed(host):
    """Picture 2 (8x8 chequer) against pictures 1 and 0: every MB's two 16x16 candidates cost thousands
    (half of the MB is the other texture), the quadrant-wise one a few hundred -- (c) wins in every
    MB, with references alternating and one vector.  The GPU assertions below rest on this and on
    the next test."""
    e, cost, vec = _planted_model(host, 2, [1, 0])
    assert (e["winner"][0] == 3).all()
    r4 = e["mref4"][0]
    assert ((r4[:, 0] == r4[:, 3]) & (r4[:, 1] == r4[:, 2]) & (r4[:, 0] != r4[:, 1])).all()
    assert (e["mv8"][0][_INTERIOR] == vec[1]).all()
    assert (e["cost"][0] < cost[0] // 2).all() and (e["cost"][0][_INTERIOR] < 1000).all()


@pytest.mark.parametrize("t", [3, 4])
def test_model_pairs_quadrants_on_the_later_chequers(host, t):
    """Picture 3 (cells 16 wide, 8 tall) against [picture 2, B, A] and picture 4 (8 wide, 16 tall)
    against [picture 3, picture 2, B, A]: the earlier chequers carry another shift and other cells,
    so each half of an MB goes to the clean texture it was cut from -- reference 1 and 2 in
    picture 3, 2 and 3 in picture 4 -- the two quadrants of a half on one reference with one
    vector (P_16x8 in picture 3, P_8x16 in picture 4)."""
    refs = [2, 1, 0] if t == 3 else [3, 2, 1, 0]
    e, cost, vec = _planted_model(host, t, refs)
    w, r4, m8 = e["winner"][0][_INTERIOR], e["mref4"][0][_INTERIOR], e["mv8"][0][_INTERIOR]
    assert (w == 3).all()
    pa, pb = ((0, 1), (2, 3)) if t == 3 else ((0, 2), (1, 3))  # the quadrants of the two halves
    clean = {len(refs) - 2, len(refs) - 1}                      # B and A in this list
    for m in range(len(r4)):
        assert r4[m][pa[0]] == r4[m][pa[1]] and r4[m][pb[0]] == r4[m][pb[1]], (m, r4[m])
        assert {int(r4[m][pa[0]]), int(r4[m][pb[0]])} == clean, (m, r4[m])
        assert (m8[m] == vec[-1]).all(), (m, m8[m])  # one vector: the picture's own shift


# ---------------------------------------------------------------- the planted clip on the GPU
@pytest.mark.gpu
def test_planted_clip_roundtrip_and_records(host):
    run = _encode(mixed_refs=True)
    _check_roundtrip(host, run)
    _check_gpu_decoder(host, run["streams"])
    assert run["stats"]["mixed_ref_mbs"] > 0
    seen, quiet_edge = set(), 0
    seg = host.parse([run["streams"][0]], 1)[0]
    assert seg["error"] is None
    refs_used = set()
    for t in range(2, 5):
        rec, mask = run["records"][t][0], seg["mask"][t]
        for m in range(WMB * HMB):
            r, k = rec["ref"][m, 0], int(rec["kind"][m])
            if k not in (P16x16, P16x8, P8x16, P8x8) or (r == r[0]).all():
                continue
            seen.add(k)
            refs_used.update(int(x) for x in r)
            mvq = rec["mv"][m, 0]
            for qa, qb in ((0, 1), (2, 3), (0, 2), (1, 3)):  # the MB's internal 8x8 edges
                bits = (0xF << (4 * qa)) | (0xF << (4 * qb))
                quiet_edge += int(r[qa] != r[qb] and (mvq[qa] == mvq[qb]).all() and not (int(mask[m]) & bits))
    assert seen == {P8x8, P16x8, P8x16}, seen
    assert {1, 2} <= refs_used, refs_used
    # equal vectors, different references, no levels on either side: bS = 1, which the strength
    # pre-pass must not call quiet (the round trip above has filtered across it)
    assert quiet_edge > 0
    # the parsed records carry the same references
    for t in range(2, 5):
        got = seg["hdr"][t].view(HDR).reshape(-1)
        inter = np.isin(run["records"][t][0]["kind"], [P16x16, P16x8, P8x16, P8x8])
        assert np.array_equal(got["ref"][inter, 0], run["records"][t][0]["ref"][inter, 0])


@pytest.mark.gpu
def test_planted_clip_gpu_cabac_equals_host_writer(host):
    assert _encode(mixed_refs=True)["streams"] == _encode(mixed_refs=True, entropy="cpu")["streams"]


@pytest.mark.gpu
def test_planted_clip_is_smaller_with_the_knob(host):
    on, off = _encode(mixed_refs=True), _encode(mixed_refs=False)
    assert "mixed_ref_mbs" not in off["stats"]
    print("planted clip bytes on / off:", len(on["streams"][0]), len(off["streams"][0]), "PSNR-Y on / off:",
          on["psnr"][0], off["psnr"][0])
    assert len(on["streams"][0]) < len(off["streams"][0])


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(refs=1), dict(partitions=False)], ids=["refs1", "no-partitions"])
def test_knob_without_effect_gives_the_same_bytes(host, kw):
    on, off = _encode(mixed_refs=True, **kw), _encode(mixed_refs=False, **kw)
    assert on["streams"] == off["streams"] and "mixed_ref_mbs" not in on["stats"]


@pytest.mark.gpu
def test_intra_only_clip_gives_the_same_bytes(host):
    on, off = _encode(mixed_refs=True, frames=1), _encode(mixed_refs=False, frames=1)
    assert on["streams"] == off["streams"]


@pytest.mark.gpu
def test_two_encodes_give_the_same_bytes(host):
    a = _encode(mixed_refs=True)
    _RUNS.clear()
    assert _encode(mixed_refs=True)["streams"] == a["streams"]


@pytest.mark.gpu
def test_slot_does_not_depend_on_its_neighbours(host):
    """a batch of three slots with different pictures (the chequers in another order) against the
    middle slot alone"""
    orders = ((0, 1, 2, 3, 4), (0, 1, 3, 4, 2), (1, 0, 4, 2, 3))
    batch = _encode(slots=3, reps=orders, mixed_refs=True)
    alone = _encode(slots=1, reps=orders[1:2], mixed_refs=True)
    assert batch["streams"][1] == alone["streams"][0]
    assert len({len(s) for s in batch["streams"]}) == 3 and batch["stats"]["mixed_ref_mbs"] > 0
    _check_roundtrip(host, batch)


@pytest.mark.gpu
def test_b_pictures_direct_from_mixed_colocated(host):
    """bframes=3: I (texture B) b b b P (texture A) b b b P (the unshifted 8x8 chequer).  The last
    anchor takes A from the anchor before it and B from the I picture, quadrant by quadrant at the
    zero vector; the three pictures coded after it as B pictures show the same chequer, so temporal
    direct -- which follows each co-located quadrant to that quadrant's own reference -- predicts
    them exactly.  B macroblocks coded as direct over a co-located MB with unequal references
    must exist, and everything decodes bit-exactly."""
    import torch
    from govideocompressor_amd.models.h264_gpu import GpuH264Encoder, H264Params
    planes = _clip()
    order = [1, 0, 1, 0, 0, 5, 5, 5, 5]
    y, u, v = (torch.from_numpy(np.ascontiguousarray(p[:, order])).cuda() for p in planes)
    enc = GpuH264Encoder(H264Params(width=W, height=H, **{**BASE, "bframes": 3, "b_adapt": 0, "direct": "temporal",
                                                           "mixed_refs": True}), slots=1)
    enc.keep_records = True
    res = enc.encode(y, u, v, keep_recon=True)
    torch.cuda.synchronize()
    run = dict(streams=[r.bitstream for r in res], recon=[[x.cpu().numpy() for x in t] for t in enc.last_recon])
    plan = enc.last_plans[0]
    records = [r[0].cpu().numpy().view(HDR).reshape(WMB * HMB) for r in enc.last_records]  # coding order
    stats = dict(enc.stats)
    enc.close()
    assert [p.kind for p in plan].count("B") == 6 and plan[5].kind == "P" and plan[5].d == 8
    _check_roundtrip(host, run)
    _check_gpu_decoder(host, run["streams"])
    assert stats["mixed_ref_mbs"] > 0
    col = records[5]  # the last anchor: RefPicList1[0] of the B pictures coded after it
    mixed = np.isin(col["kind"], [P16x8, P8x16, P8x8]) & (col["ref"][:, 0] != col["ref"][:, 0, :1]).any(axis=1)
    assert mixed.sum() > 0
    direct = sum(int(((records[t]["kind"] == BDIRECT) & mixed).sum()) for t in (6, 7, 8) if plan[t].kind == "B")
    assert direct > 0, (int(mixed.sum()), [np.bincount(records[t]["kind"], minlength=14).tolist() for t in (6, 7, 8)])


@pytest.mark.gpu
def test_weighted_reference_zero_beside_unweighted_farther(host):
    """weightp on a fade: quadrants on RefPicList0[0] are predicted with its explicit weights, their
    neighbours on a farther picture without"""
    run = _encode(fade=True, mixed_refs=True, weightp=True)
    assert run["stats"].get("weightp_pictures", 0) > 0 and run["stats"]["mixed_ref_mbs"] > 0
    _check_roundtrip(host, run)
    _check_gpu_decoder(host, run["streams"])
    zero_and_far = 0
    for t in range(2, 5):
        r = run["records"][t][0]["ref"][:, 0]
        inter = np.isin(run["records"][t][0]["kind"], [P16x8, P8x16, P8x8])
        zero_and_far += int(((r == 0).any(axis=1) & (r > 0).any(axis=1) & inter).sum())
    assert zero_and_far > 0
