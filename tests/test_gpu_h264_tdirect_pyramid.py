"""Temporal direct prediction under a b-pyramid (x264 --b-pyramid normal --direct temporal).

The co-located picture of a B picture may be the run's reference B, and a reference B may stand
in front of the anchors in list 0, so the co-located block's reference goes through
MapColToList0 (8.4.1.2.3; models/gop.py col_to_list0, csrc/kernels/h264_b.hip b_direct_mv).
Blocks whose reference is not in the current list 0 have no direct prediction: b_decide
never codes them direct.  The CPU decoder derives the mapping on its own and throws when a
direct block lacks one, so every bit-exact round trip below also proves the availability masks.
"""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, F = 176, 144, 9            # 11 x 9 MBs; IBBBPBBBP holds every case of the mapping
KIND, SEED, QP = "pan-fast", 7, 24
BASE = dict(crf=None, qp=QP, bframes=3, refs=3, pyramid=True, direct="temporal")

HDR = np.dtype([("kind", "u1"), ("cbp", "u1"), ("qp", "i1"), ("i16", "u1"), ("chroma", "u1"), ("flags", "u1"),
                ("sub_direct", "u1"), ("pad", "u1"), ("ref", "i1", (2, 4)), ("mv", "<i2", (2, 4, 2)),
                ("i4", "u1", (16,))])
assert HDR.itemsize == 64
MBK_I16, MBK_P16, MBK_B16, MBK_B8x8, MBK_BDIRECT = 1, 2, 9, 12, 13
COL_NONE = -128

_runs: dict = {}


def _encode(slots=2, entropy="gpu", anchors_at=(), slot0=0, idr_ids=None, fresh=False, **kw):
    """One encode of the shared clip -> dict(streams, recon, records, plans, stats); cached per
    configuration (``fresh``: encode again)."""
    import torch
    from govideocompressor_amd.models.h264_gpu import GpuH264Encoder, H264Params, synth_clip

    params = dict(BASE, **kw)
    key = (slots, entropy, repr(anchors_at), slot0, repr(idr_ids), tuple(sorted(params.items())))
    if key in _runs and not fresh:
        return _runs[key]
    enc = GpuH264Encoder(H264Params(width=W, height=H, **params), slots=slots, entropy=entropy)
    enc.keep_records = True
    y, u, v = synth_clip(slots, F, W, H, seed=SEED, kind=KIND, slot0=slot0)
    res = enc.encode(y, u, v, keep_recon=True, anchors_at=anchors_at, idr_ids=idr_ids)
    torch.cuda.synchronize()
    out = dict(streams=[bytes(r.bitstream) for r in res],
               recon=[[p.cpu().numpy() for p in planes] for planes in enc.last_recon],
               records=[(h.cpu().numpy().view(HDR).reshape(slots, -1), d.cpu().numpy())
                        for h, d in enc.last_records],
               plans=enc.last_plans, stats=dict(enc.stats))
    enc.close()
    if not fresh:
        _runs[key] = out
    return out


def _check_roundtrip(host, run):
    for b, stream in enumerate(run["streams"]):
        pics = host.decode(stream)  # (throws when a direct block's reference is not in list 0)
        assert len(pics) == F
        for t, pic in enumerate(pics):
            ry, ru, rv = (p[b] for p in run["recon"][t])
            assert np.array_equal(pic["y_coded"], ry), f"slot {b} frame {t}: luma differs"
            assert np.array_equal(pic["u_coded"], ru), f"slot {b} frame {t}: Cb differs"
            assert np.array_equal(pic["v_coded"], rv), f"slot {b} frame {t}: Cr differs"


# ---------------------------------------------------------------- 1. b_direct_mv, known answers
def _direct_model(col, col_l1, cmap, dsf, dcopy):
    """8.4.1.2.3 per 8x8 quadrant (direct_8x8_inference) for one slot: col [nmb] records, cmap
    [2, 4] offsets.  -> dmv [nmb, 2, 4, 2], dref [nmb, 4], pm0 / pm1 [nmb, 2], czero [nmb].
    A quadrant whose co-located reference is not in list 0 (dref -1) has zero vectors and does
    not count in the ME predictors: they are the mean, rounded half up, of the vectors of the
    quadrants that have a direct prediction (zero when none has)."""
    nmb = len(col)
    dmv = np.zeros((nmb, 2, 4, 2), np.int64)
    dref = np.zeros((nmb, 4), np.int64)
    pm = np.zeros((2, nmb, 2), np.int64)
    cz = np.zeros(nmb, np.int64)
    for mb in range(nmb):
        c = col[mb]
        intra = int(c["kind"]) in (0, 1, 4, 8)
        n = 0
        for q in range(4):
            cl = 1 if (col_l1 and c["ref"][0][q] < 0) else 0
            none = intra or c["ref"][cl][q] < 0
            cx, cy = (0, 0) if none else (int(c["mv"][cl][q][0]), int(c["mv"][cl][q][1]))
            rc = 0 if none else min(int(c["ref"][cl][q]), 3)
            rm = 0 if none else (-1 if cmap[cl][rc] == COL_NONE else rc + int(cmap[cl][rc]))
            dref[mb, q] = rm
            if not none and c["ref"][cl][q] == 0 and abs(cx) <= 1 and abs(cy) <= 1:
                cz[mb] |= 1 << q  # colZeroFlag is defined on refIdxCol
            if rm < 0:
                continue
            n += 1
            for k, cv in enumerate((cx, cy)):
                if dcopy[rm]:
                    dmv[mb, 0, q, k], dmv[mb, 1, q, k] = cv, 0
                else:
                    l0 = (int(dsf[rm]) * cv + 128) >> 8
                    dmv[mb, 0, q, k], dmv[mb, 1, q, k] = l0, l0 - cv
        if n:
            pm[:, mb] = np.floor_divide(2 * dmv[mb].sum(axis=1) + n, 2 * n)
    return dmv, dref, pm[0], pm[1], cz


def _col_records(rng, nmb, b_picture):
    """Hand-built co-located records: intra MBs, list-0, list-1-only and bi-predicted quadrants
    over every refIdxCol, vectors of both signs (the rounding of (dsf * mv + 128) >> 8), and
    near-zero vectors (colZeroFlag)."""
    col = np.zeros(nmb, HDR)
    col["kind"] = rng.choice([MBK_I16, MBK_B16 if b_picture else MBK_P16, MBK_B8x8 if b_picture else MBK_P16], nmb,
                             p=[0.15, 0.5, 0.35])
    col["ref"][:, 0] = rng.integers(0, 4, (nmb, 4))
    col["ref"][:, 1] = -1
    if b_picture:
        col["ref"][:, 1] = rng.integers(-1, 2, (nmb, 4))
        l1_only = rng.random((nmb, 4)) < 0.4
        col["ref"][:, 0][l1_only] = -1
        col["ref"][:, 1][l1_only] = rng.integers(0, 2, int(l1_only.sum()))
    mv = rng.integers(-300, 301, (nmb, 2, 4, 2))
    small = rng.random((nmb, 1, 4, 1)) < 0.2
    col["mv"] = np.where(small, rng.integers(-2, 3, mv.shape), mv)
    if not b_picture:
        # refIdxCol 2 is the entry the test maps to "none": MBs with 4, 1, 2 and 3 such quadrants
        # (the ME predictors over 0, 3, 2 and 1 vectors), the second one with negative vectors
        col["kind"][5:9] = MBK_P16
        col["ref"][5:9, 0] = [[2, 2, 2, 2], [2, 0, 1, 0], [2, 2, 0, 3], [2, 2, 2, 1]]
        col["mv"][6, 0] = [[9, 9], [-7, -13], [-22, -1], [-5, -3]]
    return col


def _run_b_direct(cols, routes, cmap, nbuf):
    import torch
    from govideocompressor_amd.ops import native

    hip = native.hip()
    B, nmb = len(routes), cols.shape[2]
    wmb, hmb = 20, nmb // 20
    dev = "cuda"
    pool = torch.from_numpy(cols.view(np.uint8).reshape(B, nbuf, nmb, 64).copy()).to(dev)
    rt = torch.from_numpy(routes.view(np.uint8).reshape(B, -1).copy()).to(dev)
    dmv = torch.full((B, nmb, 2, 4, 2), 0x5555, dtype=torch.int16, device=dev)
    dref = torch.full((B, nmb, 4), 0x55, dtype=torch.int8, device=dev)
    pm0 = torch.full((B, nmb, 2), 0x5555, dtype=torch.int16, device=dev)
    pm1 = torch.full((B, nmb, 2), 0x5555, dtype=torch.int16, device=dev)
    cz = torch.full((B, nmb), 0x55, dtype=torch.uint8, device=dev)
    cm = None if cmap is None else torch.from_numpy(np.ascontiguousarray(cmap, dtype=np.int8)).to(dev)
    hip.b_direct(B, wmb, hmb, pool.data_ptr(), [0], [1], dmv.data_ptr(), pm0.data_ptr(), pm1.data_ptr(),
                 torch.cuda.current_stream().cuda_stream, dref.data_ptr(), rt.data_ptr(), nbuf, cz.data_ptr(),
                 0 if cm is None else cm.data_ptr())
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (dmv, dref, pm0, pm1, cz)]


def _direct_case():
    from govideocompressor_amd.models.h264_gpu import ROUTE_DTYPE

    rng = np.random.default_rng(20)
    B, nbuf, nmb = 3, 3, 20 * 14  # 280 MBs: two workgroups, the second one partial
    cols = np.zeros((B, nbuf, nmb), HDR)
    rt = np.zeros(B, ROUTE_DTYPE)
    rt["kind"] = [1, 1, 0]           # two B slots, one P slot (which b_direct_mv must leave alone)
    rt["l1"] = [2, 1, 0]             # the co-located pictures' pool buffers
    rt["col_l1"] = [0, 1, 0]         # slot 1: the co-located picture is a reference B
    rt["n0"] = [3, 2, 1]
    rt["dsf"] = [[128, 85, -64, 300], [192, 51, 700, -1024], [0, 0, 0, 0]]
    rt["dcopy"] = [[0, 0, 0, 1], [0, 1, 0, 0], [1, 1, 1, 1]]
    rt["w1"], rt["disp"], rt["l0"] = 32, -1, -1
    cols[0, 2] = _col_records(rng, nmb, False)
    cols[1, 1] = _col_records(rng, nmb, True)
    cols[2, 0] = _col_records(rng, nmb, False)
    # slot 0 (after the reference B): 0 -> 1, 1 -> 2, 2 -> none, 3 -> 3 (a dcopy entry)
    # slot 1 (before it): list 0 0 -> 0, 1 -> none, 2 -> 1, 3 -> none; list 1: 0 -> none, 1 -> 1
    cmap = np.array([[[1, 1, COL_NONE, 0], [0, 0, 0, 0]],
                     [[0, COL_NONE, -1, COL_NONE], [COL_NONE, 0, 0, 0]],
                     [[0, 0, 0, 0], [0, 0, 0, 0]]], np.int8)
    return cols, rt, cmap, nbuf


@pytest.mark.parametrize("mapped", [True, False], ids=["mapped", "zero-map"])
def test_b_direct_mv_known_answers(mapped):
    cols, rt, cmap, nbuf = _direct_case()
    if not mapped:
        cmap = np.zeros_like(cmap)
    got = _run_b_direct(cols, rt, cmap, nbuf)
    names = ("dmv", "dref", "pm0", "pm1", "czero")
    for b in range(2):
        want = _direct_model(cols[b, rt["l1"][b]], bool(rt["col_l1"][b]), cmap[b], rt["dsf"][b], rt["dcopy"][b])
        for name, g, w in zip(names, got, want):
            assert np.array_equal(g[b].astype(np.int64), w), f"slot {b}: {name}"
    for name, g, sent in zip(names, got, (0x5555, 0x55, 0x5555, 0x5555, 0x55)):
        assert (g[2] == sent).all(), f"the P slot's {name} was written"
    dref = got[1][:2]
    if mapped:
        # by construction: every case occurs
        l1_only = (cols[1, 1]["ref"][:, 0] < 0) & (cols[1, 1]["kind"][:, None] != MBK_I16)
        assert l1_only.any() and (dref[1][l1_only] == -1).any() and (dref[1][l1_only] == 1).any()
        assert (dref[0] == -1).any() and (dref[0] > 0).any() and (dref == 3).any()
        assert ((dref[0] == -1).sum(axis=1) == 4).any() and (((dref[0] == -1).sum(axis=1) % 4) != 0).any()
        assert (cols[0, 2]["kind"] == MBK_I16).any() and (cols[0, 2]["mv"] < 0).any()
    else:
        # the identity: what the kernel computes with no table at all (the unmapped semantics)
        plain = _run_b_direct(cols, rt, None, nbuf)
        for name, g, p in zip(names, got, plain):
            assert np.array_equal(g, p), name
        assert (dref >= 0).all()


# ---------------------------------------------------------------- 2. round trips
CASES = {
    "refs3": dict(),
    "refs1": dict(refs=1),
    "no-bparts": dict(bpartitions=False),
    "no-gate": dict(b_gate=0),
    "no-gate-no-bparts": dict(b_gate=0, bpartitions=False),
    "slices2": dict(slices=2),
    "no-weightb": dict(weightb=False),
}


@pytest.mark.parametrize("case", list(CASES))
def test_tdirect_pyramid_roundtrip(host, case):
    run = _encode(**CASES[case])
    assert any(q.kind == "B" and q.ref for q in run["plans"][0])
    _check_roundtrip(host, run)


# ---------------------------------------------------------------- 3. the new paths are taken
def _direct_stats(run):
    """Counts over the kept records: direct quadrants (B_Direct_16x16 / B_Skip / B_Direct_8x8)
    in pictures whose co-located picture is a B, direct quadrants with refIdxL0 >= 1 in
    pictures that follow the run's reference B, MBs with a quadrant without direct prediction."""
    n = dict(col_b=0, after_ref=0, unavail_mbs=0, unavail_direct=0, ref_mismatch=0)
    for b, plan in enumerate(run["plans"]):
        by_d = {p.d: p for p in plan}
        for t, pic in enumerate(plan):
            if pic.kind != "B":
                continue
            hdr, dref = run["records"][t][0][b], run["records"][t][1][b]
            dq = (hdr["kind"] == MBK_BDIRECT)[:, None] | (
                (hdr["kind"] == MBK_B8x8)[:, None] & (((hdr["sub_direct"][:, None] >> np.arange(4)) & 1) == 1))
            n["unavail_mbs"] += int((dref < 0).any(axis=1).sum())
            n["unavail_direct"] += int((dq & (dref < 0)).sum())
            n["ref_mismatch"] += int((dq & (hdr["ref"][:, 0] != dref)).sum())
            if by_d[pic.l1].kind == "B":
                n["col_b"] += int(dq.sum())
            if by_d[pic.refs0[0]].kind == "B":
                n["after_ref"] += int((dq & (hdr["ref"][:, 0] >= 1)).sum())
    return n


def test_tdirect_pyramid_not_vacuous():
    run = _encode()
    n = _direct_stats(run)
    print("direct statistics:", n, "unavailable share:", run["stats"].get("direct_unavail_ratio"))
    assert n["unavail_direct"] == 0, "a quadrant without a direct prediction was coded direct"
    assert n["ref_mismatch"] == 0, "a direct quadrant's record does not carry the mapped refIdxL0"
    assert n["col_b"] > 0 and n["after_ref"] > 0 and n["unavail_mbs"] > 0, n
    nb = sum(1 for plan in run["plans"] for p in plan if p.kind == "B")
    assert run["stats"]["direct_unavail_ratio"] == pytest.approx(n["unavail_mbs"] / (nb * 99))


# ---------------------------------------------------------------- 4. per-slot plans
def test_tdirect_pyramid_per_slot_plans(host):
    anchors = [[], [1], [1, 2]]
    run = _encode(slots=3, anchors_at=anchors)
    plans = run["plans"]
    by_d = [{p.d: p for p in plan} for plan in plans]

    def role(b, t):
        p = plans[b][t]
        return p.kind if p.kind != "B" else "B<-" + by_d[b][p.l1].kind
    assert any({role(b, t) for b in range(3)} == {"P", "B<-P", "B<-B"} for t in range(F)), \
        [[role(b, t) for b in range(3)] for t in range(F)]
    _check_roundtrip(host, run)
    for b in range(3):
        alone = _encode(slots=1, anchors_at=[anchors[b]], slot0=b, idr_ids=[b])
        assert alone["streams"][0] == run["streams"][b], f"slot {b}: bytes depend on the other slots"


# ---------------------------------------------------------------- 5. / 6. entropy coders, determinism
def test_tdirect_pyramid_gpu_cabac_equals_host_writer():
    assert _encode()["streams"] == _encode(entropy="cpu")["streams"]


def test_tdirect_pyramid_deterministic():
    assert _encode()["streams"] == _encode(fresh=True)["streams"]


# ---------------------------------------------------------------- 7. GPU decode
def test_tdirect_pyramid_gpu_decode(host):
    from govideocompressor_amd.models.h264_decode_gpu import GpuH264Decoder

    streams = _encode()["streams"]
    dec = GpuH264Decoder()
    out = dec.decode(streams)
    assert dec.stats["segments_cpu"] == 0
    for s, d in zip(streams, out):
        ref = host.decode(s)
        assert d.path == "gpu" and d.frames == len(ref) == F
        y, u, v = d.y.cpu().numpy(), d.u.cpu().numpy(), d.v.cpu().numpy()
        for t, p in enumerate(ref):
            b = p["i420"]
            ys, cs = W * H, (W // 2) * (H // 2)
            assert np.array_equal(y[t], b[:ys].reshape(H, W)), f"picture {t}: luma"
            assert np.array_equal(u[t], b[ys:ys + cs].reshape(H // 2, W // 2)), f"picture {t}: Cb"
            assert np.array_equal(v[t], b[ys + cs:].reshape(H // 2, W // 2)), f"picture {t}: Cr"


# ---------------------------------------------------------------- 8. existing behaviour
# SHA-256 over the two slots' streams of the shared clip, measured with the encoder and kernels
# of commit b46e9fa (the parent of the change that added the map): the pyramid with spatial
# direct and temporal direct without a pyramid keep their bytes.
PARENT_SHA256 = {
    "pyramid-spatial": "f4d2087c953c880b4d7eddba5931b8f29d6711e1bdd797676bef725cb49a4a3e",
    "temporal-flat": "2a408e3e0ae65604253ab175117776cdd3b005ddb89be09e2e7c89faf38b0f3d",
}
PARENT_CONFIGS = {
    "pyramid-spatial": dict(pyramid=True, direct="spatial"),
    "temporal-flat": dict(pyramid=False, direct="temporal"),
}


def _sha(streams):
    return hashlib.sha256(b"".join(streams)).hexdigest()


@pytest.mark.parametrize("name", list(PARENT_CONFIGS))
def test_existing_configurations_keep_their_bytes(name):
    assert _sha(_encode(**PARENT_CONFIGS[name])["streams"]) == PARENT_SHA256[name]
