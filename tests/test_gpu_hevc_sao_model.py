"""HEVC SAO (csrc/kernels/hevc_filters.hip: ``hevc_sao``, ``hevc_sao_stats64``, ``sao_decide``,
``hevc_sao_apply``) against the numpy model of tests/ref_models.py.

The decoder comparison only shows that the parameters in the CTU records were applied as written.
Here ``hip.hevc_sao`` runs on planted planes and
  * the parameters in the records must be the ones ``sao_decide`` derives from ``sao_stats`` (for
    all three forms of the statistics: the 32x32 tile pass, the tile pass over the four record
    blocks of a 64x64 CTU -- ``MIVC_HEVC_SAO_TILE=1``, in a child process -- and the column-per-lane
    pass ``hevc_sao_stats64``),
  * the output planes must equal ``sao_apply`` of the kernel's own records, everywhere,
  * the change of every CTU component's squared error must be the integer the statistics predict,
  * untouched record bytes and the planes and records of an idle slot keep a sentinel.

Every quantity is an integer and compared exactly.  The one exception is a comparison of two
float64 prices that the host and the device may settle differently (``exp2``, contraction of
``dd + lam * r`` into a fused multiply-add).  The model flags a group ``near_tie`` when a candidate
with another effect on the picture prices within 1e-9 (relative) of the chosen one without being
equal to it, or when a shrink / drop comparison on the chosen candidate's path lies that close;
1e-9 is about five orders above the rounding of these twenty-odd double operations.  A flagged
group must still price, by ``sao_cost``, within 1e-9 of the model's optimum, and at most 5 % of a
test's groups may be flagged.  One more difference is harmless by construction and treated the same
way without counting as flagged: parameters that differ from the model's but do the same to the
picture at the same price -- band windows that hold the same occupied bands (a flat block has one)
price equally up to the order of their sums, and which of them is "first cheapest" depends on that
rounding.  Each test prints its shares; measured on an MI355X they are recorded in
``test_content_reaches_every_outcome``'s docstring.
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import ref_models as rm

pytestmark = pytest.mark.gpu

_SENTINEL_BYTE, _SENTINEL_SAMPLE = 0xA5, 0x5A5A
_NEAR_TIE_CAP = 0.05
_cache = {}


# ------------------------------------------------------------------ content
def _blur(a):
    """4-tap blur: the mean of a sample, its right, lower and lower-right neighbour (edge repeated)."""
    p = np.pad(a, ((0, 1), (0, 1)), mode="edge")
    return (p[:-1, :-1] + p[:-1, 1:] + p[1:, :-1] + p[1:, 1:]) / 4.0


def _content(W, H, bd, qp=30, seed=1):
    """(deb, src): three int64 planes each.  Waves plus noise as the source, the source plus
    coding-like noise, blurred, as the deblocked picture; luma columns 64 .. 127 are a smooth ramp
    whose deblocked samples of levels 96 .. 127 sit 3 too high (band offset pays), columns 128 .. 191
    are deblocked == source (off)."""
    key = (W, H, bd, qp, seed)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(seed)
    deb, src = [], []
    for c in range(3):
        h, w, sub = (H, W, 0) if c == 0 else (H // 2, W // 2, 1)
        yy, xx = np.mgrid[0:h, 0:w]
        X, Y = xx << sub, yy << sub
        s = 128 + 60 * np.sin(X / 9.0 + c) * np.cos(Y / 7.0 - c) + rng.normal(0, 6, (h, w))
        s = np.clip(np.rint(s), 16, 235).astype(np.int64)
        d = _blur(s + rng.normal(0, 1.5 * 2.0 ** ((qp - 22) / 6.0), (h, w)))
        d = np.clip(np.rint(d), 0, 255).astype(np.int64)
        ramp = 88 + (X - 64) // 2 + (Y % 32) // 8 + 2 * c
        band = (X >= 64) & (X < 128)
        s = np.where(band, ramp, s)
        d = np.where(band, ramp + 3 * ((ramp >= 96) & (ramp < 128)), d)
        d = np.where((X >= 128) & (X < 192), s, d)
        if bd == 10:
            low = rng.integers(0, 4, (h, w))
            s, d = s * 4 + low, d * 4 + low
        deb.append(d)
        src.append(s)
    _cache[key] = (deb, src)
    return deb, src


def _block_qps(B, W, H, base=22):
    """A different QP per record block and slot, 22 .. 37, multiples of 3 among them."""
    wb, hb = W // 32, H // 32
    b, y, x = np.mgrid[0:B, 0:hb, 0:wb]
    qp = (base + (x * 5 + y * 3 + b * 7) % 16).astype(np.int32)
    assert B * wb * hb < 3 or ((qp % 3 == 0).any() and (qp % 3 != 0).any())
    return qp.reshape(B, hb * wb)


# ------------------------------------------------------------------ the kernel
def _run_sao(deb, src, qp, bd, ctu64, run=None, enable=1):
    """deb, src: three [B, h, w] arrays; qp: [B, blocks].  -> records [B, blocks, 32] uint8 and the
    three output planes, both prefilled with the sentinel."""
    import torch
    from govideocompressor_amd.ops import native

    hip = native.hip()
    B, H, W = deb[0].shape
    run = [1] * B if run is None else run
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.uint16).view(np.int16)).cuda()  # noqa: E731
    d, s = [dev(p) for p in deb], [dev(p) for p in src]
    o = [torch.full_like(p, _SENTINEL_SAMPLE) for p in d]
    rec = torch.full((B, (W // 32) * (H // 32), 32), _SENTINEL_BYTE, dtype=torch.uint8).cuda()
    q = torch.from_numpy(np.ascontiguousarray(qp, dtype=np.int32)).cuda()
    r = torch.tensor(run, dtype=torch.int8).cuda()
    P = lambda t: t.data_ptr()  # noqa: E731
    hip.hevc_sao(B, W, H, bd, P(d[0]), P(d[1]), P(d[2]), P(o[0]), P(o[1]), P(o[2]), P(s[0]), P(s[1]), P(s[2]), P(rec),
                 P(q), P(r), enable, torch.cuda.current_stream().cuda_stream, ctu64)
    torch.cuda.synchronize()
    for a, b in zip(d, [dev(p) for p in deb]):
        assert torch.equal(a, b), "the deblocked input was written"
    return rec.cpu().numpy(), [p.cpu().numpy().view(np.uint16).astype(np.int64) for p in o]


def _params(rec, W, H):
    """records [blocks, 32] of one slot -> the parameter arrays sao_apply takes, per record block."""
    hb, wb = H // 32, W // 32
    r = rec.reshape(hb, wb, 32)
    return dict(type=r[:, :, 2:4].astype(np.int64), cls=r[:, :, 4:6].astype(np.int64), band=r[:, :, 6:9].astype(np.int64),
                off=r[:, :, 10:22].view(np.int8).astype(np.int64).reshape(hb, wb, 3, 4))


def _check_slot(rec, out, deb, src, qp, bd, ctu64, W, H, what):
    """One running slot against the model -> (groups, flagged, same-effect differences, type counts)."""
    hb, wb = H // 32, W // 32
    raw = rec.reshape(hb, wb, 32)
    untouched = np.r_[0:2, 9:10, 22:32]
    assert (raw[:, :, untouched] == _SENTINEL_BYTE).all(), f"{what}: a record byte outside the SAO fields was written"
    par = _params(rec, W, H)
    # ---- apply: the kernel's own records on the deblocked picture, everywhere
    want = rm.sao_apply(deb, par, bd)
    for c in range(3):
        bad = np.argwhere(out[c] != want[c])
        assert bad.size == 0, (f"{what}: plane {c}: {len(bad)} samples differ from sao_apply, first {bad[0].tolist()}: "
                               f"{out[c][tuple(bad[0])]} != {want[c][tuple(bad[0])]} (deblocked {deb[c][tuple(bad[0])]})")
    # ---- decision per CTU
    n = 2 if ctu64 else 1
    groups = flagged = same_effect = 0
    types = np.zeros((2, 3), dtype=np.int64)
    qpb = np.asarray(qp).reshape(hb, wb)
    top = (1 << bd) - 1
    for by in range(0, hb, n):
        for bx in range(0, wb, n):
            st = rm.sao_stats(deb, src, bd, bx * 32, by * 32, 32 * n)
            dec = rm.sao_decide(st, int(qpb[by, bx]), bd)
            got = {k: v[by, bx].tolist() for k, v in par.items()}
            for yy in range(by, min(by + n, hb)):      # every record block of the CTU carries the parameters
                for xx in range(bx, min(bx + n, wb)):
                    assert raw[yy, xx, 2:22].tolist() == raw[by, bx, 2:22].tolist(), f"{what}: CTU {bx},{by}: records differ"
            for g in (0, 1):
                comps = (0,) if g == 0 else (1, 2)
                groups += 1
                types[g, got["type"][g]] += 1
                where = f"{what}: block {bx},{by} group {g} qp {qpb[by, bx]}: kernel {got}, model {dec}"
                assert got["type"][g] in (0, 1, 2) and 0 <= got["cls"][g] < 4, where
                if got["type"][g] == 0:
                    assert all(got["off"][c] == [0] * 4 for c in comps), where
                same = got["type"][g] == dec["type"][g] and all(got["off"][c] == dec["off"][c] for c in comps)
                if same and dec["type"][g] == 2:
                    same = got["cls"][g] == dec["cls"][g]
                if same and dec["type"][g] == 1:
                    same = all(got["band"][c] == dec["band"][c] for c in comps)
                flagged += dec["near_tie"][g]
                if not same:
                    eff = [rm.sao_effect(st, g, p["type"][g], p["cls"][g], p["band"], p["off"]) for p in (got, dec)]
                    assert dec["near_tie"][g] or eff[0] == eff[1], where
                    same_effect += not dec["near_tie"][g]
                    cost = rm.sao_cost(st, dec["lam"], got, g)
                    assert abs(cost - dec["cost"][g]) <= rm.SAO_NEAR_TIE * max(abs(cost), abs(dec["cost"][g])), where
            # ---- the squared error against the source moves by what the statistics say
            for c in range(3):
                sub = 1 if c else 0
                ys = slice(by * 32 >> sub, (by + n) * 32 >> sub)
                xs = slice(bx * 32 >> sub, (bx + n) * 32 >> sub)
                d, s, o = deb[c][ys, xs], src[c][ys, xs], out[c][ys, xs]
                delta = int(((s - o) ** 2).sum() - ((s - d) ** 2).sum())
                unclipped = int((o - d).min()) >= 0 or int(d.min()) > 31
                unclipped &= int((o - d).max()) <= 0 or int(d.max()) < top - 31
                if unclipped:       # no sample can have met 0 or the top
                    assert delta == rm.sao_sse_delta(st, got, c), f"{what}: block {bx},{by} plane {c}: SSE change"
    return groups, flagged, same_effect, types


def _check(rec, out, deb, src, qp, bd, ctu64, run, what):
    """All slots: running ones against the model, idle ones against the sentinel."""
    B, H, W = deb[0].shape
    tot = np.zeros(3, dtype=np.int64)
    types = np.zeros((2, 3), dtype=np.int64)
    for b in range(B):
        if not run[b]:
            assert (rec[b] == _SENTINEL_BYTE).all(), f"{what}: records of idle slot {b} written"
            assert all((p[b] == _SENTINEL_SAMPLE).all() for p in out), f"{what}: planes of idle slot {b} written"
            continue
        g, f, e, t = _check_slot(rec[b], [p[b] for p in out], [p[b] for p in deb], [p[b] for p in src], qp[b], bd, ctu64,
                                 W, H, f"{what} slot {b}")
        tot += (g, f, e)
        types += t
    share = tot[1] / max(tot[0], 1)
    print(f"{what}: {tot[0]} groups, near-tie share {share:.4f}, same effect under other parameters {tot[2]}, "
          f"types off / band / edge luma {types[0].tolist()} chroma {types[1].tolist()}")
    assert share <= _NEAR_TIE_CAP
    return types


def _stack(items):
    """[(deb, src), ...] of single pictures -> ([B, h, w] x 3, [B, h, w] x 3)"""
    return ([np.stack([it[0][c] for it in items]) for c in range(3)],
            [np.stack([it[1][c] for it in items]) for c in range(3)])


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("ctu64", [0, 1])
def test_content_reaches_every_outcome(bd, ctu64):
    """224x160 (a partial CTU column at 64x64), three slots with the middle one idle, a QP per
    record block: the parameters, planes and SSE changes follow the model, every CTU row holds
    off, band and edge luma CTUs, and the idle slot keeps its sentinel.

    Measured on an MI355X: near-tie share 0 of 140 groups (32x32 blocks) and 0 of 48 (64x64 CTUs)
    at either bit depth, 0 in every other test of this file (2 .. 48 groups each); parameters that
    differed from the model's with the same effect and price: 4 of 140, 1 of 48 here, at most 1 per
    test elsewhere (band windows over the same occupied bands); no other difference."""
    W, H, B, run = 224, 160, 3, [1, 0, 1]
    deb, src = _stack([_content(W, H, bd, 30, seed) for seed in (1, 2, 3)])
    qp = _block_qps(B, W, H)
    rec, out = _run_sao(deb, src, qp, bd, ctu64, run)
    types = _check(rec, out, deb, src, qp, bd, ctu64, run, f"224x160 bd {bd} ctu64 {ctu64}")
    assert (types > 0).all(), "the content misses an outcome"
    par = _params(rec[0], W, H)
    for row in par["type"][:, :, 0]:
        assert set(row.tolist()) == {0, 1, 2}, "a CTU row misses an outcome"


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("W,H,ctu64", [(32, 32, 0), (64, 64, 0), (64, 64, 1), (96, 96, 1), (96, 96, 0)])
def test_small_pictures(W, H, ctu64, bd):
    """One block / one CTU (every sample class at a picture edge) and 96x96 with 64x64 CTUs:
    partial CTUs on the right and at the bottom and a corner CTU of a single record block."""
    deb, src = _stack([_content(W, H, bd, 27, seed=4)])
    qp = _block_qps(1, W, H, base=24)
    rec, out = _run_sao(deb, src, qp, bd, ctu64)
    _check(rec, out, deb, src, qp, bd, ctu64, [1], f"{W}x{H} bd {bd} ctu64 {ctu64}")


def _planted(bd):
    """192x128, six 64x64 CTUs.  Top row: flat | one band, source far below | one band, source far
    above.  Bottom row: waves and noise (its edge columns differ from the neighbours' adjacent
    columns, luma and chroma) | 0 .. 2 against source 0 | top - 2 .. top against source top (x 4
    plus low bits at 10 bits)."""
    key = ("planted", bd)
    if key in _cache:
        return _cache[key]
    W, H = 192, 128
    top = (1 << bd) - 1
    deb, src = (list(p) for p in _content(W, H, bd, 30, seed=5))
    deb, src = [p.copy() for p in deb], [p.copy() for p in src]
    rng = np.random.default_rng(7)       # no near tie by the model at either CTU size (seed 6 draws one, in a clip CTU)
    for c in range(3):
        n = 32 if c else 64
        cell = lambda cx, cy: (slice(cy * n, cy * n + n), slice(cx * n, cx * n + n))  # noqa: E731
        deb[c][cell(0, 0)], src[c][cell(0, 0)] = 100 << (bd - 8), (103 + c) << (bd - 8)
        deb[c][cell(1, 0)], src[c][cell(1, 0)] = top, 0
        deb[c][cell(2, 0)], src[c][cell(2, 0)] = 0, top
        few = lambda: rng.integers(0, 3, (n, n)) * (1 << (bd - 8)) + rng.integers(0, 1 << (bd - 8), (n, n))  # noqa: E731
        deb[c][cell(1, 1)], src[c][cell(1, 1)] = few(), 0
        deb[c][cell(2, 1)], src[c][cell(2, 1)] = top - few(), top
    _cache[key] = (deb, src)
    return deb, src


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("ctu64", [0, 1])
def test_planted_ctus(bd, ctu64):
    """Flat (no edge category), a whole CTU in one band with source - picture = -top and +top (the
    sign and the 16-bit count field of the packed histogram: 4096 samples, sums of +-1044480 /
    +-4190208), offsets that clip at 0 and at the top, and a CTU of ordinary content beside them."""
    W, H = 192, 128
    deb, src = _stack([_planted(bd)])
    top = (1 << bd) - 1
    st = rm.sao_stats([p[0] for p in deb], [p[0] for p in src], bd, 0, 0, 64)
    # flat: one band, and no edge category but in the column beside the next CTU and the row above the one below
    assert st["bo_cnt"][0].max() == 4096 and st["eo_cnt"][0, 0].sum() == 64 and 0 < st["eo_cnt"][0, 1].sum() <= 64
    st = rm.sao_stats([p[0] for p in deb], [p[0] for p in src], bd, 64, 0, 64)
    assert st["bo_cnt"][0, 31] == 4096 and st["bo_sum"][0, 31] == -top * 4096
    st = rm.sao_stats([p[0] for p in deb], [p[0] for p in src], bd, 128, 0, 64)
    assert st["bo_cnt"][0, 0] == 4096 and st["bo_sum"][0, 0] == top * 4096
    qp = np.full((1, 24), 22, dtype=np.int32)
    rec, out = _run_sao(deb, src, qp, bd, ctu64)
    _check(rec, out, deb, src, qp, bd, ctu64, [1], f"planted bd {bd} ctu64 {ctu64}")
    par = _params(rec[0], W, H)
    cmax = rm.sao_offset_max(bd)
    # the far-off CTUs take the largest band offset, towards the source
    assert par["type"][0, 2, 0] == 1 and par["off"][0, 2, 0, (31 - par["band"][0, 2, 0]) & 31] == -cmax
    assert par["type"][0, 4, 0] == 1 and par["off"][0, 4, 0, (0 - par["band"][0, 4, 0]) & 31] == cmax
    # the clipping CTUs: offsets that push samples past 0 / the top, clipped in the output
    free = rm.sao_apply([p[0] for p in deb], par, bd, clip=False)
    for c in range(3):
        n = 32 if c else 64
        assert free[c][n:2 * n, n:2 * n].min() < 0 and out[c][0, n:2 * n, n:2 * n].min() == 0
        assert free[c][n:2 * n, 2 * n:3 * n].max() > top and out[c][0, n:2 * n, 2 * n:3 * n].max() == top


@pytest.mark.parametrize("ctu64", [0, 1])
def test_disabled_writes_type_0_and_copies(ctu64):
    W, H, bd = 96, 64, 8
    deb, src = _stack([_content(W, H, bd, 30, seed=7)])
    qp = _block_qps(1, W, H)
    rec, out = _run_sao(deb, src, qp, bd, ctu64, enable=0)
    par = _params(rec[0], W, H)
    assert not par["type"].any() and not par["off"].any()
    for c in range(3):
        assert np.array_equal(out[c], deb[c])


def _tile_cases():
    """The 64x64-CTU cases whose records and planes the two statistics passes must share."""
    cases = []
    for bd in (8, 10):
        cases.append((_stack([_content(224, 160, bd, 30, seed) for seed in (1, 2, 3)]), _block_qps(3, 224, 160), bd, [1, 0, 1]))
        cases.append((_stack([_content(96, 96, bd, 27, seed=4)]), _block_qps(1, 96, 96, base=24), bd, [1]))
        cases.append((_stack([_planted(bd)]), np.full((1, 24), 22, dtype=np.int32), bd, [1]))
    return cases


def _ctu64_digests():
    out = []
    for (deb, src), qp, bd, run in _tile_cases():
        rec, planes = _run_sao(deb, src, qp, bd, 1, run)
        h = hashlib.sha256(rec.tobytes())
        for p in planes:
            h.update(np.ascontiguousarray(p).tobytes())
        out.append(h.hexdigest())
    return out


def test_tile_pass_gives_the_same_bytes():
    """``MIVC_HEVC_SAO_TILE=1`` (the LDS-tile statistics over the four record blocks of a CTU and
    the per-block apply) writes the records and planes of the default path byte for byte.  The
    launcher reads the variable once, so the other run is a child process."""
    here = _ctu64_digests()
    code = ("import sys; sys.path.insert(0, 'tests'); import test_gpu_hevc_sao_model as t; "
            "print(' '.join(t._ctu64_digests()))")
    env = dict(os.environ, MIVC_HEVC_SAO_TILE="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=110,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split()[-len(here):] == here


@pytest.mark.parametrize("w,h", [(96, 64), (128, 96)])
def test_encoder_call_follows_the_model(w, h):
    """A one-picture intra encode with 64x64 CTUs: the encoder's deblocked picture (``dbk`` after
    the ping-pong swap), source, per-block QPs and CTU records satisfy the same model -- the
    argument order of the real call."""
    import torch
    from govideocompressor_amd.models.h264_gpu import synth_clip
    from govideocompressor_amd.models.hevc_gpu import GpuHevcEncoder, HevcParams

    y, u, v = synth_clip(1, 1, w, h, seed=7)
    enc = GpuHevcEncoder(HevcParams(width=w, height=h, intra_only=True, crf=None, qp=30, sao=True, ctu64=True), slots=1)
    enc.encode(y, u, v, keep_recon=True)
    torch.cuda.synchronize()
    np16 = lambda t: t.cpu().numpy().view(np.uint16).astype(np.int64)  # noqa: E731
    deb, src = [np16(p) for p in enc.dbk], [np16(p) for p in enc.src]
    out = [np16(p) for p in enc.last_recon[0]]
    rec, qp = enc.ctu.cpu().numpy(), enc.ctb_qp.cpu().numpy()
    assert deb[0].shape == (1, enc.H, enc.W) and rec.shape == (1, enc.nctb, 32)
    enc.close()
    rec = rec.copy()
    keep = np.r_[0:2, 9:10, 22:32]        # the encoder's other fields: not under test here
    rec[:, :, keep] = _SENTINEL_BYTE
    types = _check(rec, out, deb, src, qp, 8, 1, [1], f"encode {w}x{h}")
    assert types[:, 1:].sum() > 0, "the encode never switched SAO on"
