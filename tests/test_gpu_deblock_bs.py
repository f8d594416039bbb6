"""deblock_bs and deblock_wavefront (csrc/kernels/deblock.hip) against the numpy model of
tests/ref_models_deblock.py: direct launches on synthetic records and planes, two slots; the
strengths, the info words, the three filtered planes and ``err`` are compared.  The same planes
are also filtered through the decoder's launcher (deblock_dpb: the model's strengths in the place
of the parser's, no info words, a two-picture DPB).

Shapes (MB columns x rows): 1x1 one MB; 1x3 one column; 5x3 a small general case; 11x9 the general
case; 21x2 wider than the slack of the rings between waves; 3x35 crosses the 32-row band of the
16 waves.  What the cases cover is counted from the model (ref_models_deblock.case_counts) and
asserted: every bS value, quiet MBs beside filtered ones on each side, wave steps with only one
half quiet, with only vertical or only horizontal edges on, quiet MBs whose left / top halo a
neighbour's own edges changed, fully quiet rows -- at least ten of each over the cases.
"""
import functools

import numpy as np
import pytest
import torch

import ref_models_deblock as M

pytestmark = pytest.mark.gpu

SEED0 = 100
COVERED = ("bs0", "bs1", "bs2", "bs3", "bs4", "quiet_left_of_busy", "quiet_right_of_busy", "quiet_above_busy",
           "quiet_below_busy", "quiet_row", "step_upper_quiet", "step_lower_quiet", "step_vertical_only",
           "step_horizontal_only", "step_quiet", "quiet_left_halo_changed", "quiet_top_halo_changed", "lines_off",
           "lines_weak", "lines_strong", "lines_plain4")


@functools.lru_cache(maxsize=None)
def _case(i):
    wmb, hmb = M.SHAPES[i]
    c = M.make_case(wmb, hmb, SEED0 + i)
    return c, M.run_case(c)


@pytest.fixture(scope="module")
def hip():
    from govideocompressor_amd.ops import native
    return native.hip()


def test_cases_cover():
    tot = {}
    for i in range(len(M.SHAPES)):
        for k, n in _case(i)[1]["counts"].items():
            tot[k] = tot.get(k, 0) + n
    short = {k: tot.get(k, 0) for k in COVERED if tot.get(k, 0) < 10}
    assert not short, short


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("i", range(len(M.SHAPES)), ids=["%dx%d" % (w * 16, h * 16) for w, h in M.SHAPES])
def test_deblock_bs_and_wavefront(hip, i):
    c, want = _case(i)
    B, wmb, hmb = c["B"], c["wmb"], c["hmb"]
    nmb = wmb * hmb
    s = torch.cuda.current_stream().cuda_stream
    hdr, nz = _t(c["hdr"]), _t(c["nz"])
    bs = torch.full((B, nmb, 16), 0xA5, dtype=torch.uint8, device="cuda")
    info = torch.full((B, nmb), -1, dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.deblock_bs(B, wmb, hmb, hdr.data_ptr(), nz.data_ptr(), bs.data_ptr(), info.data_ptr(), s)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bs.cpu().numpy(), want["bs"], err_msg="strengths")
    np.testing.assert_array_equal(info.cpu().numpy().view(np.uint32), want["info"], err_msg="info words")

    # encoder launcher: [B] planes, strengths and info words of the pre-pass
    y, u, v = _t(c["y"]), _t(c["u"]), _t(c["v"])
    hip.deblock(B, wmb, hmb, y.data_ptr(), u.data_ptr(), v.data_ptr(), hdr.data_ptr(), nz.data_ptr(), c["cqo"], 0, 0,
                err.data_ptr(), s, bs=bs.data_ptr(), info=info.data_ptr())
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    for name, t in (("y", y), ("u", u), ("v", v)):
        _same(t.cpu().numpy(), want[name], c[name], "deblock " + name)

    # decoder launcher: picture cur_idx[slot] of a [B][2] DPB, the other picture stays as it is
    cur = np.array([1, 0], np.int16)[:B]
    dpb = []
    for name in ("y", "u", "v"):
        d = np.full((B, 2) + c[name].shape[1:], 0x5A, np.uint8)
        d[np.arange(B), cur] = c[name]
        dpb.append(_t(d))
    hip.deblock_dpb(B, wmb, hmb, 2, dpb[0].data_ptr(), dpb[1].data_ptr(), dpb[2].data_ptr(), _t(cur).data_ptr(),
                    hdr.data_ptr(), nz.data_ptr(), bs.data_ptr(), c["cqo"], 0, 0, err.data_ptr(), s)
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    for name, t in zip(("y", "u", "v"), dpb):
        got = t.cpu().numpy()
        _same(got[np.arange(B), cur], want[name], c[name], "deblock_dpb " + name)
        assert (got[np.arange(B), 1 - cur] == 0x5A).all(), "deblock_dpb wrote the other picture"


def _same(got, want, src, what):
    if np.array_equal(got, want):
        return
    d = np.argwhere(got != want)
    b, r, x = d[0]
    raise AssertionError("%s: %d samples differ, first slot %d row %d col %d: got %d want %d (unfiltered %d)"
                         % (what, len(d), b, r, x, got[b, r, x], want[b, r, x], src[b, r, x]))
