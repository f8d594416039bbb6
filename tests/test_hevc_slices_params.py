"""HevcParams.slices (x265 --slices): default, range, the environment knob, the x265 / x264
option tables, presets, the encoder's tag, and the one rule that maps CTU rows to slices."""
import dataclasses

import pytest

from govideocompressor_amd.jobs import ffargs
from govideocompressor_amd.models import knobs
from govideocompressor_amd.models.h264_gpu import H264Params
from govideocompressor_amd.models.hevc_gpu import GpuHevcEncoder, HevcParams
from govideocompressor_amd.rc import presets


def test_default_is_one_slice():
    p = HevcParams(64, 64)
    assert p.slices == 1 and type(p.slices) is int
    assert p.host_cfg()["slices"] == 1
    assert HevcParams(64, 64, slices=3).host_cfg()["slices"] == 3
    p.check_slices()


def test_knob():
    env = {"MIVC_HEVC_SLICES": "4"}
    over = knobs.encoder_overrides(HevcParams, env)
    assert over == {"slices": 4} and type(over["slices"]) is int
    assert dataclasses.replace(HevcParams(640, 480), **over).slices == 4
    assert knobs.encoder_overrides(H264Params, env) == {}      # H.264 keeps its own MIVC_SLICES
    s = knobs.set_knobs(env)
    assert s["unknown"] == {} and s["encoder"] == env
    with pytest.raises(SystemExit):
        knobs.check_environment(False, env)
    assert knobs.check_environment(True, env)["encoder"] == env


def test_x265_option():
    p = ffargs.parse("-vcodec libx265 -x265-params slices=4").apply_opts(HevcParams(640, 480))
    assert p.slices == 4
    p = ffargs.parse("-vcodec libx265 -x265-params bframes=3:slices=16").apply_opts(HevcParams(640, 480))
    assert (p.bframes, p.slices) == (3, 16)


@pytest.mark.parametrize("opt", ["slices=0", "slices=17", "slices=x", "slices=-1"])
def test_x265_option_refused(opt):
    with pytest.raises(ffargs.FfArgsError):
        ffargs.parse(f"-vcodec libx265 -x265-params {opt}").apply_opts(HevcParams(640, 480))


def test_x264_option_reaches_the_existing_field():
    p = ffargs.parse("-vcodec libx264 -x264-params slices=4").apply_opts(H264Params(640, 480))
    assert p.slices == 4
    assert ffargs.parse("-vcodec libx264 -x264-params slices=0").apply_opts(H264Params(640, 480, slices=2)).slices == 0
    for opt in ("slices=17", "slices=x"):
        with pytest.raises(ffargs.FfArgsError):
            ffargs.parse(f"-vcodec libx264 -x264-params {opt}").apply_opts(H264Params(640, 480))


@pytest.mark.parametrize("w,h,ctu64,rows", [(64, 64, True, 1), (64, 160, True, 3), (64, 160, False, 5),
                                            (1920, 1080, True, 17), (1920, 1080, False, 34)])
def test_range_follows_the_ctu_rows(w, h, ctu64, rows):
    assert HevcParams(w, h, ctu64=ctu64).ctu_rows() == rows
    top = min(16, rows)
    HevcParams(w, h, ctu64=ctu64, slices=top).check_slices()
    for bad in (0, -1, top + 1, 17, True, 2.0, "2"):
        with pytest.raises(ValueError, match="slices"):
            HevcParams(w, h, ctu64=ctu64, slices=bad).check_slices()


def test_constructor_refuses_before_touching_the_device():
    # 160 rows of samples = 3 CTU rows of 64: the check precedes every device call
    with pytest.raises(ValueError, match="slices"):
        GpuHevcEncoder(HevcParams(64, 160, slices=4), slots=1, device="cpu")
    with pytest.raises(ValueError, match="slices"):
        GpuHevcEncoder(HevcParams(64, 160, slices=0), slots=1, device="cpu")


@pytest.mark.parametrize("name", presets.NAMES)
def test_no_preset_sets_it(name):
    assert presets.apply(HevcParams(640, 480), name).slices == 1
    assert presets.apply(HevcParams(640, 480, slices=3), name).slices == 3


def test_tag_shows_the_slices():
    assert "slices" not in HevcParams(640, 480).describe()
    assert HevcParams(640, 480, slices=4).describe().endswith(" slices4")


def test_slice_of_row_rule(host):
    """r * S // rows: monotone, onto 0..S-1, steps of at most one; a row starts a slice exactly
    where the slice index steps."""
    for hctu in range(1, 71):
        for S in range(1, min(16, hctu) + 1):
            sl = [host.hevc_slice_of_row(r, S, hctu) for r in range(hctu)]
            assert sl == [r * S // hctu for r in range(hctu)]
            assert sl[0] == 0 and sl[-1] == S - 1 and set(sl) == set(range(S))
            assert all(0 <= b - a <= 1 for a, b in zip(sl, sl[1:]))
            starts = [host.hevc_row_starts_slice(r, S, hctu) for r in range(hctu)]
            assert starts == [r == 0 or sl[r] != sl[r - 1] for r in range(hctu)]
            assert sum(starts) == S
