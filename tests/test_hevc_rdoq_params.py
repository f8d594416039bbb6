"""HevcParams.rdoq_level / rdoq_lambda (x265 --rdoq-level): defaults, the x265 option, the
environment knobs, and that no preset turns the tool on."""
import dataclasses

import pytest

from govideocompressor_amd.jobs import ffargs
from govideocompressor_amd.models import knobs
from govideocompressor_amd.models.hevc_gpu import HevcParams
from govideocompressor_amd.rc import presets


def test_defaults():
    p = HevcParams(64, 64)
    assert p.rdoq_level == 0 and type(p.rdoq_level) is int
    assert p.rdoq_lambda == 0.5 and type(p.rdoq_lambda) is float
    assert "rdoq_level" not in p.host_cfg() and "rdoq_lambda" not in p.host_cfg()  # no syntax of its own


@pytest.mark.parametrize("level", [0, 1, 2])
def test_x265_option(level):
    p = ffargs.parse(f"-vcodec libx265 -x265-params rdoq-level={level}").apply_opts(HevcParams(64, 64))
    assert p.rdoq_level == level and p.rdoq_lambda == 0.5


@pytest.mark.parametrize("opt", ["rdoq-level=3", "rdoq-level=-1", "psy-rdoq=1", "psy-rdoq=0"])
def test_x265_option_refused(opt):
    with pytest.raises(ffargs.FfArgsError):
        ffargs.parse(f"-vcodec libx265 -x265-params {opt}").apply_opts(HevcParams(64, 64))


def test_h264_table_has_no_rdoq():
    from govideocompressor_amd.models.h264_gpu import H264Params
    with pytest.raises(ffargs.FfArgsError):
        ffargs.parse("-vcodec libx264 -x264-params rdoq-level=2").apply_opts(H264Params(64, 64))
    assert knobs.encoder_overrides(H264Params, {"MIVC_HEVC_RDOQ": "2"}) == {}


def test_knobs():
    env = {"MIVC_HEVC_RDOQ": "2", "MIVC_HEVC_RDOQ_LAMBDA": "0.75"}
    over = knobs.encoder_overrides(HevcParams, env)
    assert over == {"rdoq_level": 2, "rdoq_lambda": 0.75}
    assert type(over["rdoq_level"]) is int and type(over["rdoq_lambda"]) is float
    p = dataclasses.replace(HevcParams(64, 64), **over)
    assert (p.rdoq_level, p.rdoq_lambda) == (2, 0.75)
    assert knobs.set_knobs(env)["unknown"] == {}


@pytest.mark.parametrize("name", presets.NAMES)
def test_no_preset_turns_it_on(name):
    p = presets.apply(HevcParams(64, 64), name)
    assert p.rdoq_level == 0 and p.rdoq_lambda == 0.5


@pytest.mark.parametrize("kw", [dict(rdoq_level=3), dict(rdoq_level=-1), dict(rdoq_level=True), dict(rdoq_lambda=0.0),
                                dict(rdoq_lambda=4.5)])
def test_encoder_refuses_values_out_of_range(kw):
    """refused where the encoder is constructed, before it touches a device"""
    from govideocompressor_amd.models.hevc_gpu import GpuHevcEncoder
    with pytest.raises(ValueError, match="rdoq"):
        GpuHevcEncoder(HevcParams(64, 64, **kw), slots=1)
