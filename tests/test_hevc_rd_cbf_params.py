"""HevcParams.rd_cbf / rd_cbf_lambda (the rate-distortion check of inter residuals against none):
defaults, ranges, the environment knobs and their coercion, the encoder's lambda table against the
model's, and that no preset and no x265 option turns the tool on."""
import dataclasses

import pytest

import ref_models_hevc_rdcbf as rc
from govideocompressor_amd.jobs import ffargs
from govideocompressor_amd.models import knobs
from govideocompressor_amd.models.hevc_gpu import HevcParams, rd_cbf_lamq_table
from govideocompressor_amd.rc import presets


def test_defaults():
    p = HevcParams(64, 64)
    assert p.rd_cbf is False
    assert p.rd_cbf_lambda == 1.0 and type(p.rd_cbf_lambda) is float
    assert "rd_cbf" not in p.host_cfg() and "rd_cbf_lambda" not in p.host_cfg()  # no syntax of its own


def test_knobs_and_coercion():
    env = {"MIVC_HEVC_RD_CBF": "1", "MIVC_HEVC_RD_CBF_LAMBDA": "2"}
    over = knobs.encoder_overrides(HevcParams, env)
    assert over == {"rd_cbf": True, "rd_cbf_lambda": 2.0}
    assert type(over["rd_cbf"]) is bool and type(over["rd_cbf_lambda"]) is float
    p = dataclasses.replace(HevcParams(64, 64), **over)
    assert (p.rd_cbf, p.rd_cbf_lambda) == (True, 2.0)
    for off in ("0", "false", "off", "no", ""):
        assert knobs.encoder_overrides(HevcParams, {"MIVC_HEVC_RD_CBF": off}) == {"rd_cbf": False}
    assert knobs.encoder_overrides(HevcParams, {"MIVC_HEVC_RD_CBF_LAMBDA": "0.75"}) == {"rd_cbf_lambda": 0.75}
    s = knobs.set_knobs(env)
    assert s["unknown"] == {} and s["encoder"] == env
    with pytest.raises(SystemExit):
        knobs.check_environment(False, env)
    assert knobs.check_environment(True, env)["encoder"] == env


def test_h264_has_no_such_knob():
    from govideocompressor_amd.models.h264_gpu import H264Params
    assert knobs.encoder_overrides(H264Params, {"MIVC_HEVC_RD_CBF": "1", "MIVC_HEVC_RD_CBF_LAMBDA": "2"}) == {}
    assert not any(f.name.startswith("rd_cbf") for f in dataclasses.fields(H264Params))


@pytest.mark.parametrize("opt", ["rd-cbf=1", "rd_cbf=1", "rd-cbf-lambda=2", "rdcbf=1"])
def test_no_x265_spelling(opt):
    with pytest.raises(ffargs.FfArgsError):
        ffargs.parse(f"-vcodec libx265 -x265-params {opt}").apply_opts(HevcParams(64, 64))


@pytest.mark.parametrize("name", presets.NAMES)
def test_no_preset_turns_it_on(name):
    p = presets.apply(HevcParams(64, 64), name)
    assert p.rd_cbf is False and p.rd_cbf_lambda == 1.0


@pytest.mark.parametrize("lam", [0.0, -1.0, 4.5, float("nan")])
@pytest.mark.parametrize("on", [False, True])
def test_encoder_refuses_lambda_out_of_range(lam, on):
    """refused where the encoder is constructed, before it touches a device, knob on or off"""
    from govideocompressor_amd.models.hevc_gpu import GpuHevcEncoder
    with pytest.raises(ValueError, match="rd_cbf_lambda"):
        GpuHevcEncoder(HevcParams(64, 64, rd_cbf=on, rd_cbf_lambda=lam), slots=1)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("lam", [0.25, 0.5, 1.0, 1.5, 2.0, 4.0, 4])
def test_encoder_table_is_the_models(lam, bd):
    t = rd_cbf_lamq_table(lam, bd)
    assert t == rc.lamq_table(lam, bd) and len(t) == 52
    assert all(type(v) is int and 0 <= v <= (1 << 23) for v in t)  # the probe's and an int32's range
    assert all(a <= b for a, b in zip(t, t[1:]))
