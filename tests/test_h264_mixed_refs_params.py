"""H264Params.mixed_refs (x264 --mixed-refs): the knob, where it takes effect, its environment
variable, its two -x264-params spellings, and that no preset turns it on yet."""
import dataclasses

import pytest

from govideocompressor_amd.jobs import ffargs
from govideocompressor_amd.models import knobs
from govideocompressor_amd.models.h264_gpu import H264Params
from govideocompressor_amd.models.hevc_gpu import HevcParams
from govideocompressor_amd.rc import presets


def test_default_is_off():
    p = H264Params(640, 480)
    assert p.mixed_refs is False and p.eff_mixed_refs() is False
    assert H264Params(640, 480, mixed_refs=True).eff_mixed_refs() is True


@pytest.mark.parametrize("over", [dict(refs=1), dict(cabac=False), dict(partitions=False)],
                         ids=["refs1", "cavlc", "no-partitions"])
def test_needs_several_references_and_the_partitions(over):
    p = H264Params(640, 480, mixed_refs=True, **over)
    assert p.mixed_refs is True and p.eff_mixed_refs() is False
    assert "mixed-refs" not in p.profile_name()


@pytest.mark.parametrize("refs", [2, 3, 4])
def test_any_list_of_two_or_more(refs):
    assert H264Params(640, 480, mixed_refs=True, refs=refs).eff_mixed_refs() is True


def test_host_cfg_is_unchanged():
    """the stream's parameter sets say nothing about it: num_ref_frames comes from refs"""
    assert H264Params(640, 480, mixed_refs=True).host_cfg() == H264Params(640, 480).host_cfg()


def test_tag():
    assert "mixed-refs" not in H264Params(640, 480).profile_name()
    name = H264Params(640, 480, mixed_refs=True).profile_name()
    assert " ref3 mixed-refs" in name and name.count("mixed-refs") == 1


def test_knob():
    env = {"MIVC_MIXED_REFS": "1"}
    assert knobs.encoder_overrides(H264Params, env) == {"mixed_refs": True}
    assert knobs.encoder_overrides(H264Params, {"MIVC_MIXED_REFS": "0"}) == {"mixed_refs": False}
    assert knobs.encoder_overrides(HevcParams, env) == {}
    p = dataclasses.replace(H264Params(640, 480), **knobs.encoder_overrides(H264Params, env))
    assert p.eff_mixed_refs() is True
    s = knobs.set_knobs(env)
    assert s["unknown"] == {} and s["encoder"] == env
    with pytest.raises(SystemExit):
        knobs.check_environment(False, env)
    assert knobs.check_environment(True, env)["encoder"] == env


def test_x264_option():
    base, on = H264Params(640, 480), H264Params(640, 480, mixed_refs=True)
    assert ffargs.parse("-vcodec libx264 -x264-params mixed-refs=1").apply_opts(base).mixed_refs is True
    assert ffargs.parse("-vcodec libx264 -x264-params mixed-refs").apply_opts(base).mixed_refs is True
    assert ffargs.parse("-vcodec libx264 -x264-params mixed-refs=0").apply_opts(on).mixed_refs is False
    assert ffargs.parse("-vcodec libx264 -x264-params no-mixed-refs").apply_opts(on).mixed_refs is False
    assert ffargs.parse("-vcodec libx264 -x264-params no-mixed-refs=1").apply_opts(on).mixed_refs is False
    p = ffargs.parse("-vcodec libx264 -x264-params ref=4:mixed-refs=1:bframes=2").apply_opts(base)
    assert (p.refs, p.mixed_refs, p.bframes) == (4, True, 2)
    assert ffargs.parse("-vcodec libx264").apply_opts(base).mixed_refs is False


@pytest.mark.parametrize("opt", ["mixed-refs=2", "mixed-refs=x", "mixed_refs=1", "mixedrefs=1"])
def test_x264_option_refused(opt):
    with pytest.raises(ffargs.FfArgsError):
        ffargs.parse(f"-vcodec libx264 -x264-params {opt}").apply_opts(H264Params(640, 480))


def test_x265_has_no_such_option():
    with pytest.raises(ffargs.FfArgsError):
        ffargs.parse("-vcodec libx265 -x265-params mixed-refs=1").apply_opts(HevcParams(640, 480))


@pytest.mark.parametrize("name", presets.NAMES)
def test_no_preset_sets_it(name):
    assert presets.apply(H264Params(640, 480), name).mixed_refs is False
    assert presets.apply(H264Params(640, 480, mixed_refs=True), name).mixed_refs is True


def test_content_rd_variant():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "content_rd.py")
    spec = importlib.util.spec_from_file_location("content_rd_for_mixed_refs", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.CONFIGS["mixedrefs"] == dict(mixed_refs=True)
    for over in mod.CONFIGS.values():
        H264Params(640, 480, **over)
