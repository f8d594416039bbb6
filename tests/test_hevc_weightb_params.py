"""HevcParams.weightb (x265 --weightb): the default, eff_weightb(), the host config, the
environment knob, the x265 options (weightb / no-weightb and the weightp pair the front lacked),
and that no preset turns the tool on."""
import dataclasses

import pytest

from govideocompressor_amd.jobs import ffargs
from govideocompressor_amd.models import knobs
from govideocompressor_amd.models.hevc_gpu import HevcParams
from govideocompressor_amd.rc import presets


def test_default_and_effective_value():
    p = HevcParams(64, 64)
    assert p.weightb is False and p.eff_weightb() is False and p.host_cfg()["weightb"] == 0
    on = HevcParams(64, 64, weightb=True)
    assert on.eff_weightb() is True and on.host_cfg()["weightb"] == 1
    assert HevcParams(64, 64, weightb=True, bframes=0).eff_weightb() is False
    assert HevcParams(64, 64, weightb=True, intra_only=True).eff_weightb() is False
    assert HevcParams(64, 64, weightb=True, keyint=4).eff_weightb() is False     # keyint GOPs are P-only
    # independent of weightp
    both_off = HevcParams(64, 64, weightb=True, weightp=False)
    assert both_off.eff_weightb() is True and both_off.host_cfg()["weightp"] == 0 and both_off.host_cfg()["weightb"] == 1
    assert HevcParams(64, 64, weightp=True).host_cfg()["weightb"] == 0


def test_knob():
    over = knobs.encoder_overrides(HevcParams, {"MIVC_HEVC_WEIGHTB": "1"})
    assert over == {"weightb": True}
    assert dataclasses.replace(HevcParams(64, 64), **over).eff_weightb() is True
    assert knobs.encoder_overrides(HevcParams, {"MIVC_HEVC_WEIGHTB": "0"}) == {"weightb": False}
    assert knobs.set_knobs({"MIVC_HEVC_WEIGHTB": "1"})["unknown"] == {}
    assert knobs.set_knobs({"MIVC_HEVC_WEIGHTB": "1"})["encoder"] == {"MIVC_HEVC_WEIGHTB": "1"}


@pytest.mark.parametrize("opt,field,want", [("weightb=1", "weightb", True), ("weightb=0", "weightb", False),
                                            ("no-weightb=1", "weightb", False), ("weightp=0", "weightp", False),
                                            ("weightp=1", "weightp", True), ("no-weightp=1", "weightp", False)])
def test_x265_options(opt, field, want):
    start = HevcParams(64, 64, weightb=not want) if field == "weightb" else HevcParams(64, 64, weightp=not want)
    p = ffargs.parse(f"-vcodec libx265 -x265-params {opt}").apply_opts(start)
    assert getattr(p, field) is want
    other = "weightp" if field == "weightb" else "weightb"
    assert getattr(p, other) == getattr(start, other)


def test_x265_options_combine():
    p = ffargs.parse("-vcodec libx265 -x265-params bframes=3:weightb=1:no-weightp=1").apply_opts(HevcParams(64, 64))
    assert (p.bframes, p.weightb, p.weightp) == (3, True, False) and p.eff_weightb()


@pytest.mark.parametrize("name", presets.NAMES)
def test_no_preset_turns_it_on(name):
    assert presets.apply(HevcParams(64, 64), name).weightb is False
