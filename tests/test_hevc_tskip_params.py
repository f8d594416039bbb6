"""HevcParams.tskip / tskip_lambda (x265 --tskip): defaults, the host configuration, the environment
knobs, the x265 option table, presets, the encoder's tag, the tool's variants and the screen
content generator."""
import dataclasses

import numpy as np
import pytest

from govideocompressor_amd.jobs import ffargs
from govideocompressor_amd.models import knobs
from govideocompressor_amd.models.h264_gpu import H264Params
from govideocompressor_amd.models.hevc_gpu import GpuHevcEncoder, HevcParams, rd_cbf_lamq_table
from govideocompressor_amd.rc import presets


def test_default_is_off():
    p = HevcParams(64, 64)
    assert p.tskip is False and p.tskip_lambda == 1.0
    assert p.host_cfg()["tskip"] == 0
    assert HevcParams(64, 64, tskip=True).host_cfg()["tskip"] == 1


def test_pps_flag_follows_the_config(host):
    a = host.hevc_parameter_sets(HevcParams(64, 64).host_cfg())
    b = host.hevc_parameter_sets(HevcParams(64, 64, tskip=True).host_cfg())
    assert a != b and len(a) == len(b)
    assert a == host.hevc_parameter_sets({k: v for k, v in HevcParams(64, 64).host_cfg().items() if k != "tskip"})


def test_knobs():
    env = {"MIVC_HEVC_TSKIP": "1", "MIVC_HEVC_TSKIP_LAMBDA": "0.5"}
    over = knobs.encoder_overrides(HevcParams, env)
    assert over == {"tskip": True, "tskip_lambda": 0.5}
    p = dataclasses.replace(HevcParams(640, 480), **over)
    assert p.tskip is True and p.tskip_lambda == 0.5
    assert knobs.encoder_overrides(HevcParams, {"MIVC_HEVC_TSKIP": "0"}) == {"tskip": False}
    assert knobs.encoder_overrides(H264Params, env) == {}
    s = knobs.set_knobs(env)
    assert s["unknown"] == {} and s["encoder"] == env
    with pytest.raises(SystemExit):
        knobs.check_environment(False, env)
    assert knobs.check_environment(True, env)["encoder"] == env


def test_x265_option():
    base = HevcParams(640, 480)
    assert ffargs.parse("-vcodec libx265 -x265-params tskip=1").apply_opts(base).tskip is True
    assert ffargs.parse("-vcodec libx265 -x265-params tskip").apply_opts(base).tskip is True
    on = HevcParams(640, 480, tskip=True)
    assert ffargs.parse("-vcodec libx265 -x265-params no-tskip=1").apply_opts(on).tskip is False
    assert ffargs.parse("-vcodec libx265 -x265-params tskip=0").apply_opts(on).tskip is False
    p = ffargs.parse("-vcodec libx265 -x265-params bframes=3:tskip=1:rdoq-level=2").apply_opts(base)
    assert (p.bframes, p.tskip, p.rdoq_level) == (3, True, 2)


@pytest.mark.parametrize("opt", ["tskip-fast=1", "tskip-fast", "tskip=2", "tskip=x", "tskip_lambda=2"])
def test_x265_option_refused(opt):
    with pytest.raises(ffargs.FfArgsError):
        ffargs.parse(f"-vcodec libx265 -x265-params {opt}").apply_opts(HevcParams(640, 480))


def test_x264_has_no_such_option():
    with pytest.raises(ffargs.FfArgsError):
        ffargs.parse("-vcodec libx264 -x264-params tskip=1").apply_opts(H264Params(640, 480))


@pytest.mark.parametrize("bad", [0.0, -1.0, 4.5])
def test_constructor_refuses_the_lambda_before_touching_the_device(bad):
    with pytest.raises(ValueError, match="tskip_lambda"):
        GpuHevcEncoder(HevcParams(64, 64, tskip=True, tskip_lambda=bad), slots=1, device="cpu")
    with pytest.raises(ValueError, match="tskip"):
        GpuHevcEncoder(HevcParams(64, 64, tskip=2), slots=1, device="cpu")


def test_lambda_table_is_the_rd_cbf_one():
    import ref_models_hevc_rdcbf as rc
    for lam, bd in ((1.0, 8), (0.5, 10), (2.0, 8)):
        assert rd_cbf_lamq_table(lam, bd) == rc.lamq_table(lam, bd)


@pytest.mark.parametrize("name", presets.NAMES)
def test_no_preset_sets_it(name):
    assert presets.apply(HevcParams(640, 480), name).tskip is False
    assert presets.apply(HevcParams(640, 480, tskip=True), name).tskip is True


def test_tag():
    assert "tskip" not in HevcParams(640, 480).describe()
    assert HevcParams(640, 480, tskip=True).describe().endswith(" tskip")
    assert HevcParams(640, 480, slices=2, tskip=True).describe().endswith(" slices2 tskip")


def test_content_rd_variant_and_kind():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "content_rd.py")
    spec = importlib.util.spec_from_file_location("content_rd_for_tskip", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.HEVC_CONFIGS["tskip"] == dict(tskip=True)
    for over in mod.HEVC_CONFIGS.values():
        HevcParams(640, 480, **over)
    from govideocompressor_amd.models.h264_gpu import CONTENT_KINDS
    assert "screen" not in CONTENT_KINDS and len(CONTENT_KINDS) == 7


def test_screen_generator():
    from govideocompressor_amd.utils.screen_synth import screen_clip
    y, u, v = screen_clip(3, 4, 96, 64, seed=5, device="cpu", plain_slots=(2,))
    assert y.shape == (3, 4, 64, 96) and u.shape == v.shape == (3, 4, 32, 48) and y.dtype.is_floating_point is False
    y2, u2, v2 = screen_clip(3, 4, 96, 64, seed=5, device="cpu", plain_slots=(2,))
    assert all((a == b).all() for a, b in ((y, y2), (u, u2), (v, v2)))          # seeded
    assert not (screen_clip(1, 1, 96, 64, seed=6, device="cpu")[0] == y[:1, :1]).all()
    yn = y.numpy().astype(np.int64)
    # scrolling by whole samples: frame t + 1 is frame t moved up by an even number of rows (and
    # columns) -- all of it in the plain slot, all but the overlays' marks in the others
    for b in range(3):
        same = max(float((yn[b, 1, :-dy, :96 - dx] == yn[b, 0, dy:, dx:]).mean()) for dy in (2, 4, 6) for dx in (0, 2))
        assert same == 1.0 if b == 2 else same > 0.85, (b, same)
    # marks: steps of 60 levels or more between horizontal neighbours, none in a plain slot
    step = np.abs(np.diff(yn[:, 0], axis=2))
    assert (step[0] >= 60).sum() > 50 and (step[1] >= 60).sum() > 50
    assert (step[2] >= 60).sum() <= 64 * 2                                         # panel edges only
    # a slot's content does not depend on its neighbours or on the other slots' make
    ya, _, _ = screen_clip(3, 4, 96, 64, seed=5, device="cpu")
    assert (ya[:2] == y[:2]).all()
    # 10 bits: the same picture, four times the scale, within rounding
    y10, u10, _ = screen_clip(3, 4, 96, 64, seed=5, device="cpu", bit_depth=10, plain_slots=(2,))
    assert y10.dtype.itemsize == 2 and int(y10.max()) <= 1023 and int(y10.max()) > 255
    assert np.abs(y10.numpy().astype(np.int64) - 4 * yn).max() <= 2
    with pytest.raises(ValueError):
        screen_clip(1, 1, 96, 64, device="cpu", bit_depth=9)


def test_entropy_context_size_comes_from_the_library(host):
    """the GPU coder's saved contexts: the size per substream is the library's (153 contexts of two
    bytes since transform_skip_flag has its own two), and the binding refuses a smaller buffer
    before anything is launched"""
    from govideocompressor_amd.ops import native
    hip = native.hip()
    assert hip.hevc_entropy_ctx_bytes() == 153 * 2
    cfg = HevcParams(64, 128, wpp=True, ctu64=False).host_cfg()
    pic = host.hevc_coder_pic(cfg, dict(idr=1, poc=0, qp=30, slice_type=2))
    need = 2 * 4 * hip.hevc_entropy_ctx_bytes()          # 2 pictures x 4 CTU rows
    fake = 64                                             # never dereferenced: the check comes first
    args = dict(pic=pic, B=2, qp=fake, ctu=fake, cu=fake, col=0, nzmap=fake, cy=fake, cb=fake, cr=fake, state=fake,
                state_bytes=0, out=fake, cap=16, sizes=fake, errs=fake, offs=fake, offs_host=fake, dst=fake, dst_cap=0,
                overflow=fake, stream=0, gprog=fake, gctx=fake)
    with pytest.raises(ValueError, match="gctx"):
        hip.hevc_entropy(**args, gctx_bytes=need - 1)
    with pytest.raises(ValueError, match="gctx"):
        hip.hevc_entropy(**args)
    with pytest.raises(ValueError, match="CoderPic"):
        hip.hevc_entropy(**dict(args, pic=pic[:-4]), gctx_bytes=need)
