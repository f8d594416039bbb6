"""Auto-variance AQ (aq_mode 2 / 3) without a GPU: the float64 model (tests/ref_models_aq_auto.py)
on cases computed by hand, the ``aq_mode`` field of both parameter classes, its two environment
knobs and the x265 spellings of the argument front."""
import numpy as np
import pytest

import ref_models as rm
import ref_models_aq_auto as am


def test_a_squared_14_is_the_neutral_picture():
    """e = 38415: e + 1 = 14^4, so a^2 = 14, m2 = 14, avg = m and every offset is 0 in mode 2."""
    e = np.full((2, 12), 38415)
    assert np.allclose(am.aq_auto_terms(e) ** 2, 14.0, rtol=0, atol=1e-12)
    assert np.abs(am.aq_auto_adj(e, 2, 1.0)).max() < 1e-12
    # mode 3 adds s (1 - 14 / 14) = 0 as well
    assert np.abs(am.aq_auto_adj(e, 3, 0.7)).max() < 1e-12


@pytest.mark.parametrize("s", [1.0, 0.5, 1.7])
def test_flat_picture(s):
    """e = 0: a = 1, m = m2 = 1, avg = 1 - 0.5 (1 - 14) = 7.5 -> s (1 - 7.5) = -6.5 s; mode 3 adds
    s (1 - 14) = -13 s."""
    e = np.zeros((1, 9), dtype=np.int64)
    assert np.allclose(am.aq_auto_adj(e, 2, s), -6.5 * s, rtol=0, atol=1e-12)
    assert np.allclose(am.aq_auto_adj(e, 3, s), -19.5 * s, rtol=0, atol=1e-12)
    assert am.offset_h264(am.aq_auto_adj(e, 3, 1.7)).tolist() == [[-24] * 9]  # -33.15 meets the clamp


@pytest.mark.parametrize("e0", [0, 255, 38415, 65535, 6242400])
def test_uniform_picture_in_general(e0):
    """All blocks alike: m = a, m2 = a^2, avg = a - 0.5 (a^2 - 14) / a -> 0.5 s (a^2 - 14)."""
    a2 = (e0 + 1.0) ** 0.25
    e = np.full((3, 7), e0)
    assert np.allclose(am.aq_auto_adj(e, 2, 0.8), 0.5 * 0.8 * (a2 - 14.0), rtol=0, atol=1e-10)
    assert np.allclose(am.aq_auto_adj(e, 3, 0.8), 0.5 * 0.8 * (a2 - 14.0) + 0.8 * (1.0 - 14.0 / a2), rtol=0, atol=1e-10)


def test_two_valued_picture():
    """Half the blocks e = 0 (a = 1), half e = 65535 (a = 65536^(1/8) = 4): m = 2.5, m2 = 8.5,
    avg = 2.5 - 0.5 (8.5 - 14) / 2.5 = 3.6 -> 2.5 (1 - 3.6) = -6.5 and 2.5 (4 - 3.6) = 1.0;
    mode 3 adds 1 - 14 = -13 and 1 - 14 / 16 = 0.125.  The statistics are per picture: a second
    picture of a = 4 blocks only gets 0.5 (16 - 14) = 1."""
    e = np.array([[0, 65535, 65535, 0], [65535] * 4])
    assert np.allclose(am.aq_auto_adj(e, 2, 1.0), [[-6.5, 1.0, 1.0, -6.5], [1.0] * 4], rtol=0, atol=1e-12)
    assert np.allclose(am.aq_auto_adj(e, 3, 1.0), [[-19.5, 1.125, 1.125, -19.5], [1.125] * 4], rtol=0, atol=1e-12)
    assert np.allclose(am.aq_auto_adj(e, 2, 2.0), [[-13.0, 2.0, 2.0, -13.0], [2.0] * 4], rtol=0, atol=1e-12)
    extra = np.array([[0.25, 0.0, -1.0, 30.0], [0.0] * 4])
    adj = am.aq_auto_adj(e, 2, 1.0, extra)
    assert np.allclose(adj[0], [-6.25, 1.0, 0.0, 23.5], rtol=0, atol=1e-12)
    assert am.offset_h264(adj)[0].tolist() == [-6, 1, 0, 24]   # rint: half to even, then the clamp
    # CTB form: mean of the four, +-12, 0 .. 51
    assert np.allclose(am.ctb_mean(adj[0]), 4.5625)
    assert am.ctb_qp_hevc(am.ctb_mean(adj[0]), [4, 50]).tolist() == [9, 51]
    assert am.ctb_qp_hevc(np.array([-40.0, 12.5, 13.5]), 30).tolist() == [18, 42, 42]


def test_bit_depth_correction():
    """Planes that are 4x an 8-bit picture have 16x its energy at bd = 10: the same a_i."""
    rng = np.random.default_rng(3)
    y = rng.integers(0, 256, (2, 32, 48))
    u, v = rng.integers(0, 256, (2, 2, 16, 24))
    e8 = rm.aq_energy(*rm.mb_blocks(y, u, v))
    e10 = rm.aq_energy(*rm.mb_blocks(4 * y, 4 * u, 4 * v))
    # (each of the three shifts drops less than one at the 8-bit scale, 16 at this one)
    assert np.abs(e10 - 16 * e8).max() < 48
    assert np.allclose(am.aq_auto_terms(e10, 10), am.aq_auto_terms(e8, 8), rtol=1e-6, atol=0)
    assert np.array_equal(am.aq_auto_terms(16 * e8, 10), am.aq_auto_terms(e8, 8))
    assert np.allclose(am.aq_auto_adj(16 * e8, 3, 1.0, bd=10), am.aq_auto_adj(e8, 3, 1.0), rtol=0, atol=1e-12)


def test_model_rejects_other_modes():
    with pytest.raises(ValueError):
        am.aq_auto_adj(np.zeros((1, 4)), 1, 1.0)


# ------------------------------------------------------------------ parameters and knobs
def test_aq_mode_defaults_and_validation():
    from govideocompressor_amd.models.h264_gpu import GpuH264Encoder, H264Params
    from govideocompressor_amd.models.hevc_gpu import GpuHevcEncoder, HevcParams

    assert H264Params(64, 64).aq_mode == 1 and HevcParams(64, 64).aq_mode == 1
    for bad in (-1, 4, 7, True, 2.5, "2"):
        with pytest.raises(ValueError, match="aq_mode"):
            GpuH264Encoder(H264Params(64, 64, aq_mode=bad), slots=1)
        with pytest.raises(ValueError, match="aq_mode"):
            GpuHevcEncoder(HevcParams(64, 64, aq_mode=bad), slots=1)


def test_hevc_aq_mode_0_is_strength_0():
    from govideocompressor_amd.models.hevc_gpu import HevcParams

    off = HevcParams(64, 64, aq_mode=0, cutree=False)
    assert off.eff_aq_strength() == 0.0 and not off.adaptive_qp() and off.host_cfg()["cu_qp_delta"] == 0
    assert HevcParams(64, 64, aq_strength=0.0, cutree=False).host_cfg()["cu_qp_delta"] == 0
    # cutree alone still needs per-CTB QPs, whatever the mode
    assert HevcParams(64, 64, aq_mode=0).adaptive_qp() and HevcParams(64, 64, aq_mode=0).host_cfg()["cu_qp_delta"] == 1
    for m in (1, 2, 3):
        p = HevcParams(64, 64, aq_mode=m, cutree=False)
        assert p.eff_aq_strength() == 1.0 and p.adaptive_qp() and p.host_cfg()["cu_qp_delta"] == 1


def test_knobs_map_and_parse():
    from govideocompressor_amd.models import knobs
    from govideocompressor_amd.models.h264_gpu import H264Params
    from govideocompressor_amd.models.hevc_gpu import HevcParams

    assert knobs.H264["MIVC_AQ_MODE"] == "aq_mode" and knobs.HEVC["MIVC_HEVC_AQ_MODE"] == "aq_mode"
    env = {"MIVC_AQ_MODE": "2", "MIVC_HEVC_AQ_MODE": "3"}
    assert knobs.encoder_overrides(H264Params, env) == {"aq_mode": 2}
    assert knobs.encoder_overrides(HevcParams, env) == {"aq_mode": 3}
    assert knobs.set_knobs(env)["encoder"] == env and not knobs.set_knobs(env)["unknown"]
    with pytest.raises(SystemExit):
        knobs.check_environment(False, env)
    assert knobs.check_environment(True, env)["encoder"] == env
    with pytest.raises(ValueError):
        knobs.encoder_overrides(H264Params, {"MIVC_AQ_MODE": "auto"})


# ------------------------------------------------------------------ argument front
def test_x265_aq_mode_and_tune_ssim():
    from govideocompressor_amd.jobs import ffargs
    from govideocompressor_amd.models.hevc_gpu import HevcParams

    for m in (2, 3):
        c = ffargs.parse(f"-vcodec libx265 -x265-params aq-mode={m}")
        assert c.opts == {"aq_mode": m}
        p = c.apply_opts(HevcParams(64, 64))
        assert (p.aq_mode, p.aq_strength) == (m, 1.0)
    c = ffargs.parse("-vcodec libx265 -x265-params aq-mode=3:aq-strength=0.6")
    assert c.apply_opts(HevcParams(64, 64)).aq_mode == 3 and c.apply_opts(HevcParams(64, 64)).aq_strength == 0.6
    c = ffargs.parse("-vcodec libx265 -tune ssim")
    assert c.tune == "ssim" and c.opts == {"aq_mode": 2}
    assert c.apply_opts(HevcParams(64, 64)).aq_mode == 2
    # an explicit mode after the tune wins; mode 0 stays "strength 0", as before
    assert ffargs.parse("-vcodec libx265 -tune ssim -x265-params aq-mode=1").apply_opts(HevcParams(64, 64)).aq_mode == 1
    assert ffargs.parse("-vcodec libx265 -x265-params aq-mode=0").opts == {"aq_strength": 0.0}
    p = ffargs.parse("-vcodec libx265 -x265-params aq-mode=0").apply_opts(HevcParams(64, 64))
    assert (p.aq_mode, p.aq_strength) == (1, 0.0)


def test_x265_aq_mode_4_names_what_is_implemented():
    from govideocompressor_amd.jobs import ffargs

    with pytest.raises(ffargs.FfArgsError) as ei:
        ffargs.parse("-vcodec libx265 -x265-params aq-mode=4")
    msg = str(ei.value)
    assert "aq-mode 4" in msg and all(f"{m} (" in msg for m in (0, 1, 2, 3))
    with pytest.raises(ffargs.FfArgsError):
        ffargs.parse("-vcodec libx265 -x265-params aq-mode=-1")
