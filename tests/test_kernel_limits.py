"""The picture sizes behind the kernels' fixed LDS arrays (csrc/kernels/geom_limits.h): the library
names them, every binding whose kernel indexes such an array refuses a larger geometry before
anything else, and the Python callers route or refuse by the same numbers.

Every call of a binding in this file is one the binding must refuse: the pointers are dummies, so
a call that got through would launch a kernel on them."""
import numpy as np
import pytest

from govideocompressor_amd.models.h264_decode_gpu import _META, _gpu_plan
from govideocompressor_amd.models.h264_gpu import GpuH264Encoder, H264Params
from govideocompressor_amd.ops import native

F = 64  # a non-null "pointer", never dereferenced: the geometry check comes first


def _args(name, wmb, hmb):
    """positional arguments of binding `name` for a picture of wmb x hmb MBs"""
    return {
        "encode_intra": (1, wmb, hmb, F, F, F, F, F, F, F, 0, F, F, F, F, F, F, 0, 0),
        "decode_picture_dpb": (1, wmb, hmb, 1, F, F, F, F, F, F, F, F, F, F, F, F, 0, 0, F, F, 0),
        "decode_picture_dpb16": (1, wmb, hmb, 1, F, F, F, F, F, F, F, F, F, F, F, F, 0, 0, 10, F, F, 0),
        "deblock": (1, wmb, hmb, F, F, F, F, F, 0, 0, 0, F, 0, 0, 0, F, F),
        "deblock_dpb": (1, wmb, hmb, 1, F, F, F, F, F, F, F, 0, 0, 0, F, 0),
        "deblock_dpb16": (1, wmb, hmb, 1, F, F, F, F, F, F, 0, 0, 0, 10, F, 0),
        "b_spatial": (1, wmb, hmb, F, F, F, F, F, [F], [F], [32], F, F, 0, F, F, F, F, 0),
        "b_spatial_exact": (1, wmb, hmb, F, F, F, F, F, 0),
        # HEVC: coded size in samples; the rows are those of 32x32 CTBs
        "hevc_intra": (1, wmb * 32, hmb * 32, F, F, F, F, F, F, F, F, F, F, F, F, F, F, 8, 1, 1, F, 0),
    }[name]


ROWS = ["encode_intra", "decode_picture_dpb", "decode_picture_dpb16", "deblock", "deblock_dpb", "deblock_dpb16",
        "b_spatial", "hevc_intra"]
COLS = ["deblock", "deblock_dpb", "b_spatial", "b_spatial_exact"]


def test_the_library_names_its_limits():
    hip = native.hip()
    assert hip.max_mb_rows == 272 and hip.max_mb_cols == 480
    assert native.kernel_limits() == (272, 480)


@pytest.mark.parametrize("name", ROWS)
def test_binding_refuses_too_many_rows(name):
    hip = native.hip()
    with pytest.raises(ValueError, match=f"^{name}: .*rows"):
        getattr(hip, name)(*_args(name, 4, hip.max_mb_rows + 1))


@pytest.mark.parametrize("name", COLS)
def test_binding_refuses_too_many_columns(name):
    hip = native.hip()
    with pytest.raises(ValueError, match=f"^{name}: .*columns"):
        getattr(hip, name)(*_args(name, hip.max_mb_cols + 1, 4))


def _segment(width, height, bit_depth):
    return dict(n=1, bit_depth=bit_depth, coded_width=width, coded_height=height,
                meta=np.ones((1, len(_META)), np.int32), gpu_ok16=np.ones(1, np.uint8))


@pytest.mark.parametrize("bit_depth, high_depth", [(8, "cpu"), (10, "gpu")])
def test_gpu_plan_sends_oversize_segments_to_the_cpu_decoder(bit_depth, high_depth):
    assert _gpu_plan(_segment(7680, 4320, bit_depth), high_depth) == (True, "")
    ok, why = _gpu_plan(_segment(8192, 4320, bit_depth), high_depth)      # 512 MB columns
    assert not ok and "columns" in why
    ok, why = _gpu_plan(_segment(1920, 4368, bit_depth), high_depth)      # 273 MB rows
    assert not ok and "rows" in why


@pytest.mark.parametrize("width, height", [(8192, 4320), (1920, 4368)])
def test_encoder_refuses_the_geometry_before_it_allocates(width, height):
    with pytest.raises(ValueError, match="macroblocks"):
        GpuH264Encoder(H264Params(width, height), slots=1, device="cpu")
