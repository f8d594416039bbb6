"""The parser's bit-depth side info for the batched GPU decoder (CPU): ``bit_depth`` and the
per-picture ``gpu_ok16`` -- ``gpu_ok`` but for the bit depth, true for 8-, 9- and 10-bit
pictures (BitDepthY == BitDepthC) the reconstruction kernels cover -- in the dicts of both
``host.parse`` and ``parse_batch(...).info``.  ``meta`` keeps its 12 columns and column 10
(``gpu_ok``) its meaning: 1 only for 8-bit pictures.
"""
import numpy as np
import pytest

from govideocompressor_amd.utils.h264_synth import random_stream

_GPU_OK = 10  # column of meta


@pytest.mark.parametrize("bd,ok16,ok8", [(8, 1, 1), (9, 1, 0), (10, 1, 0), (12, 0, 0)])
def test_high10_flags(host, bd, ok16, ok8):
    frames = 4
    kw = dict(bit_depth=bd) if bd > 8 else {}
    streams = [random_stream(host, 96, 64, frames, seed=40 + bd, intra_in_p=0.3, t8x8=True, cabac=True, **kw),
               random_stream(host, 64, 48, frames, seed=60 + bd, pcm=0.2, qp=4, **kw)]
    batch = host.parse_batch(streams, 2)
    for i, s in enumerate(streams):
        for d in (host.parse([s])[0], batch.info(i)):
            assert not d["error"]
            assert d["bit_depth"] == bd
            ok = np.asarray(d["gpu_ok16"])
            assert ok.dtype == np.uint8 and ok.shape == (frames,)
            assert np.all(ok == ok16)
            meta = np.asarray(d["meta"])
            assert meta.shape == (frames, 12)
            assert np.all(meta[:, _GPU_OK] == ok8)


def test_high10_flags_other_reasons_clear_both(host):
    """A reason other than the depth clears both flags: pictures of more than 255 slices."""
    for bd in (8, 10):
        s = random_stream(host, 16, 16 * 260, 2, seed=7, slice_rows=1, bit_depth=bd)
        d = host.parse([s])[0]
        assert not d["error"] and d["bit_depth"] == bd
        assert np.all(np.asarray(d["gpu_ok16"]) == 0)
        assert np.all(np.asarray(d["meta"])[:, _GPU_OK] == 0)
