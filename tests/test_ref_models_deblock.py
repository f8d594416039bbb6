"""tests/ref_models_deblock.py against the C++ decoder (csrc/host/h264_decoder.cc), on the CPU.

* The model's boundary strengths, derived from the parser's records, equal the parser's ``bs`` (the
  array the GPU decoder's filter is given).  Streams: the CPU encoder's (I and P, CAVLC and CABAC,
  with and without the 8x8 transform enabled) and, since that encoder picks no 8x8-transform MB
  at these sizes, streams written from random records (utils/h264_synth.random_stream: I8x8 and
  8x8-transformed inter MBs, 16x8 / 8x16 / 8x8 partitions, two references with CABAC, per-MB QPs).
* On all-IDR streams the model's filter, applied to the decoder's unfiltered pictures with the
  parser's strengths and QPs, gives the decoder's filtered pictures sample for sample.
"""
import numpy as np
import pytest

import ref_models_deblock as M
from govideocompressor_amd.utils import yuv
from govideocompressor_amd.utils.h264_synth import random_stream

SIZES = [(64, 48), (176, 144)]
CODERS = [dict(cabac=0, t8x8=0), dict(cabac=1, t8x8=0), dict(cabac=0, t8x8=1), dict(cabac=1, t8x8=1)]


def _cpu_stream(host, w, h, frames, **kw):
    c = yuv.synth_clip_cpu(frames, w, h, seed=w + kw.get("qp", 0))
    return host.CpuEncoder(dict(width=w, height=h, **kw)).encode(c.i420(), c.frames, 0)


def _check_bs(host, es):
    seg = host.parse([es], 1)[0]
    assert seg["error"] is None
    wmb, hmb = seg["coded_width"] // 16, seg["coded_height"] // 16
    seen = np.zeros(5, np.int64)
    t8 = 0
    for p in range(seg["n"]):
        hdr = seg["hdr"][p]
        assert not (hdr[:, M._FLAGS] & 4).any(), "motion below 8x8: not what the records' layout holds"
        bs = M.boundary_strengths(hdr, M.nz_from_mask(hdr, seg["mask"][p]), wmb, hmb)
        np.testing.assert_array_equal(M.pack_bs(bs), seg["bs"][p], err_msg="picture %d" % p)
        np.testing.assert_array_equal(M.unpack_bs(M.pack_bs(bs)), bs)
        seen += np.bincount(bs.reshape(-1), minlength=5)
        t8 += int(M.hdr_t8(hdr).sum())
    return seen, t8


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("coder", CODERS, ids=lambda c: "cabac%d-t8x8%d" % (c["cabac"], c["t8x8"]))
def test_bs_equals_parser_cpu_encoder(host, w, h, coder):
    seen, _ = _check_bs(host, _cpu_stream(host, w, h, 5, qp=28, keyint=3, **coder))
    assert (seen[[0, 2, 3, 4]] > 0).all(), seen


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("cabac", [False, True])
def test_bs_equals_parser_random_records(host, w, h, cabac):
    es = random_stream(host, w, h, 4, seed=w + int(cabac), qp=30, cabac=cabac, t8x8=True, refs=2 if cabac else 1,
                       mv_range=6, density=0.05)
    seen, t8 = _check_bs(host, es)
    assert (seen > 0).all(), seen   # every bS value
    assert t8 > 0


def test_info_word():
    bs = np.zeros((3, 2, 4, 4), np.int32)
    bs[1, 0, 0, 3] = 4
    bs[1, 1, 2, 0] = 1
    bs[2] = 2
    info = M.info_words(bs, np.array([18, 42, 51]))
    assert info.tolist() == [18, 42 | (1 << 8) | (1 << 14), 51 | (255 << 8)]


@pytest.mark.parametrize("w,h,kw", [
    (64, 48, dict(qp=30)),
    (64, 48, dict(qp=22, chroma_qp_offset=4, cabac=1)),
    (176, 144, dict(qp=36, t8x8=1, cabac=1, chroma_qp_offset=-2)),
    (176, 144, dict(qp=27)),
], ids=lambda v: "-".join("%s%s" % kv for kv in v.items()) if isinstance(v, dict) else str(v))
def test_filter_equals_decoder_all_idr(host, w, h, kw):
    es = _cpu_stream(host, w, h, 2, keyint=1, **kw)
    _check_filter(host, es, 2)


@pytest.mark.parametrize("w,h", SIZES)
def test_filter_equals_decoder_random_idr(host, w, h):
    """I8x8 / I16x16 / I4x4 MBs with per-MB QPs: averaged QPs across edges, 8x8-transform MBs"""
    es = random_stream(host, w, h, 2, seed=7 + w, qp=32, keyint=1, cabac=True, t8x8=True, density=0.2)
    _check_filter(host, es, 2)


def test_synthetic_cases_cover():
    """The cases of tests/test_gpu_deblock_bs.py (same seeds) hold at least ten of everything that
    test lists."""
    tot = {}
    for i, (wmb, hmb) in enumerate(M.SHAPES):
        for k, n in M.run_case(M.make_case(wmb, hmb, 100 + i))["counts"].items():
            tot[k] = tot.get(k, 0) + n
    assert len(tot) == 21 and min(tot.values()) >= 10, tot


def _check_filter(host, es, n):
    seg = host.parse([es], 1)[0]
    raw, fin = host.decode(es, skip_deblock=True), host.decode(es)
    assert seg["n"] == n and len(raw) == n and len(fin) == n
    wmb, hmb = seg["coded_width"] // 16, seg["coded_height"] // 16
    for p in range(n):
        meta = seg["meta"][p]
        assert meta[3] == 1 and meta[9] == 1  # IDR, filtered
        planes = [raw[p][k].copy() for k in ("y_coded", "u_coded", "v_coded")]
        changed = M.deblock_picture(*planes, M.unpack_bs(seg["bs"][p]), M.hdr_qp(seg["hdr"][p]), wmb, hmb,
                                    chroma_qp_offset=int(meta[8]), alpha_off=int(meta[6]), beta_off=int(meta[7]))
        assert changed.any() and not np.array_equal(planes[0], raw[p]["y_coded"])
        for a, k in zip(planes, ("y_coded", "u_coded", "v_coded")):
            np.testing.assert_array_equal(a, fin[p][k], err_msg="picture %d %s" % (p, k))
