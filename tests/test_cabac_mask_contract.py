"""The reader contract of the block masks, on the shared host / device CABAC coder.

On the GPU the coder gets every MB's non-zero block mask from the kernels that produced the
levels (``encode_inter``'s ``mask_pre``), not from a pass over the levels.  Given the masks it must
never read a block whose bit is clear -- which is also what a record layout that leaves such
blocks unwritten would rest on.  Here the masks of random records are computed, every block the
contract calls unread is overwritten with a non-zero pattern, and the slice is coded through the
symbol path with the masks handed in (``_host.cabac_slice_data_masks``): the bytes must equal those
of the intact records.

Unread, per MB: a 4x4 luma block whose bit is clear; with the 8x8 transform a whole 8x8 block
whose four chunk bits are clear (the coder reads all 64 levels of a block with any bit set);
the luma DC unless its bit is set (never for a non-Intra16x16 MB); a chroma component's DC and
a chroma AC block whose bit is clear.
"""
import numpy as np
import pytest

from govideocompressor_amd.utils.h264_synth import random_stream

_KIND, _FLAGS = 0, 5
I4x4, I16x16, PSKIP, I8x8 = 0, 1, 3, 8
MBF_T8x8 = 2
POISON = 0x5A5A
W, H = 112, 80

# (seed, density): chosen so that the records hold every kind of MB asserted below
_SETS = {False: [(3, 0.15), (1, 0.005)], True: [(3, 0.15), (1, 0.005)]}


def _poisoned(hdr, coef, masks):
    """-> (poisoned copy, counts of the MB kinds the test relies on)"""
    out = coef.copy()
    n = dict(t8_zero_chunk=0, cdc_only=0, none=0, poisoned=0)
    for mb in range(hdr.shape[0]):
        m, c = int(masks[mb]), out[mb]
        kind = int(hdr[mb, _KIND])
        t8 = kind == I8x8 or (kind not in (I4x4, I16x16, I8x8, PSKIP) and hdr[mb, _FLAGS] & MBF_T8x8)
        if t8:
            for b8 in range(4):
                bits = (m >> (4 * b8)) & 15
                if bits == 0:
                    c[b8 * 64:(b8 + 1) * 64] = POISON
                    n["poisoned"] += 4
                elif bits != 15:
                    n["t8_zero_chunk"] += 1
        else:
            for b in range(16):
                if not (m >> b) & 1:
                    c[b * 16:(b + 1) * 16] = POISON
                    n["poisoned"] += 1
        if kind != I16x16 or not (m >> 16) & 1:
            c[256:272] = POISON
        for comp in range(2):
            if not (m >> (17 + comp)) & 1:
                c[272 + comp * 4:276 + comp * 4] = POISON
        for b in range(8):
            if not (m >> (19 + b)) & 1:
                c[280 + b * 16:296 + b * 16] = POISON
        if kind not in (I4x4, I16x16, I8x8, PSKIP):  # inter MBs with a record of their own
            n["none"] += m == 0
            n["cdc_only"] += m != 0 and (m & ~(3 << 17)) == 0
    return out, n


@pytest.mark.parametrize("t8", [False, True])
def test_coder_reads_only_blocks_in_the_mask(host, t8):
    total = dict(t8_zero_chunk=0, cdc_only=0, none=0, poisoned=0)
    for seed, density in _SETS[t8]:
        recs = []
        random_stream(host, W, H, 4, seed=seed, cabac=True, t8x8=t8, records=recs, density=density)
        cfg = dict(width=W, height=H, qp=28, cabac=1, t8x8=int(t8))
        for t, (hdr, coef) in enumerate(recs):
            fp = dict(idr=int(t == 0), qp=27 + t, frame_num=t)
            masks = host.cabac_block_masks(hdr, coef)
            assert masks.dtype == np.uint32 and masks.shape == (hdr.shape[0],)
            serial, symbols, _ = host.cabac_slice_data_two_ways(cfg, fp, hdr, coef)
            assert serial == symbols
            assert host.cabac_slice_data_masks(cfg, fp, hdr, coef, masks) == serial, "masks handed in change the bytes"
            bad, n = _poisoned(hdr, coef, masks)
            assert host.cabac_slice_data_masks(cfg, fp, hdr, bad, masks) == serial, "a block outside the mask was read"
            # the poison does reach the coder where the masks come from the levels
            assert host.cabac_slice_data_two_ways(cfg, fp, hdr, bad)[1] != serial
            for k in total:
                total[k] += int(n[k])
    assert total["poisoned"] > 0
    assert total["none"] > 0, "no MB without any level"
    assert total["cdc_only"] > 0, "no MB with chroma DC levels only"
    if t8:
        assert total["t8_zero_chunk"] > 0, "no 8x8 block with a level and an all-zero chunk"
