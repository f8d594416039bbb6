#!/usr/bin/env python3
"""Record the golden bitstream hashes of tests/test_gpu_inter_layout.py (suite ``inter``),
tests/test_gpu_decide_layout.py (suite ``decide``), tests/test_gpu_gate_layout.py (suite ``gate``)
and tests/test_gpu_intra_free.py (suite ``intra``: planted intra MBs of P / B pictures, with the
counts of free and chained ones per case), tests/test_gpu_source_pass.py (suite ``source``: the
clips of the padding / AQ and mb_qp_delta flag tests through ``encode``) and
tests/test_gpu_inter_chroma8.py (suite ``chroma8``: the chroma launch of the inter residual, eight
MBs per wave; with the record statistics and the mb_qp_delta flag bytes per case) and the
end-to-end cases of tests/test_gpu_b_block_fetch.py (suite ``bfetch``: the B decision's pre-pass
and main pass; with the gate's counts and the direct MBs / quadrants of the decoded records) and
tests/test_gpu_inter_block_mask.py (suite ``mask``: the block masks the inter kernels hand to the
GPU CABAC path, which the parent's kernels do not write: its bytes, with the record statistics per
case) and tests/test_gpu_me_uniform_encode.py (suite ``me``: whole encodes through the 16x16 motion
search, whose wave-uniform work moved to the scalar unit: P only, B pictures with temporal direct,
three references with weighted P, b-pyramid, CAVLC, one HEVC encode) and
tests/test_gpu_deblock_encode.py (suite ``deblock``: whole encodes through the in-loop filter, with
the hash of the kept reconstruction per slot).

The tests pin the bytes of small encodes, at shapes where the four-MBs-per-wave lane layout can
go wrong, to what the *parent* build of the kernels emits.  So this recorder never runs on the
kernels under test: it needs MIVC_HIP_LIB to name a kernel library built from the parent
commit, e.g.

    python tools/build_variant.py parent --rev HEAD~1
    MIVC_HIP_LIB=abso/parent.so python tools/record_inter_layout.py tests/golden/inter_layout_parent.json
    MIVC_HIP_LIB=abso/parent.so python tools/record_inter_layout.py decide tests/golden/decide_layout_parent.json
    MIVC_HIP_LIB=abso/parent.so python tools/record_inter_layout.py gate tests/golden/gate_layout_parent.json
    MIVC_HIP_LIB=abso/parent.so python tools/record_inter_layout.py intra tests/golden/intra_free_parent.json
    MIVC_HIP_LIB=abso/parent.so python tools/record_inter_layout.py source tests/golden/source_pass_parent.json
    MIVC_HIP_LIB=abso/parent.so python tools/record_inter_layout.py chroma8 tests/golden/inter_chroma8_parent.json
    MIVC_HIP_LIB=abso/parent.so python tools/record_inter_layout.py bfetch tests/golden/b_block_fetch_parent.json
    MIVC_HIP_LIB=abso/parent.so python tools/record_inter_layout.py mask tests/golden/inter_block_mask_parent.json
    MIVC_HIP_LIB=abso/parent.so python tools/record_inter_layout.py me tests/golden/me_uniform_parent.json
    MIVC_HIP_LIB=abso/parent.so python tools/record_inter_layout.py deblock tests/golden/deblock_bs_parent.json

The file holds, per case, the arguments (size, frames, clip seed / class, parameter overrides)
and the SHA-256 of every slot's bitstream.  Per case it also prints what the test asserts
(``inter``: split partitions, waves of four MBs mixing intra and inter MBs, waves mixing MBs
with and without the 8x8 transform; ``decide``: merge / skip CUs and bi-predicted CUs of the HEVC
merge passes, B_Direct / B_Skip MBs of H.264 spatial direct; ``gate``: MBs the search gate stopped
and MBs it let through, in the B pictures' list searches and in the farther list-0 pictures'), so
a case that would pass vacuously shows here.  The ``gate`` suite stores those counts in the file.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLOTS = 2
_B3 = dict(bframes=3, weightb=True)
_P = dict(bframes=0)
_PART = dict(partitions=True, part_overhead=0, part_min_satd=0)
# size -> nmb % 4: 48x48 -> 9 MBs (one live MB in the last wave), 96x48 -> 18 (two), 80x48 -> 15
# (three, and 5 MBs per row: waves straddle MB rows), 176x144 -> 99 (baseline)
CASES = [
    dict(id="48x48-p-t8-trellis2", width=48, height=48, frames=5, seed=3, kind="default",
         params=dict(crf=None, qp=24, t8x8=True, trellis=2, aq_strength=0.0, **_P)),
    dict(id="48x48-b-not8-trellis0", width=48, height=48, frames=9, seed=4, kind="default",
         params=dict(crf=None, qp=26, t8x8=False, trellis=0, aq_strength=0.0, **_B3)),
    dict(id="96x48-b-t8-trellis2-aq", width=96, height=48, frames=7, seed=5, kind="default",
         params=dict(crf=None, qp=26, t8x8=True, trellis=2, aq_strength=1.0, **_B3)),
    dict(id="96x48-p-refs3-weightp", width=96, height=48, frames=6, seed=6, kind="fade",
         params=dict(crf=None, qp=26, t8x8=False, trellis=2, aq_strength=0.0, refs=3, weightp=True, **_P)),
    dict(id="80x48-b-t8-trellis0-part", width=80, height=48, frames=9, seed=7, kind="default",
         params=dict(crf=None, qp=24, t8x8=True, trellis=0, aq_strength=0.0, **_B3, **_PART)),
    dict(id="80x48-p-t8-trellis2-aq", width=80, height=48, frames=5, seed=8, kind="default",
         params=dict(crf=None, qp=28, t8x8=True, trellis=2, aq_strength=1.0, **_P)),
    dict(id="80x48-p-noise-lowqp", width=80, height=48, frames=6, seed=9, kind="noise",
         params=dict(crf=None, qp=18, t8x8=True, trellis=2, aq_strength=1.0, **_P)),
    dict(id="176x144-p-part", width=176, height=144, frames=9, seed=3, kind="default",
         params=dict(crf=None, qp=24, t8x8=True, trellis=2, **_P, **_PART)),
    dict(id="176x144-b-refs3-weightp-aq", width=176, height=144, frames=9, seed=10, kind="default",
         params=dict(crf=None, qp=26, t8x8=True, trellis=2, aq_strength=1.0, refs=3, weightp=True, **_B3)),
    dict(id="176x144-b-noise-lowqp", width=176, height=144, frames=9, seed=11, kind="noise",
         params=dict(crf=None, qp=16, t8x8=True, trellis=2, aq_strength=1.0, **_B3)),
]

# The decision kernels that no other golden reaches: the HEVC merge passes (hevc_b_init_p /
# hevc_b_merge, hevc_merge_refine, hevc_b_choose) and H.264 spatial direct (b_spatial_exact /
# b_spatial_fixup, b_spatial_decide).  HEVC sizes are padded to the CTB, so a wave is always
# full; what can go wrong is a wave straddling rows of 16x16 blocks (6 and 10 blocks per row)
# and the z-scan availability at CTU edges (32x32 CTBs and 64x64 CTUs).  merge_exact=False
# needs refs=1 (the neighbour-vector approximation carries no refIdx).
_HQ = dict(crf=None, qp=30)
_SP = dict(crf=None, qp=26, bframes=3, direct="spatial")
DECIDE_CASES = [
    dict(id="hevc-96x64-p-exact", codec="hevc", width=96, height=64, frames=6, seed=3, kind="default",
         params=dict(bframes=0, merge_exact=True, ctu64=False, **_HQ)),
    dict(id="hevc-96x64-p-refine", codec="hevc", width=96, height=64, frames=6, seed=4, kind="default",
         params=dict(bframes=0, merge_exact=False, refs=1, ctu64=False, **_HQ)),
    dict(id="hevc-96x64-b-tmvp", codec="hevc", width=96, height=64, frames=7, seed=5, kind="default",
         params=dict(bframes=1, tmvp=True, ctu64=False, **_HQ)),
    dict(id="hevc-160x96-b-tmvp", codec="hevc", width=160, height=96, frames=7, seed=6, kind="default",
         params=dict(bframes=1, tmvp=True, ctu64=False, **_HQ)),
    dict(id="hevc-160x96-p-refs3", codec="hevc", width=160, height=96, frames=8, seed=7, kind="default",
         params=dict(bframes=0, merge_exact=True, refs=3, ref_gate=0, ctu64=False, **_HQ)),
    dict(id="hevc-192x128-p-exact-ctu64", codec="hevc", width=192, height=128, frames=6, seed=8, kind="default",
         params=dict(bframes=0, merge_exact=True, ctu64=True, **_HQ)),
    dict(id="hevc-192x128-p-refine-ctu64", codec="hevc", width=192, height=128, frames=6, seed=9, kind="default",
         params=dict(bframes=0, merge_exact=False, refs=1, ctu64=True, **_HQ)),
    dict(id="hevc-192x128-b-tmvp-ctu64", codec="hevc", width=192, height=128, frames=7, seed=10, kind="default",
         params=dict(bframes=1, tmvp=True, ctu64=True, **_HQ)),
    dict(id="h264-80x48-spatial-fast", codec="h264", width=80, height=48, frames=9, seed=11, kind="default",
         params=dict(**_SP)),
    dict(id="h264-80x48-spatial-wavefront", codec="h264", width=80, height=48, frames=9, seed=12, kind="default",
         params=dict(spatial_wavefront=True, **_SP)),
    dict(id="h264-176x144-spatial-fast-pyramid", codec="h264", width=176, height=144, frames=9, seed=13,
         kind="default", params=dict(pyramid=True, **_SP)),
    dict(id="h264-176x144-spatial-wavefront", codec="h264", width=176, height=144, frames=9, seed=14,
         kind="default", params=dict(spatial_wavefront=True, **_SP)),
]

# Gated motion searches (me.hip: one wave per run of MBs): the B pictures' two list searches
# behind b_gate (temporal direct's cost; < 0: lambdas of the MB's QP, which AQ changes inside a
# run; 0: no gate) and the farther list-0 pictures' behind ref_gate (0: a gate nothing passes).
# 15 and 99 MBs per slot: one partial run, and runs that end inside the picture for every run
# length up to 64.
_G = dict(crf=None, bframes=3, weightb=False, aq_strength=0.0)
GATE_CASES = [
    dict(id="80x48-bgate2400", width=80, height=48, frames=9, seed=21, kind="default",
         params=dict(qp=24, b_gate=2400, refs=1, **_G)),
    dict(id="80x48-bgate-150-weightb-aq", width=80, height=48, frames=9, seed=22, kind="default",
         params=dict(crf=None, qp=24, bframes=3, weightb=True, aq_strength=1.0, b_gate=-150, refs=1)),
    dict(id="80x48-bgate0", width=80, height=48, frames=5, seed=23, kind="default",
         params=dict(qp=26, b_gate=0, refs=1, **_G)),
    dict(id="80x48-bgate2400-refs3-refgate3000", width=80, height=48, frames=9, seed=24, kind="default",
         params=dict(qp=24, b_gate=2400, refs=3, ref_gate=3000, **_G)),
    dict(id="176x144-bgate2400-refs3-refgate3000", width=176, height=144, frames=9, seed=25, kind="default",
         params=dict(qp=26, b_gate=2400, refs=3, ref_gate=3000, **_G)),
    dict(id="176x144-bgate-150-refs3-refgate0", width=176, height=144, frames=9, seed=26, kind="default",
         params=dict(qp=26, b_gate=-150, refs=3, ref_gate=0, **_G)),
    dict(id="176x144-bgate0-refs3-refgate3000", width=176, height=144, frames=7, seed=27, kind="default",
         params=dict(qp=24, b_gate=0, refs=3, ref_gate=3000, **_G)),
]
GATE_SENTINEL = -12345
NO_COST = 0x3FFFFFFF

# Intra MBs of P / B pictures (encode_intra.hip: free MBs a wave per run, chained MBs in the
# wavefront): see tests/test_gpu_intra_free.py, whose clip builders and classifier this suite
# runs.  spots: per slot, (mx, my) of the MBs planted in display frame plant_t; pics: display
# indices of the pictures whose intra MBs are counted (None: every picture with an inter MB);
# need: the classes the case is there for; free_spots / chained_spots: what single MBs must be.
_IP = dict(crf=None, qp=26, bframes=0)
_ISO = [[0, 3], [10, 2], [4, 0], [5, 8], [2, 5], [4, 5], [8, 4], [8, 6], [9, 8]]
_PAIRS = [[2, 1], [3, 1], [6, 1], [6, 2], [1, 4], [2, 5], [6, 5], [5, 6]]
_G33 = [[x, y] for y in (1, 2, 3) for x in (1, 2, 3)]
_LSHAPE = [[6, 4], [6, 5], [6, 6], [7, 6], [8, 6]]


def _spots(id_, w, h, spots, need, params=None, **kw):
    return dict(dict(id=id_, width=w, height=h, frames=2, seed=17, clip="spots", plant_t=1, spots=spots, pics=[1],
                     need=need, params=dict(_IP, **(params or {}))), **kw)


INTRA_CASES = [
    # every picture edge, two in a row two columns apart, two in a column two rows apart, one in
    # the last partial run (MB 96 of 99); only free MBs: the wavefront launch returns at once
    _spots("176x144-isolated", 176, 144, [_ISO, _ISO], ["free"], free_only=True, free_spots=[_ISO, _ISO]),
    # one chained MB through L, T, TL and TR alone
    _spots("176x144-pairs", 176, 144, [_PAIRS, _PAIRS], ["free", "chained"],
           free_spots=[[[2, 1], [6, 1], [1, 4], [6, 5]]] * 2, chained_spots=[[[3, 1], [6, 2], [2, 5], [5, 6]]] * 2),
    _spots("176x144-tr-pair-i4x4", 176, 144, [[[6, 5], [5, 6]]] * 2, ["free", "chained"], params=dict(i4x4_in_p=True),
           free_spots=[[[6, 5]]] * 2, chained_spots=[[[5, 6]]] * 2),
    _spots("176x144-groups", 176, 144, [_G33 + _LSHAPE] * 2, ["free", "chained"],
           free_spots=[[[1, 1], [6, 4]]] * 2, chained_spots=[[s for s in _G33 + _LSHAPE if s not in ([1, 1], [6, 4])]] * 2),
    # 5 MBs per row, 15 MBs: one partial run; slot 0 codes MB 1 then MB 8, slot 1 MB 1 then MB 12
    # (one column right of the previous one, two rows down)
    _spots("80x48-straddle", 80, 48, [[[1, 0], [3, 1]], [[1, 0], [2, 2]]], ["free"], free_only=True,
           free_spots=[[[1, 0], [3, 1]], [[1, 0], [2, 2]]]),
    # 11 MBs per row: MBs 37 and 50 (and 32 and 45, inside one run of 16); slot 1: MBs 37 and 60
    # (column + 1, two rows down) and MB 96 in the last partial run
    _spots("176x144-straddle", 176, 144, [[[4, 3], [6, 4], [10, 2], [1, 4]], [[4, 3], [5, 5], [8, 8]]], ["free"],
           free_only=True, free_spots=[[[4, 3], [6, 4], [10, 2], [1, 4]], [[4, 3], [5, 5], [8, 8]]]),
    # row runs and the edges of a wave's span: MBs 31 | 32 (a pair across the edge of a span of 16
    # or 32 MBs), MBs 65 and 66 (last of a row, first of the next: raster neighbours that are not
    # neighbours); slot 1: a run of four over MBs 47 | 48
    _spots("176x144-span-edge", 176, 144, [[[9, 2], [10, 2], [10, 5], [0, 6]], [[3, 4], [4, 4], [5, 4], [6, 4]]],
           ["free", "chained"], free_spots=[[[9, 2], [10, 5], [0, 6]], [[3, 4]]],
           chained_spots=[[[10, 2]], [[4, 4], [5, 4], [6, 4]]]),
    # slot 0 without an intra MB: both launches return for it
    _spots("176x144-empty-slot", 176, 144, [[], _G33 + _ISO[1:2] + [[8, 6], [9, 8], [7, 0]]], ["free", "chained"]),
    dict(id="176x144-scenecut", width=176, height=144, frames=30, seed=2, clip="cut", cut=27, pics=[27],
         need=["free", "chained"], params=dict()),
    _spots("176x144-b-planted", 176, 144, [[[2, 2], [8, 6], [5, 4], [6, 4]]] * 2, ["free", "chained"],
           params=dict(bframes=3, lookahead=False), frames=5, plant_t=2, pics=[2], b_picture=True,
           free_spots=[[[2, 2], [8, 6], [5, 4]]] * 2, chained_spots=[[[6, 4]]] * 2),
    # two slices of four MB rows: (5, 4) starts the second slice right under (5, 3)
    _spots("176x128-slices2", 176, 128, [[[5, 3], [5, 4], [8, 1], [9, 1]]] * 2, ["free", "chained"], params=dict(slices=2),
           free_spots=[[[5, 3], [5, 4], [8, 1]]] * 2, chained_spots=[[[9, 1]]] * 2),
    # the two noisy cases of the inter suite, with their counts
    dict(id="80x48-p-noise-lowqp", width=80, height=48, frames=6, seed=9, clip="synth", kind="noise", pics=None, need=[],
         params=dict(crf=None, qp=18, t8x8=True, trellis=2, aq_strength=1.0, **_P)),
    dict(id="176x144-b-noise-lowqp", width=176, height=144, frames=9, seed=11, clip="synth", kind="noise", pics=None,
         need=["free", "chained"], params=dict(crf=None, qp=16, t8x8=True, trellis=2, aq_strength=1.0, **_B3)),
]

# The source pass (aq.hip prep_aq_rows) and the mb_qp_delta flags of encode_inter: see
# tests/test_gpu_source_pass.py, whose clip builders this suite runs.  planes-*: random bytes at
# the shapes of the padding test (one with per-slot plans: every slot pads another display
# picture); flags-*: static noise with one changed and one intra-predictable MB per frame, 9 and
# 15 MBs (one and three live MBs in the last wave), one with per-slot plans: a slot codes a P
# picture while the other codes a B picture.
_SRC = dict(crf=None, qp=32, aq_strength=1.0, bframes=0)
_FLG = dict(crf=None, qp=26, aq_strength=1.0, bframes=3, lookahead=False)
SOURCE_CASES = [
    dict(id=f"planes-{w}x{h}", clip="random", width=w, height=h, slots=3, frames=4, seed=31 + i, params=dict(_SRC))
    for i, (w, h) in enumerate([(48, 32), (48, 24), (48, 18), (16, 24), (1040, 24), (40, 24)])
] + [
    dict(id="planes-48x24-per-slot-plans", clip="random", width=48, height=24, slots=3, frames=4, seed=41,
         anchors_at=[[2], [], [3]], params=dict(_SRC, bframes=2, lookahead=False)),
] + [
    dict(id=f"flags-{w}x48-trellis{tr}", clip="flags", width=w, height=48, slots=2, frames=6, seed=51 + i,
         need_flags=True, params=dict(_FLG, trellis=tr))
    for i, (w, tr) in enumerate([(48, 0), (48, 2), (80, 0), (80, 2)])
] + [
    dict(id="flags-80x48-per-slot-plans", clip="flags", width=80, height=48, slots=2, frames=6, seed=61,
         anchors_at=[[3], [2]], need_flags=True, params=dict(_FLG, trellis=2)),
]

# The chroma launch of the inter residual (encode_inter_chroma: eight MBs per wave): see
# tests/test_gpu_inter_chroma8.py, whose clip builder, spy and statistics this suite runs.  Sizes
# by nmb % 8: 48x32 -> 6 MBs (one partly filled wave), 48x48 -> 9 (one live MB in the second
# wave), 64x48 -> 12 (four), 80x48 -> 15 (seven; 5 MBs per row), 96x48 -> 18 (two), 112x48 -> 21
# (7 MBs per row: every wave straddles rows), 176x144 -> 99.  AQ is on everywhere (qp_flags live).
_C8P = dict(crf=None, bframes=0, aq_strength=1.0)
_C8B = dict(crf=None, bframes=3, weightb=True, aq_strength=1.0, lookahead=False)


def _c8(id_, family, w, h, frames, seed, kind, **params):
    return dict(id=id_, family=family, width=w, height=h, frames=frames, seed=seed, kind=kind, params=params)


CHROMA8_CASES = [
    _c8("48x32-p-part-t8-trellis2", "p-part", 48, 32, 6, 71, "default", qp=26, t8x8=True, trellis=2, chroma_qp_offset=-4,
        **_C8P, **_PART),
    _c8("112x48-p-part-not8-trellis0", "p-part", 112, 48, 6, 72, "zoom", qp=24, t8x8=False, trellis=0, **_C8P, **_PART),
    _c8("176x144-p-part-t8-trellis2", "p-part", 176, 144, 5, 73, "default", qp=28, t8x8=True, trellis=2,
        chroma_qp_offset=-6, **_C8P, **_PART),
    _c8("64x48-p-refs3-weightp-trellis2", "p-refs", 64, 48, 7, 74, "fade", qp=26, t8x8=False, trellis=2, refs=3,
        weightp=True, chroma_qp_offset=-4, **_C8P),
    _c8("80x48-p-refs3-weightp-t8-trellis0", "p-refs", 80, 48, 7, 75, "fade", qp=28, t8x8=True, trellis=0, refs=3,
        weightp=True, chroma_qp_offset=-6, **_C8P),
    _c8("176x144-p-refs3-weightp-trellis2", "p-refs", 176, 144, 6, 76, "fade", qp=26, t8x8=True, trellis=2, refs=3,
        weightp=True, ref_gate=0, chroma_qp_offset=-4, **_C8P),
    _c8("48x48-b-not8-trellis0", "b-weightb", 48, 48, 9, 77, "default", qp=26, t8x8=False, trellis=0, chroma_qp_offset=-4,
        **_C8B),
    _c8("80x48-b-t8-trellis2", "b-weightb", 80, 48, 9, 78, "pan-fast", qp=28, t8x8=True, trellis=2, chroma_qp_offset=-6,
        **_C8B),
    _c8("112x48-b-t8-trellis2", "b-weightb", 112, 48, 9, 79, "default", qp=24, t8x8=True, trellis=2, **_C8B),
    _c8("176x144-b-refs3-trellis0", "b-weightb", 176, 144, 9, 80, "zoom", qp=28, t8x8=True, trellis=0, refs=3,
        chroma_qp_offset=-6, **_C8B),
    # noise at a low QP (every block has levels), in the families of their picture types
    _c8("96x48-p-part-noise-lowqp", "p-part", 96, 48, 6, 81, "noise", qp=18, t8x8=True, trellis=2, **_C8P, **_PART),
    _c8("96x48-b-noise-lowqp", "b-weightb", 96, 48, 9, 82, "noise", qp=16, t8x8=True, trellis=2, **_C8B),
]

# The B decision (h264_b.hip: pre-pass, gated searches, main pass over the searched MBs): see
# tests/test_gpu_b_block_fetch.py, whose clip builder and statistics this suite runs.  need: the
# counts the case is there for (the wavefront decides direct against explicit itself: searched
# MBs get no direct quadrant from b_decide).
_BF = dict(crf=None, bframes=3, lookahead=False)
_BF_ALL = ["b_gated", "b_searched", "direct"]


def _bf(id_, w, h, frames, seed, kind, need, **params):
    return dict(id=id_, width=w, height=h, frames=frames, seed=seed, kind=kind, need=need, params=dict(_BF, **params))


BFETCH_CASES = [
    _bf("48x48-temporal-weightb", 48, 48, 9, 91, "default", _BF_ALL, qp=26, weightb=True, refs=1, partitions=False),
    _bf("80x48-temporal-weightb-aq-bgate-600", 80, 48, 9, 92, "default", _BF_ALL, qp=24, weightb=True, refs=1,
        aq_strength=1.0, b_gate=-600, partitions=False),
    _bf("176x144-refs2-pyramid", 176, 144, 9, 93, "default", _BF_ALL, qp=26, weightb=True, refs=2, pyramid=True),
    _bf("80x48-bpartitions", 80, 48, 9, 94, "default", _BF_ALL + ["b8x8_direct"], qp=24, weightb=True, refs=1,
        partitions=True, bpartitions=True, part_overhead=0, part_min_satd=0),
    _bf("176x144-bpartitions-zoom", 176, 144, 7, 95, "zoom", _BF_ALL + ["b8x8_direct"], qp=26, weightb=False, refs=1,
        partitions=True, bpartitions=True),
    _bf("80x48-spatial-fast", 80, 48, 9, 96, "default", _BF_ALL, qp=26, weightb=True, refs=1, direct="spatial"),
    _bf("176x144-spatial-wavefront-gate", 176, 144, 7, 97, "default", _BF_ALL, qp=26, weightb=True, refs=1,
        direct="spatial", spatial_wavefront=True, spatial_gate=True),
]

# The 16x16 motion search in whole encodes (me_search.h): every picture type and list search that
# calls it, at 15 MBs (5 per row: no MB has its window inside the picture), 49 (7 x 7) and 99.
# 112x112 and 176x144 have MBs on both the interior and the edge path of every phase.
_MQ = dict(crf=None, qp=26)
ME_CASES = [
    dict(id="h264-80x48-p", codec="h264", width=80, height=48, frames=5, seed=101, kind="default",
         params=dict(bframes=0, refs=1, **_MQ)),
    dict(id="h264-176x144-p-pan", codec="h264", width=176, height=144, frames=6, seed=102, kind="pan-fast",
         params=dict(bframes=0, refs=1, aq_strength=1.0, **_MQ)),
    dict(id="h264-112x112-b3-temporal", codec="h264", width=112, height=112, frames=9, seed=103, kind="default",
         params=dict(bframes=3, direct="temporal", refs=1, **_MQ)),
    dict(id="h264-176x144-b3-temporal-zoom", codec="h264", width=176, height=144, frames=9, seed=104, kind="zoom",
         params=dict(bframes=3, direct="temporal", weightb=True, **_MQ)),
    dict(id="h264-176x144-p-refs3-weightp-fade", codec="h264", width=176, height=144, frames=7, seed=105, kind="fade",
         params=dict(bframes=0, refs=3, weightp=True, **_MQ)),
    dict(id="h264-112x112-p-refs3-weightp", codec="h264", width=112, height=112, frames=6, seed=106, kind="default",
         params=dict(bframes=0, refs=3, weightp=True, ref_gate=0, **_MQ)),
    dict(id="h264-176x144-b3-pyramid", codec="h264", width=176, height=144, frames=9, seed=107, kind="default",
         params=dict(bframes=3, pyramid=True, refs=2, **_MQ)),
    dict(id="h264-80x48-b3-cavlc", codec="h264", width=80, height=48, frames=9, seed=108, kind="default",
         params=dict(bframes=3, cabac=False, **_MQ)),
    dict(id="h264-176x144-p-cavlc", codec="h264", width=176, height=144, frames=5, seed=109, kind="pan-fast",
         params=dict(bframes=0, cabac=False, **_MQ)),
    dict(id="hevc-176x144-p", codec="hevc", width=176, height=144, frames=6, seed=110, kind="default",
         params=dict(bframes=0, crf=None, qp=30)),
]

INTRA_KINDS = (0, 1, 4, 8)
SPLIT_KINDS = (5, 6, 7, 10, 11, 12)


def encode_case(case):
    """-> (encoder, results); the caller closes the encoder."""
    import torch
    from govideocompressor_amd.models.h264_gpu import GpuH264Encoder, H264Params, synth_clip

    p = H264Params(width=case["width"], height=case["height"], **case["params"])
    enc = GpuH264Encoder(p, slots=SLOTS)
    y, u, v = synth_clip(SLOTS, case["frames"], case["width"], case["height"], seed=case["seed"], kind=case["kind"])
    res = enc.encode(y, u, v, keep_recon=True)
    torch.cuda.synchronize()
    return enc, res


def record_stats(host, bitstreams):
    """What the decoded records say about the waves of encode_inter_mb (four consecutive MBs of
    a P / B picture): split partition MBs, waves with intra and inter MBs, waves with inter MBs
    on and off the 8x8 transform, MB QPs per picture."""
    import numpy as np

    out = dict(split=0, mixed_intra=0, mixed_t8=0, qps=0)
    for seg in host.parse(list(bitstreams), 1):
        for hdr in np.asarray(seg["hdr"]):
            kind, flags, qp = hdr[:, 0], hdr[:, 5], hdr[:, 2]
            intra = np.isin(kind, INTRA_KINDS)
            if intra.all():
                continue
            out["split"] += int(np.isin(kind, SPLIT_KINDS).sum())
            out["qps"] = max(out["qps"], int(np.unique(qp[~intra]).size))
            t8 = (flags & 2) != 0
            for w0 in range(0, kind.size, 4):
                i, t = intra[w0:w0 + 4], t8[w0:w0 + 4]
                out["mixed_intra"] += int(i.any() and not i.all())
                out["mixed_t8"] += int((t & ~i).any() and (~t & ~i).any())
    return out


def encode_decide_case(case):
    """-> (encoder, results); the caller closes the encoder.  HEVC cases run the host entropy
    writer with its CU counters on."""
    import torch
    from govideocompressor_amd.models.h264_gpu import synth_clip

    if case["codec"] == "h264":
        return encode_case(case)
    from govideocompressor_amd.models.hevc_gpu import GpuHevcEncoder, HevcParams

    p = HevcParams(width=case["width"], height=case["height"], **case["params"])
    enc = GpuHevcEncoder(p, slots=SLOTS, entropy="host")
    enc.cu_stats = {}
    y, u, v = synth_clip(SLOTS, case["frames"], case["width"], case["height"], seed=case["seed"], kind=case["kind"])
    res = enc.encode(y, u, v, keep_recon=True)
    torch.cuda.synchronize()
    return enc, res


def decide_stats(host, case, enc, bitstreams):
    """HEVC: merge + skip CUs of the P / B pictures (the writer's counters) and bi-predicted CUs
    (decoded records).  H.264: B_Direct_16x16 / B_Skip MBs (decoded records)."""
    import numpy as np

    if case["codec"] == "h264":
        direct = sum(int((np.asarray(seg["hdr"])[:, :, 0] == 13).sum()) for seg in host.parse(list(bitstreams), 1))
        return dict(direct=direct)
    merge = sum(int(st.get("merge_cus", 0)) + int(st.get("skip_cus", 0)) for k, st in enc.cu_stats.items() if k != "I")
    bi = 0
    for s in bitstreams:
        for p in host.hevc_decode(s):
            cu = p["cu"]
            bi += int(((cu[:, 0] == 1) & (cu[:, 12] == 3)).sum())
    return dict(merge=merge, bi=bi)


class _GateCounter:
    """Stands in for the encoder's kernel module: counts, per gated ``me`` launch, the MBs the
    gate stopped (cost kNoCost) and let through, from the encoder's own cost buffer.  The
    buffer is prefilled with a sentinel so that slots the launch skips (another picture type, a
    shorter list 0) are told apart; their rows are put back, so the encode is unchanged."""

    def __init__(self, enc):
        self._enc, self._hip = enc, enc.hip
        self.counts = dict(b_gated=0, b_searched=0, far_gated=0, far_searched=0)

    def __getattr__(self, name):
        return getattr(self._hip, name)

    def me(self, *a):
        if len(a) <= 24 or not a[18]:  # (positional as h264_gpu.py calls it: 18 = gate_cost, 24 = want)
            return self._hip.me(*a)
        enc = self._enc
        outs = [enc.me_cost] + ([enc.me_cost1] if hasattr(enc, "me_cost1") else [])
        outs += [enc.xcost[k] for k in range(enc.xcost.shape[0])] if hasattr(enc, "xcost") else []
        t = next(x for x in outs if x.data_ptr() == a[7])
        keep = t.clone()
        t.fill_(GATE_SENTINEL)
        self._hip.me(*a)
        live = (t != GATE_SENTINEL).any(dim=1)
        key = "b" if a[24] == 1 else "far"
        self.counts[key + "_gated"] += int((t[live] == NO_COST).sum())
        self.counts[key + "_searched"] += int((t[live] < NO_COST).sum())
        t[~live] = keep[~live]


def encode_gate_case(case):
    """-> (encoder, results, counts of _GateCounter); the caller closes the encoder."""
    import torch
    from govideocompressor_amd.models.h264_gpu import GpuH264Encoder, H264Params, synth_clip

    p = H264Params(width=case["width"], height=case["height"], **case["params"])
    enc = GpuH264Encoder(p, slots=SLOTS)
    counter = _GateCounter(enc)
    enc.hip = counter
    y, u, v = synth_clip(SLOTS, case["frames"], case["width"], case["height"], seed=case["seed"], kind=case["kind"])
    res = enc.encode(y, u, v, keep_recon=True)
    torch.cuda.synchronize()
    return enc, res, counter.counts


def gate_expect(case):
    """The counts that must be > 0 for the case to exercise both sides of its gates."""
    keys = []
    if case["params"]["b_gate"] != 0:
        keys += ["b_gated", "b_searched"]
    if case["params"].get("refs", 1) > 1 and case["params"].get("ref_gate", 0) > 0:
        keys += ["far_gated", "far_searched"]
    return keys


def record_intra(host, path) -> None:
    """Suite ``intra``: per case the per-slot hashes and the free / chained intra MB counts of
    the decoded P / B pictures.  The clips and the classifier are the test's own (the test
    module reads the golden file when imported, so a first recording starts from an empty one)."""
    import torch
    from govideocompressor_amd.models.h264_gpu import GpuH264Encoder, H264Params

    if not os.path.exists(path):
        with open(path, "w") as f:
            json.dump(dict(slots=SLOTS, cases=[]), f)
    from tests import test_gpu_intra_free as T

    rows = []
    for case in INTRA_CASES:
        case = json.loads(json.dumps(case))  # as the test will read it
        enc = GpuH264Encoder(H264Params(width=case["width"], height=case["height"], **case["params"]), slots=SLOTS)
        y, u, v = T._clip(case, SLOTS)
        res = enc.encode(y, u, v, keep_recon=True)
        torch.cuda.synchronize()
        slice_rows = int(enc.slice_rows)
        enc.close()
        streams = [bytes(r.bitstream) for r in res]
        counts, planted = T._counts(case, [host.decode(s) for s in streams], slice_rows)
        vac = [k for k in case["need"] if counts[k] == 0]
        for b, (kinds, intra, free, chained) in enumerate(planted):
            vac += [f"slot {b} {s} not intra" for s in case["spots"][b] if not intra[s[1], s[0]]]
            vac += [f"slot {b} {s} not free" for s in case.get("free_spots", [[], []])[b] if not free[s[1], s[0]]]
            vac += [f"slot {b} {s} not chained" for s in case.get("chained_spots", [[], []])[b] if not chained[s[1], s[0]]]
            if case.get("b_picture") and not np_isin_any(kinds, (9, 10, 11, 12, 13)):
                vac.append(f"slot {b}: not a B picture")
            if case.get("free_only") and chained.any():
                vac.append(f"slot {b}: chained MBs")
        print(case["id"], [len(s) for s in streams], counts, "VACUOUS: " + "; ".join(vac) if vac else "", flush=True)
        rows.append(dict(case, counts=counts, sha256=[hashlib.sha256(s).hexdigest() for s in streams]))
    with open(path, "w") as f:
        json.dump(dict(slots=SLOTS, cases=rows), f, indent=1)
        f.write("\n")


def record_source(host, path) -> None:
    """Suite ``source``: per case the per-slot hashes.  The clips are the test's own (the test
    module reads the golden file when imported, so a first recording starts from an empty one)."""
    import numpy as np

    if not os.path.exists(path):
        with open(path, "w") as f:
            json.dump(dict(cases=[]), f)
    from tests import test_gpu_source_pass as T

    rows = []
    for case in SOURCE_CASES:
        case = json.loads(json.dumps(case))  # as the test will read it
        enc, res, _ = T._encode(case)
        streams = [bytes(r.bitstream) for r in res]
        kinds = [np.unique(np.asarray(seg["hdr"])[:, :, 0]).tolist() for seg in host.parse(streams, 1)]
        enc.close()
        print(case["id"], [len(s) for s in streams], "MB kinds per slot", kinds, flush=True)
        rows.append(dict(case, sha256=[hashlib.sha256(s).hexdigest() for s in streams]))
    with open(path, "w") as f:
        json.dump(dict(cases=rows), f, indent=1)
        f.write("\n")


def record_chroma8(host, path) -> None:
    """Suite ``chroma8``: per case the per-slot hashes, the record statistics and the counts of the
    mb_qp_delta flag bytes.  The clips, the spy and the statistics are the test's own (the test
    module reads the golden file when imported, so a first recording starts from an empty one)."""
    if not os.path.exists(path):
        with open(path, "w") as f:
            json.dump(dict(slots=SLOTS, cases=[]), f)
    from tests import test_gpu_inter_chroma8 as T

    rows, fam = [], {}
    for case in CHROMA8_CASES:
        case = json.loads(json.dumps(case))  # as the test will read it
        enc, res, spy = T.encode(case, SLOTS)
        streams = [bytes(r.bitstream) for r in res]
        enc.close()
        stats = T.chroma_stats(host, streams)
        print(case["id"], [len(s) for s in streams], stats, "flag bytes", spy.counts, flush=True)
        tot = fam.setdefault(case["family"], {})
        for k, n in list(stats.items()) + [(f"flag{k}", n) for k, n in spy.counts.items()]:
            tot[k] = tot.get(k, 0) + n
        rows.append(dict(case, stats=stats, flag_bytes={str(k): n for k, n in spy.counts.items()},
                         sha256=[hashlib.sha256(s).hexdigest() for s in streams]))
    for name, tot in fam.items():
        vac = [k for k in T._NEED[name] + ("flag0", "flag1", "flag2") if tot[k] == 0]
        print("family", name, tot, "VACUOUS: " + ",".join(vac) if vac else "", flush=True)
    with open(path, "w") as f:
        json.dump(dict(slots=SLOTS, cases=rows), f, indent=1)
        f.write("\n")


def record_bfetch(host, path) -> None:
    """Suite ``bfetch``: per case the per-slot hashes, the gate's counts and the direct MBs /
    quadrants of the decoded records.  The clips and the statistics are the test's own (the test
    module reads the golden file when imported, so a first recording starts from an empty one)."""
    if not os.path.exists(path):
        with open(path, "w") as f:
            json.dump(dict(slots=SLOTS, cases=[]), f)
    from tests import test_gpu_b_block_fetch as T

    rows = []
    for case in BFETCH_CASES:
        case = json.loads(json.dumps(case))  # as the test will read it
        enc, res, counts = T.encode(case, SLOTS)
        streams = [bytes(r.bitstream) for r in res]
        enc.close()
        counts.update(T.b_stats(host, streams))
        vac = [k for k in case["need"] if counts[k] == 0]
        print(case["id"], [len(s) for s in streams], counts, "VACUOUS: " + ",".join(vac) if vac else "", flush=True)
        rows.append(dict(case, counts=counts, sha256=[hashlib.sha256(s).hexdigest() for s in streams]))
    with open(path, "w") as f:
        json.dump(dict(slots=SLOTS, cases=rows), f, indent=1)
        f.write("\n")


def record_mask(host, path) -> None:
    """Suite ``mask``: per case the per-slot hashes and the record statistics.  The cases, the
    clips and the statistics are the test's own (the test module reads the golden file when
    imported, so a first recording starts from an empty one)."""
    if not os.path.exists(path):
        with open(path, "w") as f:
            json.dump(dict(slots=SLOTS, cases=[]), f)
    from tests import test_gpu_inter_block_mask as T

    rows, tot = [], {}
    for case in T.CASES:
        case = json.loads(json.dumps(case))  # as the test will read it
        enc, res, spy = T.encode(case, poison=False)
        if spy.mask_pre != {False}:
            raise SystemExit("this kernel library writes block masks: not the parent's")
        streams = [bytes(r.bitstream) for r in res]
        enc.close()
        stats = T.record_stats(host, streams)
        vac = [k for k in T._NEED.get(case["id"], ()) if stats[k] == 0]
        print(case["id"], [len(s) for s in streams], stats, "VACUOUS: " + ",".join(vac) if vac else "", flush=True)
        for k, n in stats.items():
            tot[k] = tot.get(k, 0) + n
        rows.append(dict(case, stats=stats, sha256=[hashlib.sha256(s).hexdigest() for s in streams]))
    vac = [k for k in T._NEED_ALL if tot[k] == 0]
    print("all cases", tot, "VACUOUS: " + ",".join(vac) if vac else "", flush=True)
    with open(path, "w") as f:
        json.dump(dict(slots=SLOTS, cases=rows), f, indent=1)
        f.write("\n")


def record_deblock(host, path) -> None:
    """Suite ``deblock``: per case the per-slot hashes of the bitstream and of the kept
    reconstruction (every picture filtered), with the share of P-picture MBs whose 32 boundary
    strengths are all zero (from the parser).  The cases and the clips are the test's own."""
    import numpy as np
    from tests import test_gpu_deblock_encode as T

    rows = []
    for case in T.CASES:
        case = json.loads(json.dumps(case))  # as the test will read it
        streams, recon, bs = T.encode(case)
        if bs:
            raise SystemExit("this kernel library has the deblocking pre-pass: not the parent's")
        quiet = [float((np.asarray(seg["bs"])[np.asarray(seg["meta"])[:, 4] % 5 == 0] == 0).all(axis=2).mean())
                 for seg in host.parse(streams, 1)]
        print(case["id"], [len(s) for s in streams], "quiet MBs of P pictures", [round(q, 3) for q in quiet], flush=True)
        rows.append(dict(case, **T.hashes(streams, recon)))
    with open(path, "w") as f:
        json.dump(dict(slots=SLOTS, cases=rows), f, indent=1)
        f.write("\n")


def np_isin_any(a, values) -> bool:
    import numpy as np

    return bool(np.isin(a, values).any())


def main() -> None:
    suite = "inter"
    if len(sys.argv) == 3 and sys.argv[1] in ("inter", "decide", "gate", "intra", "source", "chroma8", "bfetch", "mask", "me",
                                              "deblock"):
        suite = sys.argv.pop(1)
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    lib = os.environ.get("MIVC_HIP_LIB")
    if not lib or not os.path.exists(lib):
        raise SystemExit("MIVC_HIP_LIB must name a kernel library built from the parent commit")
    from govideocompressor_amd.ops import native

    host = native.host()
    rows = []
    if suite == "intra":
        record_intra(host, sys.argv[1])
        return
    if suite == "source":
        record_source(host, sys.argv[1])
        return
    if suite == "chroma8":
        record_chroma8(host, sys.argv[1])
        return
    if suite == "bfetch":
        record_bfetch(host, sys.argv[1])
        return
    if suite == "mask":
        record_mask(host, sys.argv[1])
        return
    if suite == "deblock":
        record_deblock(host, sys.argv[1])
        return
    if suite == "gate":
        for case in GATE_CASES:
            enc, res, counts = encode_gate_case(case)
            streams = [bytes(r.bitstream) for r in res]
            enc.close()
            vac = [k for k in gate_expect(case) if counts[k] == 0]
            print(case["id"], [len(s) for s in streams], counts, "VACUOUS: " + ",".join(vac) if vac else "", flush=True)
            rows.append(dict(case, counts=counts, sha256=[hashlib.sha256(s).hexdigest() for s in streams]))
    for case in ([] if suite == "gate" else CASES if suite == "inter" else ME_CASES if suite == "me" else DECIDE_CASES):
        if suite == "inter":
            enc, res = encode_case(case)
        else:
            try:
                enc, res = encode_decide_case(case)
            except Exception as e:  # noqa: BLE001  the parent rejects the combination: not recorded
                print(case["id"], "DROPPED:", repr(e), flush=True)
                continue
        streams = [bytes(r.bitstream) for r in res]
        stats = (record_stats(host, streams) if suite == "inter" else {} if suite == "me" else
                 decide_stats(host, case, enc, streams))
        enc.close()
        print(case["id"], [len(s) for s in streams], stats, flush=True)
        rows.append(dict(case, sha256=[hashlib.sha256(s).hexdigest() for s in streams]))
    with open(sys.argv[1], "w") as f:
        json.dump(dict(slots=SLOTS, cases=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
