"""MapColToList0 of temporal direct prediction under a b-pyramid (models/gop.py col_to_list0):
the host-side map against a brute force over the plans, and the SlotRoute row that carries it."""
import numpy as np
import pytest

from govideocompressor_amd.models.gop import col_to_list0, dpb_frames, h264_plan

_TYPES = ["IBBBPBBBP", "IBBPBBBPBP", "IBPBBBP", "IBBBPBBPBBBPBPBBP"]
_REFS = [1, 2, 3, 4]


def _brute(cur, col):
    """[l][r] -> lowest index of the named picture in cur.refs0, None when absent, or "free" where
    the co-located list has no entry r (no block can carry that refIdxCol)."""
    out = []
    for names in (col.refs0, col.refs1):
        row = []
        for r in range(4):
            if r >= len(names):
                row.append("free")
                continue
            hit = [i for i, d in enumerate(cur.refs0) if d == names[r]]
            row.append(hit[0] if hit else None)
        out.append(row)
    return out


def _b_pictures(types, refs, pyramid):
    nb = max(len(run) for run in types[1:].replace("I", "P").split("P"))
    plan = h264_plan(types, refs, pyramid, dpb_frames(refs, pyramid, nb))
    by_d = {p.d: p for p in plan}
    return [(p, by_d[p.l1]) for p in plan if p.kind == "B"]


def test_col_to_list0_matches_brute_force():
    seen_shift = seen_none = 0
    for types in _TYPES:
        for refs in _REFS:
            for cur, col in _b_pictures(types, refs, True):
                got, want = col_to_list0(cur, col), _brute(cur, col)
                for l in range(2):
                    for r in range(4):
                        if want[l][r] == "free":
                            continue
                        assert got[l][r] == want[l][r], (types, refs, cur.d, col.d, l, r, got, want)
                        seen_none += want[l][r] is None
                        seen_shift += want[l][r] is not None and want[l][r] != r
    # the plans exercise both cases (else the comparison above is vacuous)
    assert seen_shift > 0 and seen_none > 0, (seen_shift, seen_none)


def test_col_to_list0_issue_table():
    """The worked example: IBBBPBBBP at refs 3, coding order I0 P4 B2 B1 B3 P8 B6 B5 B7."""
    pics = {cur.d: (cur, col) for cur, col in _b_pictures("IBBBPBBBP", 3, True)}
    m = {d: col_to_list0(*pics[d]) for d in pics}
    assert pics[1][1].d == 2 and pics[5][1].d == 6 and pics[3][1].d == 4 and pics[7][1].d == 8
    assert m[2][0][0] == 0
    assert m[1][0][0] == 0 and m[1][1][0] is None          # B1 <- B2: list 1 names P4
    assert m[3][0][0] == 1                                  # B3: B2 in front of I0
    assert m[6][0][:3] == (0, 1, 2)
    assert m[5][0][:3] == (0, 1, None) and m[5][1][0] is None
    assert m[7][0][:3] == (1, 2, None)


@pytest.mark.parametrize("types", _TYPES)
def test_col_to_list0_identity_without_pyramid(types):
    for refs in _REFS:
        for cur, col in _b_pictures(types, refs, False):
            assert col.kind == "P"
            got = col_to_list0(cur, col)
            for r in range(len(col.refs0)):
                assert got[0][r] in (r, None), (types, refs, cur.d, got)
                # (every anchor the co-located P names is in the B picture's list 0 here)
                assert got[0][r] == r


def test_route_row_and_map_table_layout():
    """The route row keeps the size the kernels step by; the map travels beside it as offsets
    from refIdxCol, so zeros (and plans without a pyramid) are the identity."""
    from govideocompressor_amd.models.h264_gpu import COL_NONE, ROUTE_DTYPE, col_map_row
    from govideocompressor_amd.ops import native

    assert ROUTE_DTYPE.itemsize == native.hip().route_bytes()
    assert ROUTE_DTYPE.itemsize % 8 == 0
    pics = {cur.d: (cur, col) for cur, col in _b_pictures("IBBBPBBBP", 3, True)}
    row = col_map_row(*pics[7])  # 0 -> 1, 1 -> 2, 2 -> none
    assert row.dtype == np.int8 and row.shape == (2, 4)
    assert row[0].tolist() == [1, 1, COL_NONE, 0] and row[1].tolist() == [0, 0, 0, 0]
    assert col_map_row(*pics[1])[1, 0] == COL_NONE
    for types in _TYPES:
        for refs in _REFS:
            for cur, col in _b_pictures(types, refs, False):
                assert not col_map_row(cur, col).any()
