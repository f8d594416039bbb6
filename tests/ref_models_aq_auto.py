"""Float64 model of auto-variance adaptive quantisation (x264 --aq-mode 2 / 3, csrc/kernels/aq_auto.h)
on top of ref_models.aq_energy / mb_blocks.  Per slot and coded picture, over its N 16x16 blocks
with energy e_i at bit depth bd:

    c     = 1 / 4^(bd - 8)
    a_i   = (e_i * c + 1) ^ 0.125
    m     = mean a_i          m2 = mean a_i^2
    avg   = m - 0.5 * (m2 - 14) / m
    mode 2:  adj_i = s * m * (a_i - avg)
    mode 3:  adj_i = s * m * (a_i - avg) + s * (1 - 14 / a_i^2)

The functions return the unrounded ``adj`` so that a caller can build the band around its
half-integers; rounding and clamps are those of mode 1 (ref_models.aq_offset_h264 / aq_ctb_hevc).
"""
import numpy as np

BAND, BAND_CAP = 1e-3, 0.01


def aq_auto_terms(e, bd: int = 8) -> np.ndarray:
    """a_i of every block: e [..., N] integer energies -> float64 [..., N]."""
    c = 1.0 / 4.0 ** (bd - 8)
    return (np.asarray(e, dtype=np.int64).astype(np.float64) * c + 1.0) ** 0.125


def aq_auto_stats(a):
    """(m, avg) of each picture: a [..., N] -> two arrays [..., 1]."""
    m = a.mean(axis=-1, keepdims=True)
    m2 = (a * a).mean(axis=-1, keepdims=True)
    return m, m - 0.5 * (m2 - 14.0) / m


def aq_auto_adj(e, mode: int, strength: float, extra=None, bd: int = 8, stats=None) -> np.ndarray:
    """The unrounded offsets: e [..., N] (the last axis is one picture) -> float64 [..., N].
    extra: optional per-block term added to them; stats: (m, avg) to use instead of the
    pictures' own (a test evaluates a slot with its neighbour's statistics that way)."""
    if mode not in (2, 3):
        raise ValueError("mode 2 or 3")
    a = aq_auto_terms(e, bd)
    m, avg = aq_auto_stats(a) if stats is None else stats
    adj = float(strength) * m * (a - avg)
    if mode == 3:
        adj = adj + float(strength) * (1.0 - 14.0 / (a * a))
    if extra is not None:
        adj = adj + np.asarray(extra, dtype=np.float64)
    return adj


def offset_h264(adj) -> np.ndarray:
    """Per-MB QP offset: round-half-even, clamped to +-24."""
    return np.clip(np.rint(adj), -24, 24).astype(np.int64)


def ctb_mean(adj4) -> np.ndarray:
    """adj of a CTB's four blocks on the last axis -> the CTB's unrounded offset."""
    return 0.25 * np.asarray(adj4).sum(axis=-1)


def ctb_qp_hevc(mean, base_qp) -> np.ndarray:
    """Per-CTB QP: base_qp plus the rounded mean clamped to +-12, the sum clamped to 0 .. 51."""
    off = np.clip(np.rint(mean), -12, 12).astype(np.int64)
    return np.clip(np.asarray(base_qp, dtype=np.int64) + off, 0, 51)


def check_band(got, want, adj, what):
    """The comparison rule of tests/test_gpu_aq_model.py: equal outside a band of BAND around the
    half-integers of the float64 ``adj``, at most one apart inside it, at most BAND_CAP of the
    values in the band.  Returns the band's share."""
    got, want = np.asarray(got, dtype=np.int64), np.asarray(want, dtype=np.int64)
    band = np.abs(adj - np.floor(adj) - 0.5) < BAND
    share = float(band.mean())
    diff = got - want
    print(what, "distinct", np.unique(want).size, "range", int(want.min()), int(want.max()), "band share", share,
          "differ inside the band", int((diff[band] != 0).sum()), "outside", int((diff[~band] != 0).sum()))
    assert share <= BAND_CAP
    bad = np.argwhere((diff != 0) & ~band)
    assert bad.size == 0, f"{what}: {len(bad)} blocks differ, first {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
    assert np.abs(diff).max() <= 1
    return share
