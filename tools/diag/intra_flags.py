"""Diagnostics: where the intra MBs of P and B pictures lie, and how many of them depend on
another intra MB of their picture (encode_intra.hip codes those in wavefront order; the others
are free to be coded in any order).

Reads ``enc.intra_flag`` after every inter coding step of one batch of the headline content
(bench.py's clip of step 0: seed 1000, 60 frames of 1920x1080, CRF 23) and prints, per picture
class, the intra MBs per slot-picture, the share that is free (none of the left / top-left /
top / top-right neighbours is intra) and chained (the rest), the longest true dependency chain
per picture and the largest count in one MB row.

    python tools/diag/intra_flags.py [slots=16] [frames=60]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from govideocompressor_amd.models.h264_gpu import GpuH264Encoder, H264Params, synth_clip  # noqa: E402


def classify(f: np.ndarray, slice_rows: int = 0):
    """f: [hmb, wmb] bool intra map of one picture -> (free, chained, depth): bool maps and the
    length of the longest dependency chain ending at each intra MB (1 for a free MB)."""
    hmb, wmb = f.shape
    top = np.ones(hmb, dtype=bool)
    top[0] = False
    if slice_rows > 0:
        top[::slice_rows] = False
    p = np.zeros((hmb + 1, wmb + 2), dtype=bool)
    p[1:, 1:-1] = f
    left = p[1:, :-2]
    tl, t, tr = (p[:-1, :-2] & top[:, None], p[:-1, 1:-1] & top[:, None], p[:-1, 2:] & top[:, None])
    dep = left | tl | t | tr
    depth = np.zeros((hmb + 1, wmb + 2), dtype=np.int32)
    for y, x in zip(*np.nonzero(f)):  # raster order: every dependency comes earlier
        d = depth[y + 1, x]
        if top[y]:
            d = max(d, depth[y, x], depth[y, x + 1], depth[y, x + 2])
        depth[y + 1, x + 1] = d + 1
    return f & ~dep, f & dep, depth[1:, 1:-1]


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    F = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    W, H = 1920, 1080
    enc = GpuH264Encoder(H264Params(width=W, height=H, fps=30.0, crf=23.0, bframes=3), slots=B)
    y, u, v = synth_clip(B, F, W, H, seed=1000)
    rows = {"P": [], "B": []}  # per slot-picture: (intra, free, chained, longest chain, most in a row)
    step = enc._encode_step

    def spy(st, hdr, coef, cut=None):
        step(st, hdr, coef, cut)
        if not (st["P"] or st["B"]):
            return
        flags = enc.intra_flag.cpu().numpy().reshape(B, enc.hmb, enc.wmb) != 0
        for b, k in enumerate(st["kinds"]):
            if k not in (0, 1):
                continue
            free, chained, depth = classify(flags[b], enc.slice_rows)
            rows["PB"[k]].append((int(flags[b].sum()), int(free.sum()), int(chained.sum()), int(depth.max()),
                                  int(flags[b].sum(axis=1).max())))

    enc._encode_step = spy
    enc.encode(y, u, v, metrics=False, keep_recon=False)
    torch.cuda.synchronize()
    print(f"{B} slots x {F} frames of {W}x{H}, {enc.wmb * enc.hmb} MBs per picture")
    for k in ("P", "B"):
        a = np.array(rows[k], dtype=np.int64).reshape(-1, 5)
        n = max(1, int(a[:, 0].sum()))
        print(f"{k}: {len(a)} slot-pictures, intra MBs {int(a[:, 0].sum())} (mean {a[:, 0].mean():.1f}, max {a[:, 0].max()} "
              f"per slot-picture), free {a[:, 1].sum() / n:.1%}, chained {a[:, 2].sum() / n:.1%}, "
              f"longest chain mean {a[:, 3].mean():.2f} max {a[:, 3].max()}, most in one row mean {a[:, 4].mean():.2f} "
              f"max {a[:, 4].max()}", flush=True)
    enc.close()


if __name__ == "__main__":
    main()
