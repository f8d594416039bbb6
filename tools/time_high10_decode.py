#!/usr/bin/env python3
"""High 10 H.264 decode, CPU route against GPU route (profiles/high10_gpu_decode.md).

One batch of ``--segments`` random-record 10-bit segments (``--size`` WxH, ``--frames`` pictures
each, CABAC, 8x8 transform, intra MBs in P pictures) is parsed once and reconstructed with
``GpuH264Decoder(high_depth="cpu")`` and ``high_depth="gpu"`` in turn, ``--repeats`` times each
after one warm-up; prints ``stats["gpu_s"]`` / ``stats["cpu_fallback_s"]`` of every repeat and
checks that the two routes return the same planes.

    python tools/time_high10_decode.py --cache segs.pkl --make-only   # no GPU needed
    python tools/time_high10_decode.py --cache segs.pkl
    rocprofv3 --kernel-trace --stats -d out -o run -- python tools/time_high10_decode.py --cache segs.pkl --route gpu

The segments are generated from seeds; ``--cache`` keeps them in a file so that a GPU run does
not spend its time in the numpy record generator.
"""
import argparse
import os
import pickle
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def segments(host, a):
    if a.cache and os.path.exists(a.cache):
        with open(a.cache, "rb") as f:
            key, segs = pickle.load(f)
        if key == (a.size, a.frames, a.segments, a.bit_depth):
            return segs
    from govideocompressor_amd.utils.h264_synth import random_stream
    w, h = (int(x) for x in a.size.split("x"))
    segs = [random_stream(host, w, h, a.frames, seed=900 + i, cabac=True, t8x8=True, intra_in_p=0.2, refs=2,
                          bit_depth=a.bit_depth) for i in range(a.segments)]
    if a.cache:
        with open(a.cache, "wb") as f:
            pickle.dump(((a.size, a.frames, a.segments, a.bit_depth), segs), f)
    return segs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="640x368")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--segments", type=int, default=16)
    ap.add_argument("--bit-depth", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--route", default="both", choices=["both", "cpu", "gpu"])
    ap.add_argument("--cache", default=None)
    ap.add_argument("--make-only", action="store_true")
    a = ap.parse_args()
    from govideocompressor_amd.ops import native
    host = native.host()
    segs = segments(host, a)
    print(f"{len(segs)} segments, {a.size}, {a.frames} pictures, {a.bit_depth}-bit, {sum(map(len, segs))} bytes")
    if a.make_only:
        return
    import torch
    from govideocompressor_amd.models.h264_decode_gpu import GpuH264Decoder
    routes = ["cpu", "gpu"] if a.route == "both" else [a.route]
    dec = {r: GpuH264Decoder(high_depth=r) for r in routes}
    t0 = time.perf_counter()
    parsed = dec[routes[0]].parse(segs)
    print(f"parse_s {time.perf_counter() - t0:.4f}")
    out = {}
    for rep in range(a.repeats + 1):  # repeat 0 warms up; routes alternate
        for r in routes:
            out[r] = dec[r].reconstruct(parsed)
            torch.cuda.synchronize()
            s = dec[r].stats
            tag = "warmup" if rep == 0 else f"repeat {rep}"
            print(f"{tag} high_depth={r}: gpu_s {s['gpu_s']:.4f} cpu_fallback_s {s['cpu_fallback_s']:.4f} "
                  f"segments_gpu {s['segments_gpu']} segments_cpu {s['segments_cpu']}")
    if len(routes) == 2:
        same = all(torch.equal(x.y, y.y) and torch.equal(x.u, y.u) and torch.equal(x.v, y.v)
                   for x, y in zip(out["cpu"], out["gpu"]))
        print("routes agree:", same)
        if not same:
            raise SystemExit(1)


if __name__ == "__main__":
    main()
