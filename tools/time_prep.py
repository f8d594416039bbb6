"""Time the source pass (padding + AQ offsets) and the mb_qp_delta flag pass alone at the
headline batch shape: B slots of 1920x1080 taken out of a [B, 4, 1080, 1920] clip with one
frame index per slot, ms per launch (mean of 5) and the GB/s that implies.

    [MIVC_HIP_LIB=abso/parent.so] python tools/time_prep.py [B]

A kernel library from before the fused launch reports the old launches only.
"""
import sys

import numpy as np
import torch

from govideocompressor_amd.models.h264_gpu import COEF_PER_MB, MB_HDR_BYTES, ROUTE_DTYPE, synth_clip
from govideocompressor_amd.ops import native


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    hip = native.hip()
    w, h, F, W, H = 1920, 1080, 4, 1920, 1088
    wmb, hmb = W // 16, H // 16
    nmb = wmb * hmb
    y, u, v = synth_clip(B, F, w, h, seed=5)
    dev = y.device
    oy = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    ou, ov = (torch.empty((B, H // 2, W // 2), dtype=torch.uint8, device=dev) for _ in range(2))
    aq = torch.zeros((B, nmb), dtype=torch.int8, device=dev)
    fsel = torch.from_numpy((np.arange(B) % F).astype(np.int32)).to(dev)
    hdr = torch.zeros((B, nmb, MB_HDR_BYTES), dtype=torch.uint8, device=dev)
    coef = torch.zeros((B, nmb, COEF_PER_MB), dtype=torch.int16, device=dev)
    nz = torch.zeros((B, nmb, 16), dtype=torch.uint8, device=dev)
    flags = torch.zeros((B, nmb), dtype=torch.uint8, device=dev)
    qp = torch.full((B,), 27, dtype=torch.int32, device=dev)
    # every slot codes a P picture; 1 % of the MBs were handed to the intra kernels
    rt = np.zeros(B, dtype=ROUTE_DTYPE)
    rt_d = torch.from_numpy(rt.view(np.uint8).reshape(B, 32)).to(dev)
    g = torch.Generator(device="cpu").manual_seed(1)
    r = torch.rand((B, nmb), generator=g)
    pre = ((r < 0.5).to(torch.uint8) + (r > 0.99).to(torch.uint8) * 2).to(dev)
    P = lambda t: t.data_ptr()  # noqa: E731
    s = torch.cuda.current_stream().cuda_stream
    cs = (w // 2) * (h // 2)

    def old():
        hip.prep(P(y), P(u), P(v), w, h, F * h * w, F * cs, B, P(oy), P(ou), P(ov), w, h, W, H, s, P(fsel))
        hip.aq_offsets(B, wmb, hmb, P(oy), P(ou), P(ov), 1.0, P(aq), s)

    def fused():
        assert hip.prep_aq(P(y), P(u), P(v), w, h, F * h * w, F * cs, B, P(oy), P(ou), P(ov), W, H, 1.0, P(aq), s, P(fsel))

    def fixup(**kw):
        hip.qp_fixup(B, wmb, hmb, P(hdr), P(coef), P(nz), P(flags), P(qp), s, 0, **kw)

    def run(fn, n=5):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        ev0.record()
        for _ in range(n):
            fn()
        ev1.record()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) / n

    src = B * (w * h + 2 * cs)        # bytes of the clip's pictures
    pad = B * (W * H * 3 // 2)        # bytes of the coded-size planes
    lv = B * nmb * 350                # what the flag pass reads per MB from the levels, about
    rows = [("prep + aq_offsets", old, src + 2 * pad)]
    if hasattr(hip, "prep_aq"):
        rows.append(("prep_aq (one launch)", fused, src + pad))
    rows.append(("qp_fixup", fixup, lv))
    if hasattr(hip, "prep_aq"):
        rows.append(("qp_fixup with pre", lambda: fixup(pre=P(pre), route=P(rt_d)), B * nmb * 2))
    for name, fn, nbytes in rows:
        ms = run(fn)
        print(f"{name}: {ms:.3f} ms, {nbytes / 1e9:.2f} GB moved, {nbytes / ms / 1e6:.0f} GB/s", flush=True)


if __name__ == "__main__":
    main()
