"""Time the H.264 deblocking launches alone at the headline batch shape (B slots of 1080p, the
records and the unfiltered-again reconstruction of an encoded P picture): the pre-pass deblock_bs
and the wavefront, each alone.  With a kernel library from before the pre-pass (MIVC_HIP_LIB) the
one launch of that time.

    python tools/time_deblock.py [B]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from govideocompressor_amd.models.h264_gpu import GpuH264Encoder, H264Params, synth_clip  # noqa: E402


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    enc = GpuH264Encoder(H264Params(width=1920, height=1080, lookahead=False, bframes=0), slots=B)
    y, u, v = synth_clip(B, 2, 1920, 1080, seed=5)
    enc.encode(y, u, v, metrics=False, keep_recon=False)
    torch.cuda.synchronize()
    P = lambda t: t.data_ptr()  # noqa: E731
    s = torch.cuda.current_stream().cuda_stream
    # the P picture's records: the parity whose MBs are mostly inter; planes: contiguous [B]
    # copies of pool buffer 0 (filtered once already: the timing is of the launch, and the
    # strengths, which decide what runs, come from the records)
    k = max(range(2), key=lambda i: int((enc.hdr[i][:, :, 0] >= 2).sum()))
    hdr = enc.hdr[k]
    cur = [p[:, 0].contiguous() for p in enc.rec_pool]
    new = hasattr(enc.hip, "deblock_bs")
    kw = dict(bs=P(enc.dbk_bs), info=P(enc.dbk_info)) if new else {}

    def pre():
        enc.hip.deblock_bs(B, enc.wmb, enc.hmb, P(hdr), P(enc.nz), kw["bs"], kw["info"], s)

    def wavefront():
        enc.hip.deblock(B, enc.wmb, enc.hmb, P(cur[0]), P(cur[1]), P(cur[2]), P(hdr), P(enc.nz),
                        enc.p.chroma_qp_offset, 0, 0, P(enc.err), s, **kw)

    def timed(fn, n=5):
        fn()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(n):
            fn()
        ev1.record()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) / n

    if new:
        t_pre = timed(pre)
        info = enc.dbk_info.view(B, -1)
        quiet = float(((info >> 8) & 255).eq(0).float().mean())
        print(f"deblock_bs B={B}: {t_pre:.3f} ms; MBs with every edge off: {100 * quiet:.1f} %", flush=True)
    print(f"deblock B={B}: {timed(wavefront):.3f} ms, err={int(enc.err.item())}", flush=True)


if __name__ == "__main__":
    main()
