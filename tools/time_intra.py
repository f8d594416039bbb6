"""Time the H.264 intra launch of a P / B coding step alone at the headline batch shape
(B slots of 1920x1088, Intra16x16 + chroma, no I4x4 / I8x8 trial) on synthetic maps of the MBs
that encode_inter left to it.

    python tools/time_intra.py [B]

The flag map and the per-slot counts are put back before every launch (the launch may
reclassify them in place); each launch is timed by its own pair of events, mean of 5.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from govideocompressor_amd.models.h264_gpu import GpuH264Encoder, H264Params, synth_clip  # noqa: E402


def flag_maps(B, hmb, wmb, dev):
    """name -> [B, hmb, wmb] uint8 maps.  'Singly' = on the even-even lattice, so that no two
    flagged MBs touch; the 2x2 groups sit on a lattice of four."""
    g = torch.Generator(device="cpu").manual_seed(7)
    nmb = hmb * wmb
    n = round(0.004 * nmb)

    def lattice(step, count, size):
        m = torch.zeros((B, hmb, wmb), dtype=torch.uint8)
        ys, xs = (hmb - size) // step + 1, (wmb - size) // step + 1
        for b in range(B):
            pick = torch.randperm(ys * xs, generator=g)[:count]
            for dy in range(size):
                for dx in range(size):
                    m[b, (pick // xs) * step + dy, (pick % xs) * step + dx] = 1
        return m

    single = lattice(2, n, 1)
    heavy = single.clone()
    heavy[B // 2].view(-1)[torch.randperm(nmb, generator=g)[:round(0.05 * nmb)]] = 1
    maps = {
        "no intra MB": torch.zeros((B, hmb, wmb), dtype=torch.uint8),
        "0.4 % scattered singly": single,
        "0.4 % in 2x2 groups": lattice(4, max(1, n // 4), 2),
        "one slot 5 %, the others 0.4 %": heavy,
        "every MB intra": torch.ones((B, hmb, wmb), dtype=torch.uint8),
    }
    return {k: m.to(dev) for k, m in maps.items()}


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    enc = GpuH264Encoder(H264Params(width=1920, height=1080, lookahead=False), slots=B)
    y, u, v = synth_clip(B, 2, 1920, 1080, seed=5)
    enc.encode(y, u, v, metrics=False, keep_recon=False)
    enc._prep(y, u, v, 1)
    torch.cuda.synchronize()
    dev = enc.intra_flag.device
    P = lambda t: t.data_ptr()  # noqa: E731
    s = torch.cuda.current_stream().cuda_stream
    enc.qp.fill_(27)
    # unrouted: each slot's reconstruction is its own plane (a copy of the source, so that the
    # neighbours of an intra MB look like a reconstructed picture)
    rec = [x.clone() for x in enc.src]
    flags, counts = enc.intra_flag, enc.intra_count

    def launch():
        enc.hip.encode_intra(B, enc.wmb, enc.hmb, P(enc.src[0]), P(enc.src[1]), P(enc.src[2]), P(rec[0]), P(rec[1]),
                             P(rec[2]), P(enc.qp), enc.p.chroma_qp_offset, P(enc.hdr[0]), P(enc.coef[0]), P(enc.nz),
                             P(flags), P(counts), P(enc.err), 0, s, 0, 0, 0, 0, enc.slice_rows,
                             trellis=enc.p.eff_intra_trellis(), trellis_lambda=float(enc.p.trellis_lambda))

    for name, m in flag_maps(B, enc.hmb, enc.wmb, dev).items():
        cnt = m.view(B, -1).sum(dim=1, dtype=torch.int32)
        ms = []
        for i in range(6):  # the first launch warms up
            flags.copy_(m.view(B, -1))
            counts.copy_(cnt)
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            launch()
            ev1.record()
            torch.cuda.synchronize()
            ms.append(ev0.elapsed_time(ev1))
        ms = ms[1:]
        print(f"{name}: {sum(ms) / len(ms):.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}), "
              f"{int(cnt.sum())} intra MBs, err={int(enc.err.item())}", flush=True)
    enc.close()


if __name__ == "__main__":
    main()
