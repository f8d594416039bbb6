"""How much of the deblocking wavefront's work the boundary strengths switch off, on one batch of
the headline content (1080p, CRF 23, 60 frames): from the info words deblock_bs writes at every
coding step with P pictures, the slots that code one.

    python tools/diag/deblock_quiet.py [slots=16] [frames=60]

Reports, over all those pictures:
* the share of MBs with all 32 strengths zero;
* the share of (wave step, direction, edge) triples in which neither MB of the step has the edge
  on -- a wave filters MB (x, y) of an even row and MB (x - 2, y + 1) in one step, and runs an
  edge when either has it on;
* the share of wave steps with no horizontal edge on, with no vertical edge on, and with none.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from govideocompressor_amd.models.h264_gpu import GpuH264Encoder, H264Params, synth_clip  # noqa: E402


def step_bits(on):
    """on [hmb, wmb] (the info words' eight on bits) -> [pairs of rows, wmb + 2]: the bits of a wave step"""
    hmb, wmb = on.shape
    if hmb & 1:
        on = np.concatenate([on, np.zeros((1, wmb), on.dtype)])
    z = np.zeros((on.shape[0] // 2, 2), on.dtype)
    return np.concatenate([on[0::2], z], axis=1) | np.concatenate([z, on[1::2]], axis=1)


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    F = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    enc = GpuH264Encoder(H264Params(width=1920, height=1080, crf=23), slots=B)
    if enc.dbk_info is None:
        raise SystemExit("this kernel library has no deblock_bs")
    taken = []
    inner = enc._encode_step

    def spy(st, *a, **kw):
        inner(st, *a, **kw)
        p = np.flatnonzero(np.asarray(st["kinds"]) == 0)
        if p.size and st["deblock"]:
            taken.append(((enc.dbk_info[torch.from_numpy(p).to(enc.dbk_info.device)] >> 8) & 255).cpu().numpy())

    enc._encode_step = spy
    y, u, v = synth_clip(B, F, 1920, 1080, seed=0)
    enc.encode(y, u, v, metrics=False)
    torch.cuda.synchronize()
    on = np.concatenate(taken).reshape(-1, enc.hmb, enc.wmb).astype(np.uint8)
    steps = np.stack([step_bits(o) for o in on])
    edge_off = np.mean([((steps >> i) & 1) == 0 for i in range(8)])
    print(f"P pictures: {on.shape[0]} ({B} slots x {F} frames)")
    print(f"MBs with all 32 strengths zero:            {100 * np.mean(on == 0):.1f} %")
    print(f"(step, direction, edge) with the edge off: {100 * edge_off:.1f} %")
    print(f"wave steps with no horizontal edge on:     {100 * np.mean((steps >> 4) == 0):.1f} %")
    print(f"wave steps with no vertical edge on:       {100 * np.mean((steps & 15) == 0):.1f} %")
    print(f"wave steps with no edge on:                {100 * np.mean(steps == 0):.1f} %")
    enc.close()


if __name__ == "__main__":
    main()
