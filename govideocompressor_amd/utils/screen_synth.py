"""Screen-like synthetic content (text, UI, line art) for tests and rate-distortion runs.

``screen_clip`` draws, per slot, a canvas of flat and gradient panels with glyph-like marks (small
rectangles of one ink per panel, laid out in text lines with word gaps) and 1-sample horizontal
and vertical rules, and scrolls it by whole samples per frame (an even number of luma samples, so
the 4:2:0 chroma planes scroll by whole samples too).  About a quarter of the panels of the frame
are overlays that do not scroll: their marks stay in place over the moving background, and in
every picture some of their glyph cells show another glyph (a clock, a cursor).  Luma and chroma
both carry the marks: a stroke one or two luma samples wide is single-sample detail in a chroma
4x4 block.  Seeded and
device-independent (the layout comes from numpy's generator, the drawing is torch on the CPU);
renders 8 bits (uint8) or 10 bits (int16), the same picture at either depth.

The content kinds of csrc/kernels/synth.hip (``CONTENT_KINDS``) are untouched; this generator is a
class of its own (``--kinds screen`` in tools/content_rd.py).
"""
from __future__ import annotations

import numpy as np
import torch

CELL = 8          # glyph cell (luma samples)
PANEL = 64        # panel size (luma samples)
NGLYPHS = 48      # glyph shapes per slot


def _glyphs(rng) -> np.ndarray:
    """[NGLYPHS, CELL, CELL] bool: two to four strokes (1 - 2 samples wide) inside a 6 x 7 box"""
    g = np.zeros((NGLYPHS, CELL, CELL), dtype=bool)
    for k in range(NGLYPHS):
        for _ in range(int(rng.integers(2, 5))):
            w = int(rng.integers(1, 3))
            if rng.random() < 0.5:   # vertical stroke
                x, y0, y1 = int(rng.integers(0, 7 - w)), int(rng.integers(0, 3)), int(rng.integers(4, 8))
                g[k, y0:y1, x:x + w] = True
            else:                    # horizontal stroke
                y, x0, x1 = int(rng.integers(0, 8 - w)), int(rng.integers(0, 2)), int(rng.integers(3, 7))
                g[k, y:y + w, x0:x1] = True
    return g


def _canvas(rng, hc: int, wc: int, plain: bool):
    """8-bit-scale float canvases (y [hc, wc], u and v [hc / 2, wc / 2]) of one slot"""
    ph, pw = -(-hc // PANEL), -(-wc // PANEL)
    yy, xx = np.mgrid[0:ph * PANEL, 0:pw * PANEL]
    py, px = yy // PANEL, xx // PANEL
    # panels: flat or a ramp of up to +-40 levels across the panel, each with its own ink
    base = rng.integers(40, 216, (ph, pw)).astype(np.float64)
    ramp = np.where(rng.random((ph, pw)) < (1.0 if plain else 0.4), rng.uniform(-40, 40, (ph, pw)), 0.0)
    horiz = rng.random((ph, pw)) < 0.5
    t = np.where(horiz[py, px], (xx % PANEL) / PANEL, (yy % PANEL) / PANEL) - 0.5
    y = base[py, px] + ramp[py, px] * t
    cu, cv = rng.integers(96, 160, (ph, pw)).astype(np.float64), rng.integers(96, 160, (ph, pw)).astype(np.float64)
    u, v = cu[py, px], cv[py, px]
    if not plain:
        ink = np.where(base > 128, base - rng.integers(60, 121, (ph, pw)), base + rng.integers(60, 121, (ph, pw)))
        iu, iv = rng.integers(32, 224, (ph, pw)).astype(np.float64), rng.integers(32, 224, (ph, pw)).astype(np.float64)
        # text: glyph cells on every other cell row, words of 2 - 9 glyphs with gaps, some panels empty
        gh, gw = ph * PANEL // CELL, pw * PANEL // CELL
        idx = rng.integers(0, NGLYPHS, (gh, gw))
        on = (rng.random((gh, gw)) < 0.8) & ((np.arange(gh) % 2 == 0)[:, None])
        gap = np.zeros((gh, gw), dtype=bool)
        for r in range(0, gh, 2):
            c = 0
            while c < gw:
                c += int(rng.integers(2, 10))
                gap[r, c:c + 1] = True
                c += 1
        textp = rng.random((ph, pw)) < 0.7
        on &= ~gap & textp[np.arange(gh)[:, None] * CELL // PANEL, np.arange(gw)[None, :] * CELL // PANEL]
        lib = _glyphs(rng)
        mask = (lib[idx] & on[:, :, None, None]).transpose(0, 2, 1, 3).reshape(gh * CELL, gw * CELL)
        # 1-sample rules: a few horizontal and vertical lines per panel row / column
        for _ in range(max(1, ph * pw // 2)):
            p, q = int(rng.integers(0, ph)), int(rng.integers(0, pw))
            o = int(rng.integers(0, PANEL))
            if rng.random() < 0.5:
                mask[p * PANEL + o, q * PANEL:(q + 1) * PANEL] = True
            else:
                mask[p * PANEL:(p + 1) * PANEL, q * PANEL + o] = True
        y = np.where(mask, ink[py, px], y)
        u = np.where(mask, iu[py, px], u)
        v = np.where(mask, iv[py, px], v)
    return y[:hc, :wc], u[:hc:2, :wc:2], v[:hc:2, :wc:2]


def _overlay(rng, frames: int, height: int, width: int):
    """static overlay panels in frame coordinates: per frame a mark mask [frames, H, W] (glyph rows
    whose cells change with probability 0.15 per picture), and one ink (y, u, v) per slot"""
    ph, pw = -(-height // PANEL), -(-width // PANEL)
    panel = rng.random((ph, pw)) < 0.25
    gh, gw = ph * PANEL // CELL, pw * PANEL // CELL
    lib = _glyphs(rng)
    idx = rng.integers(0, NGLYPHS, (gh, gw))
    on = (rng.random((gh, gw)) < 0.7) & ((np.arange(gh) % 2 == 1)[:, None])
    on &= panel[np.arange(gh)[:, None] * CELL // PANEL, np.arange(gw)[None, :] * CELL // PANEL]
    masks = []
    for _ in range(frames):
        change = rng.random((gh, gw)) < 0.15
        idx = np.where(change, rng.integers(0, NGLYPHS, (gh, gw)), idx)
        m = (lib[idx] & on[:, :, None, None]).transpose(0, 2, 1, 3).reshape(gh * CELL, gw * CELL)
        masks.append(m[:height, :width])
    ink = (float(rng.integers(0, 2)) * 215.0 + 20.0, float(rng.integers(32, 224)), float(rng.integers(32, 224)))
    return np.stack(masks), ink


def screen_clip(slots: int, frames: int, width: int, height: int, seed: int = 0, device="cuda", bit_depth: int = 8,
                plain_slots=()):
    """B x F I420 frames [slots, frames, H, W] (+ half-size chroma) of scrolling screen content;
    uint8 at 8 bits, int16 (0 .. 1023) at 10.  ``plain_slots``: slots that show panels only
    (flat and gradient, no marks, no rules): smooth content of the same make."""
    if bit_depth not in (8, 10):
        raise ValueError("screen_clip: bit_depth must be 8 or 10")
    if width % 2 or height % 2:
        raise ValueError("screen_clip: width and height must be even")
    k = 1 << (bit_depth - 8)
    dt = torch.uint8 if bit_depth == 8 else torch.int16
    ys, us, vs = [], [], []
    for b in range(slots):
        rng = np.random.default_rng([int(seed) & 0xFFFFFFFF, b])
        dx, dy = 2 * int(rng.integers(0, 2)), 2 * int(rng.integers(1, 4))   # whole (even) samples per frame
        hc, wc = height + dy * frames, width + dx * frames
        planes = _canvas(rng, hc, wc, b in plain_slots)
        # the same picture at either depth: 8-bit-scale values times 2^(bd - 8), rounded once
        cy, cu, cv = (torch.from_numpy(np.clip(np.rint(p * k), 0, 256 * k - 1).astype(np.int16)) for p in planes)
        fy = torch.stack([cy[t * dy:t * dy + height, t * dx:t * dx + width] for t in range(frames)])
        fu = torch.stack([cu[t * dy // 2:(t * dy + height) // 2, t * dx // 2:(t * dx + width) // 2] for t in range(frames)])
        fv = torch.stack([cv[t * dy // 2:(t * dy + height) // 2, t * dx // 2:(t * dx + width) // 2] for t in range(frames)])
        if b not in plain_slots:
            masks, ink = _overlay(rng, frames, height, width)
            m = torch.from_numpy(masks)
            fy = torch.where(m, torch.tensor(int(round(ink[0] * k)), dtype=torch.int16), fy)
            mc = m[:, ::2, ::2]
            fu = torch.where(mc, torch.tensor(int(round(ink[1] * k)), dtype=torch.int16), fu)
            fv = torch.where(mc, torch.tensor(int(round(ink[2] * k)), dtype=torch.int16), fv)
        ys.append(fy)
        us.append(fu)
        vs.append(fv)
    return tuple(torch.stack(p).to(dt).contiguous().to(device) for p in (ys, us, vs))
