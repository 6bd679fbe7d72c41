"""NumPy / plain-Python restatement of the post-filters of the dense stereo matcher (rules 9 and 10
of thor_slam_amd/stereo_depth.py), written from the rules alone: the median by sorting the window's
values, the speckle filter by flood fill.  Nothing is shared with the device code, and the product
does not import this.  The device output must equal it bit for bit
(tests/test_gpu_stereo_filter.py)."""

from __future__ import annotations

import numpy as np

from ref_stereo_depth import depth_from_disp32

_BIG = np.int64(1) << 40


def median(disp32: np.ndarray, m: int) -> np.ndarray:
    """Rule 9: the lower median of the non-zero values of the clamped m x m window at every
    non-zero pixel; m = 0 returns the input."""
    d = np.asarray(disp32).astype(np.int64)
    if m == 0:
        return d.astype(np.uint16)
    assert m in (3, 5, 7)
    r = m // 2
    H, W = d.shape
    pad = np.pad(d, r, mode="edge")                         # clamped coordinates, duplicates counted
    win = np.stack([pad[j:j + H, i:i + W] for j in range(m) for i in range(m)], axis=-1)
    n = (win != 0).sum(-1)
    ordered = np.sort(np.where(win != 0, win, _BIG), axis=-1)   # v_0 <= ... <= v_(n-1), then the zeros' places
    k = np.maximum(n - 1, 0) // 2
    out = np.take_along_axis(ordered, k[..., None], -1)[..., 0]
    return np.where(d != 0, out, 0).astype(np.uint16)


def components(disp32: np.ndarray, r: int) -> tuple[np.ndarray, list[int]]:
    """Rule 10's partition: (label [H][W], -1 where disp32 = 0, else the component's number;
    the components' sizes)."""
    d = np.asarray(disp32).astype(np.int64)
    H, W = d.shape
    vals = d.tolist()
    label = [[-1] * W for _ in range(H)]
    sizes: list[int] = []
    for y0 in range(H):
        for x0 in range(W):
            if vals[y0][x0] == 0 or label[y0][x0] >= 0:
                continue
            c = len(sizes)
            label[y0][x0] = c
            stack = [(y0, x0)]
            size = 0
            while stack:
                y, x = stack.pop()
                size += 1
                a = vals[y][x]
                for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                    if 0 <= yy < H and 0 <= xx < W and label[yy][xx] < 0:
                        b = vals[yy][xx]
                        if b != 0 and abs(a - b) <= r:
                            label[yy][xx] = c
                            stack.append((yy, xx))
            sizes.append(size)
    return np.array(label, np.int64).reshape(H, W), sizes


def speckle(disp32: np.ndarray, size: int, rng: int) -> np.ndarray:
    """Rule 10: every pixel of a component with at most `size` pixels becomes 0; size 0 = off."""
    d = np.asarray(disp32).astype(np.uint16)
    if size == 0:
        return d
    label, sizes = components(d, rng)
    small = np.array(sizes + [0], np.int64) <= size          # the last entry serves label -1
    return np.where((label >= 0) & small[label], 0, d).astype(np.uint16)


def filter_disp32(disp32: np.ndarray, m: int = 0, size: int = 0, rng: int = 32) -> np.ndarray:
    """Rule 9, then rule 10."""
    return speckle(median(disp32, m), size, rng)


def filtered(disp32: np.ndarray, fxb: float, m: int = 0, size: int = 0, rng: int = 32):
    """(depth u16 mm, disp32 u16) after the filters: rule 8 from the filtered disp32."""
    out = filter_disp32(disp32, m, size, rng)
    return depth_from_disp32(out, fxb), out
