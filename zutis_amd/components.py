"""Mask components: the definition, in NumPy, of what zh_second_largest_component computes on the device.

The last four lines of the reference's bilateral_solver_output (utils/bilateral_solver.py:185-193) are

    binary = ndimage.binary_fill_holes(soft > 0.5);  labeled, nr = ndimage.label(binary)
    counts = [np.sum(labeled == i) for i in range(nr + 1)];  mask = labeled == np.argsort(counts)[-2]      # all True without an object

restated here from the public definitions of those operations, without scipy:

  fill holes  a background pixel becomes foreground unless it is 4-connected, through background pixels, to a pixel on the image border.
  label       the 4-connected foreground components are numbered 1 .. nr in raster order of each component's first pixel (its smallest
              linear index y * W + x); 0 is background.
  counts      counts[i] = number of pixels with label i, i = 0 .. nr.  Label 0 is a candidate like any other: when the filled foreground
              is larger than the background, the background is what gets selected (and a full image selects nothing: counts [0, H*W]).
  select      nr = 0: the mask is all ones.  Otherwise the chosen label is the SECOND LARGEST UNDER THE KEY (count, label):
              np.argsort(counts, kind="stable")[-2].

Ties.  The reference's plain np.argsort is an unstable sort: among equal counts the order it returns is whatever its introsort leaves
(with NumPy 2.2 it already differs from the stable order on five elements), so the reference's answer is implementation-defined exactly
when the largest or the second-largest count is not unique.  The stable rule above is the one kept, on the host and on the device;
everywhere else the two agree bit for bit (tests/test_components_cpu.py, tests/test_components_gpu.py).
"""
from __future__ import annotations

from typing import Tuple

import numpy as np


def _foreground(x, threshold: float = 0.5) -> np.ndarray:
    """bool [H,W]: x > threshold for a float image (a NaN is background), x != 0 for an integer or bool one."""
    x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError(f"components: a 2-D image is needed, got shape {x.shape}")
    return x > threshold if x.dtype.kind == "f" else x != 0


def label_np(foreground) -> Tuple[np.ndarray, int]:
    """(int32 labels [H,W], nr) of the 4-connected components of `foreground` (non-zero = foreground), numbered as scipy.ndimage.label
    numbers them.  Runs of each row are joined with the overlapping runs of the row above in a union-find forest whose roots are the
    smallest run index — runs are in raster order, so a component's root is the run that holds its first pixel."""
    fg = np.asarray(foreground) != 0
    H, W = fg.shape
    edges = np.diff(np.pad(fg.astype(np.int8), ((0, 0), (1, 1))), axis=1)           # [H, W + 1]: +1 where a run starts, -1 behind its end
    ys, xs = np.nonzero(edges == 1)
    _, xe = np.nonzero(edges == -1)                                                 # the same order: one end per start, row by row
    n = len(ys)
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    row = np.searchsorted(ys, np.arange(H + 1))
    s, e = xs.tolist(), xe.tolist()
    for y in range(1, H):
        a, a1, b, b1 = int(row[y - 1]), int(row[y]), int(row[y]), int(row[y + 1])
        while a < a1 and b < b1:
            if s[a] < e[b] and s[b] < e[a]:                                         # the two runs share a column
                ra, rb = find(a), find(b)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
            if e[a] <= e[b]:
                a += 1
            else:
                b += 1
    roots = np.fromiter((find(i) for i in range(n)), dtype=np.int64, count=n)
    is_root = roots == np.arange(n)
    number = np.cumsum(is_root)                                                     # 1-based number of each root
    run_label = number[roots] if n else np.zeros(0, np.int64)
    paint = np.zeros((H, W + 1), dtype=np.int64)
    np.add.at(paint, (ys, xs), run_label)
    np.add.at(paint, (ys, xe), -run_label)
    return np.cumsum(paint, axis=1)[:, :W].astype(np.int32), int(is_root.sum())


def fill_holes_np(foreground) -> np.ndarray:
    """bool [H,W]: `foreground` with its holes filled, as scipy.ndimage.binary_fill_holes fills them."""
    fg = np.asarray(foreground) != 0
    bg_labels, nr = label_np(~fg)
    is_open = np.zeros(nr + 1, dtype=bool)
    for edge in (bg_labels[0], bg_labels[-1], bg_labels[:, 0], bg_labels[:, -1]):
        is_open[edge] = True
    is_open[0] = True                                                               # label 0 of the background's labels is the foreground
    return fg | ~is_open[bg_labels]


def select_np(labels: np.ndarray, nr: int) -> Tuple[np.ndarray, np.ndarray]:
    """(bool mask [H,W], int32 stats [4] = {nr, chosen label, chosen count, fallback}) — the stable rule of the module docstring.  In the
    fallback (nr = 0) the mask is all ones, the label -1 and the count H * W."""
    labels = np.asarray(labels)
    if nr == 0:
        return np.ones(labels.shape, dtype=bool), np.array([0, -1, labels.size, 1], dtype=np.int32)
    counts = np.bincount(labels.reshape(-1), minlength=nr + 1)
    chosen = int(np.argsort(counts, kind="stable")[-2])
    return labels == chosen, np.array([nr, chosen, counts[chosen], 0], dtype=np.int32)


def components_np(x, threshold: float = 0.5):
    """Every output of the device entry for one image: (mask bool, filled bool, labels int32, stats int32 [4])."""
    filled = fill_holes_np(_foreground(x, threshold))
    labels, nr = label_np(filled)
    mask, stats = select_np(labels, nr)
    return mask, filled, labels, stats


def postprocess_np(x, threshold: float = 0.5) -> np.ndarray:
    """bilateral_solver.py:185-193 under the stable tie rule: x float [H,W] (foreground = x > threshold) or an integer / bool mask
    (non-zero) -> bool [H,W]."""
    return components_np(x, threshold)[0]


def has_tie(x, threshold: float = 0.5) -> bool:
    """True when the largest or the second-largest count is not unique: the inputs on which the reference's unstable argsort may
    choose another label than the stable rule."""
    _, _, labels, stats = components_np(x, threshold)
    if stats[3]:
        return False
    c = np.sort(np.bincount(labels.reshape(-1), minlength=int(stats[0]) + 1))
    return bool(c[-1] == c[-2] or (len(c) > 2 and c[-2] == c[-3]))
