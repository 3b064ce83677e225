"""The mask-component cases shared by tests/test_components_cpu.py and tests/test_components_gpu.py: small u8 images {0,1}, each with a
name.  Every case but the two whose name starts with "tie_" is tie-free for the reference (largest and second-largest count unique),
so scipy, the reference's restatement (oracle.bilateral_ref.postprocess) and zutis_amd.components agree on it exactly; the noise seeds
are the first tie-free ones.  T = the tile edge of csrc/components.hip (ZH_CCL_TILE_H / _W of the header).

Plain helper module (no fixtures, no pytest hooks).
"""
import numpy as np

from zutis_amd import _lib

TH, TW = _lib.constants()["ZH_CCL_TILE_H"], _lib.constants()["ZH_CCL_TILE_W"]
NOISE_SEEDS = {(0.3, 37, 53): 0, (0.45, 37, 53): 0, (0.55, 37, 53): 0, (0.7, 37, 53): 0,
               (0.3, 65, 130): 0, (0.45, 65, 130): 0, (0.55, 65, 130): 0, (0.7, 65, 130): 0}


def _img(rows):
    return np.array(rows, dtype=np.uint8)


def serpentine(H, W):
    """One pixel wide: every even row, joined to the next one alternately at its right and its left end."""
    a = np.zeros((H, W), np.uint8)
    a[0::2] = 1
    for k, y in enumerate(range(1, H, 2)):
        a[y, W - 1 if k % 2 == 0 else 0] = 1
    return a


def spiral(H, W):
    """One pixel wide with one-pixel gaps, from the top-left corner inwards."""
    a = np.zeros((H, W), np.uint8)
    top, left, bottom, right = 0, 0, H - 1, W - 1
    y, x = 0, 0
    a[0, 0] = 1
    while True:
        moved = False
        for dy, dx, stop in ((0, 1, lambda: x >= right), (1, 0, lambda: y >= bottom), (0, -1, lambda: x <= left), (-1, 0, lambda: y <= top + 2)):
            while not stop():
                y, x = y + dy, x + dx
                a[y, x] = 1
                moved = True
            if (dy, dx) == (-1, 0):
                top, left, bottom, right = top + 2, left + 2, bottom - 2, right - 2
        if not moved or top > bottom or left > right:
            return a


def comb(H, W, teeth_to):
    """Teeth in every second column up to `teeth_to` that join only in the last row, and a lone pixel to their right."""
    a = np.zeros((H, W), np.uint8)
    a[:, 0:teeth_to:2] = 1
    a[H - 1, 0:teeth_to] = 1
    a[0, W - 2] = 1
    return a


def corner_blobs(H, W):
    """A rectangle with a one-pixel hole across every tile corner inside the image (areas all different), one at the image's top left
    and one in its bottom right corner (the last, partial tile)."""
    a = np.zeros((H, W), np.uint8)
    a[0:2, 0:3] = 1
    a[H - 3:H, W - 4:W] = 1
    k = 0
    for cy in range(TH, H, TH):
        for cx in range(TW, W, TW):
            a[max(cy - 2 - 3 * k, 0):cy + 2, max(cx - 3, 0):cx + 4 + 2 * k] = 1
            a[cy - 1, cx - 1] = 0
            k += 1
    return a


def noise(p, H, W, seed):
    return (np.random.default_rng(seed).random((H, W)) < p).astype(np.uint8)


def _ring_in_ring():
    a = np.zeros((15, 17), np.uint8)
    a[1:14, 1:16] = 1
    a[2:13, 2:15] = 0
    a[4:11, 4:13] = 1
    a[5:10, 5:12] = 0
    a[7, 8] = 1
    a[0, 16] = 1
    return a


def _cases():
    c = [("1x1_zero", _img([[0]])), ("1x1_one", _img([[1]])),
         ("1x7", _img([[1, 0, 1, 1, 0, 0, 1]])), ("7x1", _img([[1, 0, 1, 1, 0, 0, 1]]).T.copy()),
         ("all_zeros", np.zeros((5, 6), np.uint8)), ("all_ones", np.ones((5, 6), np.uint8))]
    big = np.zeros((8, 9), np.uint8)
    big[1:7, 1:8] = 1
    c.append(("blob_over_half", big))
    c.append(("plus", _img([[0, 1, 0], [1, 0, 1], [0, 1, 0]])))
    c.append(("ring_in_ring_island", _ring_in_ring()))
    open_hole = np.zeros((7, 8), np.uint8)
    open_hole[0:5, 1:6] = 1
    open_hole[0:4, 2:5] = 0                                   # a C open to the top border
    open_hole[6, 7] = 1
    c.append(("hole_open_to_border", open_hole))
    c.append(("diagonal_pocket", _img([[0, 1, 1, 0, 0], [1, 0, 1, 0, 0], [1, 1, 1, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 1]])))
    c.append(("serpentine", serpentine(2 * TH + 1, 2 * TW + 1)))
    c.append(("spiral", spiral(2 * TH + 1, 2 * TW + 1)))
    c.append(("comb_late_merge", comb(TH + 8, TW + 9, TW + 5)))
    yy, xx = np.mgrid[:9, :11]
    c.append(("checkerboard", ((yy + xx) % 2 == 0).astype(np.uint8)))
    grid = np.zeros((TH + 1, TW + 3), np.uint8)
    grid[0::2, 0::2] = 1
    grid[0, 1] = 1                                            # one component of three pixels: the second-largest count is unique
    c.append(("stride2_grid", grid))
    for h in (TH - 1, TH, TH + 1, 2 * TH + 1):
        for w in (TW - 1, TW, TW + 1, 2 * TW + 1):
            c.append((f"corner_blobs_{h}x{w}", corner_blobs(h, w)))
    for h, w in ((37, 53), (65, 130)):
        c.append((f"corner_blobs_{h}x{w}", corner_blobs(h, w)))
        for p in (0.3, 0.45, 0.55, 0.7):
            c.append((f"noise_p{p}_{h}x{w}_seed{NOISE_SEEDS[(p, h, w)]}", noise(p, h, w, NOISE_SEEDS[(p, h, w)])))
    c.append(("tie_largest", _img([[1, 1, 1, 0, 1, 1, 1]] * 3)))                      # counts [3, 9, 9]
    c.append(("tie_second_capacity", _img([[1, 0, 1, 0, 1, 0, 1, 0, 1]])))            # counts [4, 1, 1, 1, 1, 1]: (H*W + 1) / 2 components
    return c


CASES = _cases()
TIE_FREE = [(n, a) for n, a in CASES if not n.startswith("tie_")]
TIES = [(n, a) for n, a in CASES if n.startswith("tie_")]


def same_shape_triples():
    """[(names, u8 [3,H,W])]: every three cases of one shape next to each other in the list, for the batched runs."""
    by_shape = {}
    for n, a in CASES:
        by_shape.setdefault(a.shape, []).append((n, a))
    out = []
    for group in by_shape.values():
        if len(group) >= 3:
            for i in range(len(group) if len(group) > 3 else 1):
                tri = [group[(i + j) % len(group)] for j in range(3)]
                out.append((tuple(n for n, _ in tri), np.stack([a for _, a in tri])))
    return out


def working_size_case():
    """512 x 683 (the pseudo-label working size): an ellipse with 0.1 % of the pixels flipped."""
    H, W = 512, 683
    yy, xx = np.mgrid[:H, :W]
    a = (((yy - 250) / 150.0) ** 2 + ((xx - 340) / 220.0) ** 2 < 1.0)
    flip = np.random.default_rng(7).random((H, W)) < 0.001
    return (a ^ flip).astype(np.uint8)
