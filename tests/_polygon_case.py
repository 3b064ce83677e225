"""Seeded polygon annotations [(polygons, h, w)] for tests/test_polygons_cpu.py and tests/test_polygons_gpu.py, and the host yardstick
(rle.from_polygons) of a list of them."""
import numpy as np

from zutis_amd import rle


def host_counts(annotations):
    return [rle.counts_np(rle.from_polygons(p, h, w)["counts"]) for p, h, w in annotations]


def random_polygon(rng, h, w, max_vertices=12):
    """1 .. max_vertices vertices with 0 - 2 decimals in [-5, side + 5]."""
    k = int(rng.integers(1, max_vertices + 1))
    dec = int(rng.integers(0, 3))
    xy = np.stack([rng.uniform(-5, w + 5, k), rng.uniform(-5, h + 5, k)], axis=1)
    return np.round(xy, dec).reshape(-1).tolist()


def random_singles(seed, n):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        h, w = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        out.append(([random_polygon(rng, h, w)], h, w))
    return out


def _rect(x0, y0, x1, y1):
    return [x0, y0, x1, y0, x1, y1, x0, y1]


def random_multis(seed, n):
    """Annotations of 2 - 4 polygons: disjoint, overlapping, one inside another, the same polygon twice, and free ones."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        h, w = int(rng.integers(4, 41)), int(rng.integers(4, 41))
        kind = i % 5
        if kind == 0:                                          # disjoint: left and right of a column
            c = float(rng.integers(1, w))
            polys = [_rect(float(rng.uniform(-2, c - 1)), float(rng.uniform(-2, h)), c - .5, float(rng.uniform(0, h + 2))),
                     _rect(c + .5, float(rng.uniform(-2, h)), float(rng.uniform(c + 1, w + 2)), float(rng.uniform(0, h + 2)))]
        elif kind == 1:                                        # overlapping
            polys = [random_polygon(rng, h, w, 6), random_polygon(rng, h, w, 6)]
            polys.append([v + 1.5 for v in polys[0]])
        elif kind == 2:                                        # one inside another
            polys = [_rect(0.0, 0.0, float(w), float(h)), _rect(w / 4, h / 4, w / 2, h / 2)]
            if rng.random() < .5:
                polys.append(random_polygon(rng, h, w))
        elif kind == 3:                                        # the same polygon twice (and once more, or not)
            p = random_polygon(rng, h, w)
            polys = [p, list(p)] + ([list(p)] if rng.random() < .5 else [])
        else:
            polys = [random_polygon(rng, h, w) for _ in range(int(rng.integers(2, 5)))]
        out.append((polys, h, w))
    return out


def star(rng, h, w):
    """A star-shaped polygon of 8 - 80 vertices and radius 10 - 120 px, as annotation files hold them."""
    k = int(rng.integers(8, 81))
    r = float(rng.uniform(10, 120))
    cx, cy = float(rng.uniform(0, w)), float(rng.uniform(0, h))
    ang = np.sort(rng.uniform(0, 2 * np.pi, k))
    rad = r * rng.uniform(.6, 1.0, k)
    return np.round(np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1), 2).reshape(-1).tolist()


def coco_like(seed, n, h=480, w=640, polys=(1, 1)):
    rng = np.random.default_rng(seed)
    return [([star(rng, h, w) for _ in range(int(rng.integers(polys[0], polys[1] + 1)))], h, w) for _ in range(n)]


# tests/test_coco_eval_cpu.py::test_from_polygons_by_hand, restated: (polygons, h, w, the pixels set as (y0, x0, y1, x1) boxes or a mask)
def hand_cases():
    def box(h, w, y0, x0, y1, x1):
        m = np.zeros((h, w), bool)
        m[y0:y1, x0:x1] = True
        return m
    tri = np.array([[c + r < 5 for c in range(6)] for r in range(6)])
    return [([[1, 1, 4, 1, 4, 3, 1, 3]], 5, 6, box(5, 6, 1, 1, 3, 4)),
            ([1.0, 1.0, 4.0, 1.0, 4.0, 3.0, 1.0, 3.0], 5, 6, box(5, 6, 1, 1, 3, 4)),
            ([[0, 0, 6, 0, 6, 5, 0, 5]], 5, 6, np.ones((5, 6), bool)),
            ([[0, 0, 6, 0, 0, 6]], 6, 6, tri),
            ([[-2, 1, 4, 1, 4, 9, -2, 9]], 5, 6, box(5, 6, 1, 0, 5, 4)),
            ([[0, 0, 3, 0, 3, 3, 0, 3], [2, 2, 5, 2, 5, 4, 2, 4]], 5, 6, box(5, 6, 0, 0, 3, 3) | box(5, 6, 2, 2, 4, 5))]


def edge_cases():
    """The smallest shapes at which the walk, the filter, the sort or the union can go wrong (tests/test_polygons_gpu.py lists them)."""
    full = lambda h, w: _rect(-1.0, -1.0, w + 1.0, h + 1.0)
    cases = []
    for h, w in ((1, 1), (1, 7), (7, 1)):
        cases += [([full(h, w)], h, w), ([[0, 0, w, 0, w, h, 0, h]], h, w), ([[0.4, 0.4, 0.6, 0.4, 0.6, 0.6]], h, w),
                  ([[0, 0, w, h]], h, w), ([[0.5, 0.5]], h, w), ([[-3, -3, -1, -3, -1, -1]], h, w)]
    h, w = 9, 11
    cases += [([[2.0, 3.0]], h, w), ([[2.0, 3.0, 8.0, 6.0]], h, w), ([[2.0, 3.0, 8.0, 6.0, 4.0, 8.0]], h, w),          # 1, 2, 3 vertices
              ([[2, 2, 2, 2, 8, 2, 8, 2, 8, 7, 8, 7, 2, 7]], h, w), ([[3, 3, 3, 3, 3, 3]], h, w),                   # zero-length edges
              ([[1, 1, 6, 6, 1, 6]], h, w), ([[6, 6, 1, 1, 6, 1]], h, w), ([[1, 6, 6, 1, 6, 6]], h, w),             # dx == dy, both ways
              ([[1, 1, 9, 3, 2, 8]], h, w), ([[9, 3, 1, 1, 2, 8]], h, w), ([[1, 1, 3, 8, 9, 2]], h, w),             # the four flip cases:
              ([[3, 8, 1, 1, 9, 2]], h, w), ([[5, 1, 9, 5, 5, 8, 1, 5]], h, w), ([[5, 8, 9, 5, 5, 1, 1, 5]], h, w),  # either order, either axis
              ([[20, 20, 30, 20, 30, 30]], h, w), ([[-9, -9, -2, -9, -2, -2]], h, w), ([[2, 20, 8, 20, 8, 30]], h, w),    # outside: [h * w]
              ([full(h, w)], h, w), ([[0, 0, w, 0, w, h, 0, h]], h, w),                                                # everything: [0, h * w]
              ([[0, 0, 3, 0, 3, 2, 0, 2]], h, w), ([[8, 5, 11, 5, 11, 9, 8, 9]], h, w), ([[8, 5, 14, 5, 14, 12, 8, 12]], h, w),  # 0 and h * w
              ([[-2.5, -1.5, 6.5, 2.5, 3.5, 12.5]], h, w), ([[0.5, 0.5, 10.5, 0.5, 10.5, 8.5, 0.5, 8.5]], h, w),   # negative, halves
              ([[-0.1, -0.1, 4.25, -0.3, 4.75, 5.5, -0.7, 3.3]], h, w), ([], h, w),
              ([[1, 1, 4, 1, 4, 4, 1, 4], [1, 1, 4, 1, 4, 4, 1, 4]], h, w), ([full(h, w), [2, 2, 5, 2, 5, 5]], h, w),
              ([[20, 20, 30, 20, 30, 30], [-9, -9, -2, -9, -2, -2]], h, w)]
    return cases


def zigzag(teeth, h=8):
    """One polygon whose boundary crosses about 2 * `teeth` column centres: a saw of one-pixel teeth over a wide image, closed below."""
    w = teeth + 4
    top = [v for c in range(teeth) for v in (c + .5, (1.0 if c & 1 else 6.0))]
    return ([[0.5, 7.0] + top + [teeth - .5, 7.0]], h, w)
