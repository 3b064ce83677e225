"""-m gpu: zh_polygon_runs (csrc/polygon.hip) through polygons.runs_device against polygons.runs_np and rle.from_polygons, count for
count, on the smallest shapes at which the walk, the filter, the sort or the union can go wrong, and coco_eval's device route of polygon
ground truth against its host route for equality of everything mask_ap returns."""
import numpy as np
import pytest

from tests import _cocoeval_case as CC
from tests import _polygon_case as PC
from zutis_amd import _lib, coco_eval, polygons, rle

pytestmark = pytest.mark.gpu


def check(dev, anns, host_fallback=0):
    got, stats = polygons.runs_device(anns, dev)
    want_np, want = polygons.runs_np(polygons.pack(anns)), PC.host_counts(anns)
    assert stats == {"annotations": len(anns), "polygons": sum(len(polygons._polys(p)) for p, _, _ in anns), "host_fallback": host_fallback}
    assert len(got) == len(anns)
    bad = [i for i, (g, n, r) in enumerate(zip(got, want_np, want))
           if g.dtype != np.int64 or not np.array_equal(g, r) or not np.array_equal(n, r)]
    assert not bad, (len(bad), anns[bad[0]], got[bad[0]], want_np[bad[0]], want[bad[0]])
    return got


def test_edge_cases(dev):
    """1 x 1, 1 x 7 and 7 x 1 images; polygons of 1, 2 and 3 vertices; zero-length edges; dx == dy; the four flip cases; a polygon
    outside the image and one covering it; crossings at 0 and at h * w; negative and half-integer coordinates; no polygon at all; the
    same polygon twice."""
    anns = PC.edge_cases()
    got = check(dev, anns)
    assert [g.tolist() for g, (p, h, w) in zip(got, anns) if (h, w) == (9, 11) and g.size == 1].count([99]) >= 4      # outside: [h * w]
    assert sum(1 for g, (p, h, w) in zip(got, anns) if g.tolist() == [0, h * w]) >= 5                                   # everything: [0, h * w]
    assert any(g[0] == 0 and g.size > 2 for g in got) and any(g.size > 1 and g.size % 2 == 0 and g[0] > 0 for g in got)  # crossings at 0; a run to h * w
    for p, h, w, mask in PC.hand_cases():
        assert np.array_equal(check(dev, [(p, h, w)])[0], rle._counts(mask))


def test_each_edge_case_alone(dev):
    """One annotation per call: nothing of a neighbour's state helps or hides."""
    for a in PC.edge_cases()[:24]:
        check(dev, [a])
    assert polygons.runs_device([], dev) == ([], {"annotations": 0, "polygons": 0, "host_fallback": 0})


def test_random_small_polygons(dev):
    check(dev, PC.random_singles(21, 2000))


def test_coco_like_polygons(dev):
    got = check(dev, PC.coco_like(22, 200))
    assert max(g.size for g in got) > 300                                   # hundreds of crossings in one sort


def test_unions(dev):
    check(dev, PC.random_multis(23, 300) + PC.coco_like(24, 12, 200, 260, (2, 3)))


def test_mixed_sizes_in_one_batch(dev):
    anns = PC.coco_like(25, 3) + PC.random_multis(26, 40) + PC.random_singles(27, 40) + PC.coco_like(28, 3, 100, 333, (1, 3)) + PC.edge_cases()
    rng = np.random.default_rng(29)
    check(dev, [anns[i] for i in rng.permutation(len(anns))])


def test_a_file_in_several_chunks(dev, monkeypatch):
    """More annotations than one launch takes: the chunks' results and counters join up (7 per chunk here, the last one short)."""
    monkeypatch.setattr(polygons, "CHUNK_ANNOTATIONS", 7)
    small = ([[1, 1, 4, 1, 4, 3, 1, 3]], 5, 6)
    anns = PC.random_multis(32, 12) + [PC.zigzag(polygons.LDS_CROSSINGS)] + PC.random_singles(33, 16) + [PC.zigzag(polygons.LDS_CROSSINGS), small]
    events = []
    check(dev, anns, host_fallback=2)
    polygons.runs_device(anns, dev, events=events)
    assert len(events) == 5 and len(anns) == 31


def test_over_capacity_goes_to_the_host_and_is_counted(dev):
    cap = _lib.load(raw=True).zh_polygon_lds_crossings()
    assert cap == polygons.LDS_CROSSINGS
    z = PC.zigzag(cap)
    assert len(rle._polygon_boundary(z[0][0], z[1], z[2])) > cap           # not only the bound: its crossings exceed the LDS sort
    small = ([[1, 1, 4, 1, 4, 3, 1, 3]], 5, 6)
    got = check(dev, [small, z, small], host_fallback=1)
    assert got[1].size > cap
    under = PC.zigzag(cap // 8)                                            # the same shape inside the capacity stays on the device
    assert check(dev, [under])[0].size > cap // 8


def test_to_rles_gives_from_polygons_dicts(dev):
    anns = PC.random_multis(30, 10) + PC.random_singles(31, 10)
    assert polygons.to_rles(anns, dev) == [rle.from_polygons(p, h, w) for p, h, w in anns]


def _mixed_file(seed=4):
    """8 images whose ground truth is polygons (one or several, in and out of the image), compressed RLE and a crowd RLE, mixed."""
    sizes, cats, g, d = CC.synthetic_corpus(seed=seed, n_images=8)
    ann, preds = CC.to_coco(sizes, cats, g, d)
    rng = np.random.default_rng(seed)
    n_poly = 0
    ann["annotations"][2]["iscrowd"] = 1                                    # a crowd, kept as RLE
    for j, a in enumerate(ann["annotations"]):
        if a["iscrowd"] or j % 3 == 2:
            continue                                                        # stays RLE
        h, w = sizes[a["image_id"]]
        ys, xs = np.nonzero(rle.decode(a["segmentation"]))
        y0, y1, x0, x1 = float(ys.min()), float(ys.max() + 1), float(xs.min()), float(xs.max() + 1)
        polys = [[x0, y0, x1 + .5, y0 - .25, x1, y1, (x0 + x1) / 2, y1 + 2.5, x0 - 1.5, (y0 + y1) / 2]]
        if j % 3 == 1:
            polys.append(PC.random_polygon(rng, h, w, 6))
        a["segmentation"] = polys
        a["area"] = float(rle.decode(rle.from_polygons(polys, h, w)).sum())
        n_poly += 1
    assert n_poly >= 4 and any(a["iscrowd"] for a in ann["annotations"]) and any(isinstance(a["segmentation"], dict) and not a["iscrowd"] for a in ann["annotations"])
    preds[0]["segmentation"] = [[2.0, 2.0, 30.5, 3.0, 20.0, 25.5]]        # a prediction may carry polygons too
    return ann, preds


@pytest.mark.parametrize("use_categories", [True, False])
def test_mask_ap_device_route_equals_host_route(dev, use_categories):
    ann, preds = _mixed_file()
    timings = {}
    d = coco_eval.mask_ap_route(ann, preds, polygons="device", use_categories=use_categories, device=dev, timings=timings)
    h = coco_eval.mask_ap_route(ann, preds, polygons="host", use_categories=use_categories, device=dev)
    m = coco_eval.mask_ap(ann, preds, use_categories=use_categories, device=dev)
    assert list(d) == list(h) == list(m)
    for k in ("stats", "precision", "recall"):
        assert np.array_equal(d[k], h[k]) and np.array_equal(m[k], h[k]) and d[k].dtype == h[k].dtype, k
    assert all(d[k] == h[k] for k in coco_eval.metric_names())
    assert d["AP"] > 0 and timings["stats"]["host_fallback"] == 0 and timings["stats"]["annotations"] >= 5
    assert [n for n, _, _ in timings["events"]] == ["zh_polygon_runs"]
