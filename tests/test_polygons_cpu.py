"""CPU: zutis_amd/polygons.py's host layers — pack (the flat arrays the kernel reads) and runs_np (the parallel statement of
rleFrPoly + union the kernel computes) — against rle.from_polygons / rle._polygon_boundary, count for count, and
coco_eval.prepare(polygon_counts=...) against prepare without it.  tests/test_polygons_gpu.py runs the kernel."""
import ctypes
import re

import numpy as np
import pytest

from tests import _cocoeval_case as CC
from tests import _polygon_case as PC
from zutis_amd import _lib, build, coco_eval, polygons, rle


def _reference_lists(xy):
    """The scaled vertices and the per-edge step counts as rle._polygon_boundary builds them (its first lines, restated)."""
    k = len(xy) // 2
    x = [int(5.0 * float(xy[2 * j]) + .5) for j in range(k)]
    y = [int(5.0 * float(xy[2 * j + 1]) + .5) for j in range(k)]
    steps = [max(abs(x[(j + 1) % k] - x[j]), abs(y[(j + 1) % k] - y[j])) + 1 for j in range(k)]
    return x, y, steps


def test_pack_scales_and_counts_steps_as_the_boundary_walk_does():
    anns = [([[-2.5, -0.1, 3.5, 7.5, 50.25, -7.75, 0.5, 0.3, -0.5, -0.7]], 6, 8),             # negatives, halves, beyond w / h
            ([[1.5, 2.5, 1.5, 2.5], [-0.09, -0.11, 100.0, 3.0, 7.1, 200.0]], 5, 9),
            ([0.1, 0.9, 2.3, 4.7, 6.5, -1.5], 7, 3)]                                              # one flat list
    pk = polygons.pack(anns)
    assert pk["poly_off"].tolist() == [0, 1, 3, 4] and pk["vert_off"].tolist() == [0, 5, 7, 10, 13]
    assert pk["hw"].tolist() == [[6, 8], [5, 9], [7, 3]]
    p = 0
    for polys, _, _ in anns:
        for xy in polygons._polys(polys):
            x, y, steps = _reference_lists(xy)
            lo, hi = pk["vert_off"][p], pk["vert_off"][p + 1]
            assert pk["xs"][lo:hi].tolist() == x and pk["ys"][lo:hi].tolist() == y and pk["steps"][lo:hi].tolist() == steps
            assert pk["step_pref"][lo + p:hi + p + 1].tolist() == np.concatenate(([0], np.cumsum(steps))).tolist()
            p += 1
    assert pk["xs"][0] == -12 and pk["xs"][4] == -2 and pk["ys"][4] == -3                        # truncation toward zero, not floor
    assert all(pk[k].dtype == np.int32 for k in ("xs", "ys", "steps", "step_pref", "vert_off", "poly_off", "hw", "out_off"))
    assert not pk["host"].any() and pk["out_off"].tolist() == np.concatenate(([0], np.cumsum([pk["bound"][0] + 1, pk["bound"][1:3].sum() + 1, pk["bound"][3] + 1]))).tolist()


def test_pack_marks_what_the_kernel_does_not_take():
    cap = polygons.LDS_CROSSINGS
    pk = polygons.pack([PC.zigzag(cap), ([[1, 1, 4, 1, 4, 3]], 5, 6), ([[1.0]], 5, 6), ([[1, 1, float("nan"), 2]], 5, 6),
                        ([[1, 1, 1e9, 2]], 5, 6), ([[1, 1, 2, 1e6]], 5, 6), ([[1, 1, 4, 1, 4, 3]], 0, 6)])
    assert pk["over_cap"].tolist() == [True] + [False] * 6
    assert pk["unsafe"].tolist() == [False, False, True, True, True, True, True]
    assert pk["host"].tolist() == [True, False, True, True, True, True, True]
    assert np.diff(pk["out_off"]).tolist() == [1, int(pk["bound"][1]) + 1, 1, 1, 1, 1, 1]
    with pytest.raises(ValueError, match="2\\^31"):
        polygons.pack([([[1, 1, 4, 1, 4, 3]], 1 << 16, 1 << 15)])
    assert polygons.pack([])["out_off"].tolist() == [0]


def test_capacity_bound_holds_the_crossings():
    anns = PC.random_singles(11, 2000)
    pk = polygons.pack(anns)
    true = np.asarray([len(rle._polygon_boundary(p[0], h, w)) for p, h, w in anns])
    ann, poly, pos = polygons.crossings_np(pk)
    assert np.array_equal(np.bincount(poly, minlength=len(anns)), true)                            # the parallel walk keeps the same crossings
    assert (pk["bound"] >= true).all() and true.max() > 20
    big = PC.coco_like(3, 20)
    assert (polygons.pack(big)["bound"] >= [len(rle._polygon_boundary(p[0], h, w)) for p, h, w in big]).all()


def test_crossings_equal_the_boundary_walk_as_multisets():
    anns = PC.random_singles(12, 300) + [a for a in PC.edge_cases() if len(polygons._polys(a[0])) == 1 and len(a[0][0]) >= 2]
    ann, poly, pos = polygons.crossings_np(polygons.pack(anns))
    for a, (p, h, w) in enumerate(anns):
        assert sorted(pos[ann == a].tolist()) == sorted(rle._polygon_boundary(polygons._polys(p)[0], h, w).tolist()), (p, h, w)


def _assert_equal(anns, got, want=None):
    want = PC.host_counts(anns) if want is None else want
    assert len(got) == len(want)
    bad = [i for i, (g, r) in enumerate(zip(got, want)) if g is None or g.dtype != np.int64 or not np.array_equal(g, r)]
    assert not bad, (len(bad), anns[bad[0]], got[bad[0]], want[bad[0]])


def test_runs_np_on_random_single_polygons():
    anns = PC.random_singles(1, 5000)
    got = polygons.runs_np(polygons.pack(anns))
    _assert_equal(anns, got)
    assert sum(1 for g in got if g[0] == 0 and len(g) > 1) > 100 and sum(1 for g in got if len(g) == 1) > 10       # leading empty runs; empty masks


def test_runs_np_on_unions():
    anns = PC.random_multis(2, 1000)
    _assert_equal(anns, polygons.runs_np(polygons.pack(anns)))


def test_runs_np_on_edge_and_hand_cases():
    anns = PC.edge_cases()
    got = polygons.runs_np(polygons.pack(anns))
    _assert_equal(anns, got)
    for p, h, w, mask in PC.hand_cases():
        c = polygons.runs_np(polygons.pack([(p, h, w)]))[0]
        assert np.array_equal(c, rle._counts(mask)) and np.array_equal(c, rle.counts_np(rle.from_polygons(p, h, w)["counts"]))
    assert polygons.runs_np(polygons.pack([([[20, 20, 30, 20, 30, 30]], 9, 11)]))[0].tolist() == [99]
    assert polygons.runs_np(polygons.pack([([[-1, -1, 12, -1, 12, 10, -1, 10]], 9, 11)]))[0].tolist() == [0, 99]
    z = PC.zigzag(300)
    _assert_equal([z], polygons.runs_np(polygons.pack([z])))


def test_runs_np_on_a_mixed_batch_of_sizes_and_a_coco_like_polygon():
    anns = PC.coco_like(5, 3) + PC.random_multis(6, 20) + PC.coco_like(7, 2, 300, 200, (2, 3)) + PC.random_singles(8, 20)
    _assert_equal(anns, polygons.runs_np(polygons.pack(anns)))


def test_prepare_takes_converted_polygons():
    sizes, cats, g, d = CC.synthetic_corpus(seed=3, n_images=2)
    ann, preds = CC.to_coco(sizes, cats, g, d)
    im = {i["id"]: i for i in ann["images"]}
    for j, a in enumerate(ann["annotations"]):
        if j % 2 == 0:
            h, w = im[a["image_id"]]["height"], im[a["image_id"]]["width"]
            a["segmentation"] = [[1.5 + j, 2.0, w - 2.25, 3.5, w / 2, h - 1.5], [0, 0, 4, 0, 4, 5]]
            a.pop("area", None)
    keys, items = coco_eval.polygon_segmentations(ann, preds)
    assert keys == [("annotation", j) for j in range(0, len(ann["annotations"]), 2)] and all(len(it[0]) == 2 for it in items)
    counts = polygons.runs_np(polygons.pack(items))
    a, b = coco_eval.prepare(ann, preds), coco_eval.prepare(ann, preds, polygon_counts=dict(zip(keys, counts)))
    assert len(a.masks) == len(b.masks) and a.mask_names == b.mask_names
    assert all(np.array_equal(x[0], y[0]) and x[0].dtype == y[0].dtype and x[1] == y[1] for x, y in zip(a.masks, b.masks))
    for ga, gb in zip(a.groups, b.groups):
        assert ga.gt_mask == gb.gt_mask and np.array_equal(ga.gt_ignore, gb.gt_ignore) and np.array_equal(ga.gt_order, gb.gt_order)
    keys_sub, _ = coco_eval.polygon_segmentations(ann, preds, image_ids=[ann["images"][0]["id"]])
    assert keys_sub and set(keys_sub) < set(keys)
    # a wrong array handed in is what prepare uses: the mapping is taken, not recomputed
    c = coco_eval.prepare(ann, preds, polygon_counts={keys[0]: np.asarray([3, 4, sizes[ann["annotations"][0]["image_id"]][0] * sizes[ann["annotations"][0]["image_id"]][1] - 7])})
    assert c.masks[[n for n in c.mask_names].index(f"annotation {ann['annotations'][0].get('id', 0)}")][0].tolist()[:2] == [3, 4]


def test_header_declares_the_polygon_entries():
    build.build(verbose=False)
    lib = _lib.load()
    vp, i = ctypes.c_void_p, ctypes.c_int
    e = _lib.entries()
    assert (e["zh_polygon_runs"].restype, e["zh_polygon_runs"].argtypes) == (i, [vp] * 8 + [i, vp, vp, vp]) and e["zh_polygon_runs"].plannable
    assert (e["zh_polygon_lds_crossings"].restype, e["zh_polygon_lds_crossings"].argtypes) == (i, [])
    assert _lib.header_abi_version() >= 236
    limit = _lib.constants()["ZH_POLYGON_LDS_CROSSINGS"]
    from zutis_amd import ops
    assert lib.zh_polygon_lds_crossings() == limit == polygons.LDS_CROSSINGS == ops.POLYGON_LDS_CROSSINGS == 4096   # the library was compiled with the header's value
    assert 4 * limit + 2 * limit + 4 * limit + 64 <= 64 * 1024                    # keys, coverage, boundaries: inside one workgroup's 64 KB
    assert lib.zh_polygon_runs(None, None, None, None, None, None, None, None, 0, None, None, None) == 0          # an empty call launches nothing
    assert lib.zh_polygon_runs(None, 16, 16, 16, 16, 16, 16, 16, 1, 16, 16, None) == -1 and b"null" in lib.zh_last_error()
    assert lib.zh_polygon_runs(16, 16, 16, 16, 16, 16, 16, 16, -1, 16, 16, None) == -1 and b"negative" in lib.zh_last_error()


def test_mask_ap_keeps_its_signature_and_the_route_is_spelled_out_beside_it():
    import inspect
    p = inspect.signature(coco_eval.mask_ap_route).parameters
    assert p["polygons"].default == "device" and p["polygons"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(coco_eval.prepare).parameters["polygon_counts"].default is None
    with pytest.raises(ValueError, match="device.*host"):
        coco_eval.mask_ap_route({}, [], polygons="gpu")
    assert not re.search(r"^(import|from) torch", open(polygons.__file__).read(), re.M)           # no torch import at module level
