"""Instance predictions as pictures, the parts that need no GPU: paint_reference (the NumPy statement of zh_instance_paint, the oracle of
the GPU tests) against literal cases small enough to check by eye, the colour table, and the validation of predict_from_files' instance_*
arguments, which comes before any device work."""
import inspect
import os

import numpy as np
import pytest
import torch

from zutis_amd import _lib, instance_paint as IP, predict_files as PF

# one image colour and three instance colours; b* = (image * 128 + colour * 128 + 128) >> 8, worked out by hand
I = (200, 100, 0)
C0, C1, C2 = (0, 0, 255), (255, 0, 0), (0, 255, 0)
b0 = (100, 50, 128)         # (25600 + 0 + 128) >> 8, (12800 + 0 + 128) >> 8, (0 + 32640 + 128) >> 8
b1 = (228, 50, 0)           # (25600 + 32640 + 128) >> 8 = 58368 >> 8
b2 = (100, 178, 0)          # (12800 + 32640 + 128) >> 8 = 45568 >> 8


def _grid(rows):
    return np.array(rows, dtype=np.uint8)


def _three_masks():
    """4 x 5: slot 0 (score 0.5) the left 4 x 3 block; slot 1 (0.9) rows 1-2 of the right three columns — it overlaps slot 0 in column 2;
    slot 2 (0.5, ties slot 0) row 3, columns 1-3 — it overlaps slot 0 in columns 1-2."""
    m = np.zeros((3, 4, 5), np.uint8)
    m[0, :, 0:3] = 1
    m[1, 1:3, 2:5] = 1
    m[2, 3, 1:4] = 1
    return np.full((4, 5, 3), I, np.uint8), m, [0.5, 0.9, 0.5], _grid([C0, C1, C2])


def test_overlap_by_score_tie_by_slot_and_the_two_kinds_of_outline():
    image, masks, scores, colours = _three_masks()
    ids, overlay = IP.paint_reference(image, masks, scores, colours, alpha=128, outline=True, min_score=0.0)
    assert ids.dtype == np.int64 and overlay.dtype == np.uint8
    assert ids.tolist() == [[1, 1, 1, 0, 0],
                            [1, 1, 2, 2, 2],        # column 2: slot 1 (0.9) over slot 0 (0.5)
                            [1, 1, 2, 2, 2],
                            [1, 1, 1, 3, 0]]        # columns 1-2: slots 0 and 2 tie at 0.5, the lower slot wins
    # (0,0), (1,0), (2,0), (3,0), (0,1), (3,1): at the image border, every neighbour inside has the same id -> blended, not outlined
    # (0,2), (3,3)...: a neighbour with no id; (1,1), (2,1), (3,2): a neighbour of another instance -> the pure colour
    assert overlay.tolist() == _grid([[b0, b0, C0, I, I],
                                      [b0, C0, C1, C1, C1],
                                      [b0, C0, C1, C1, C1],
                                      [b0, b0, C0, C2, I]]).tolist()


def test_a_mask_over_the_whole_image_has_no_outline():
    image = _grid([[(0, 0, 0), (255, 255, 255)], [(10, 20, 30), (40, 50, 60)]])
    ids, overlay = IP.paint_reference(image, np.ones((1, 2, 2), np.uint8), [1.0], _grid([(255, 0, 128)]), alpha=64, outline=True)
    assert ids.tolist() == [[1, 1], [1, 1]]
    # (v * 192 + c * 64 + 128) >> 8 with c = (255, 0, 128)
    assert overlay.tolist() == [[[64, 0, 32], [255, 191, 223]], [[71, 15, 55], [94, 38, 77]]]


def test_a_row_of_three_with_one_pixel_painted():
    image = _grid([[(1, 2, 3), (100, 150, 200), (7, 8, 9)]])
    masks = np.array([[[0, 7, 0]]], np.uint8)                    # any non-zero byte is in the mask
    ids, overlay = IP.paint_reference(image, masks, [0.3], _grid([(0, 255, 0)]), alpha=128, outline=False)
    assert ids.tolist() == [[0, 1, 0]]
    assert overlay.tolist() == [[[1, 2, 3], [50, 203, 100], [7, 8, 9]]]   # (12800 + 128) >> 8, (19200 + 32640 + 128) >> 8, (25600 + 128) >> 8
    _, outlined = IP.paint_reference(image, masks, [0.3], _grid([(0, 255, 0)]), alpha=128, outline=True)
    assert outlined.tolist() == [[[1, 2, 3], [0, 255, 0], [7, 8, 9]]]     # both neighbours have no id; they themselves are never outlined


def test_alpha_0_is_the_image_off_the_outlines_and_alpha_256_the_pure_colour():
    image, masks, scores, colours = _three_masks()
    _, overlay = IP.paint_reference(image, masks, scores, colours, alpha=0, outline=True)
    assert overlay.tolist() == _grid([[I, I, C0, I, I], [I, C0, C1, C1, C1], [I, C0, C1, C1, C1], [I, I, C0, C2, I]]).tolist()
    for outline in (True, False):
        _, overlay = IP.paint_reference(image, masks, scores, colours, alpha=256, outline=outline)
        assert overlay.tolist() == _grid([[C0, C0, C0, I, I], [C0, C0, C1, C1, C1], [C0, C0, C1, C1, C1], [C0, C0, C0, C2, I]]).tolist()
    for alpha in (-1, 257, 0.5):
        with pytest.raises(ValueError, match="alpha"):
            IP.paint_reference(image, masks, scores, colours, alpha=alpha)


def test_without_outline_every_painted_pixel_is_the_blend():
    image, masks, scores, colours = _three_masks()
    _, overlay = IP.paint_reference(image, masks, scores, colours, alpha=128, outline=False)
    assert overlay.tolist() == _grid([[b0, b0, b0, I, I], [b0, b0, b1, b1, b1], [b0, b0, b1, b1, b1], [b0, b0, b0, b2, I]]).tolist()
    rng = np.random.default_rng(0)
    image = rng.integers(0, 256, (6, 7, 3), dtype=np.uint8)
    masks = (rng.random((4, 6, 7)) < 0.4).astype(np.uint8)
    colours = rng.integers(0, 256, (4, 3), dtype=np.uint8)
    ids, overlay = IP.paint_reference(image, masks, [0.1, 0.2, 0.3, 0.4], colours, alpha=77, outline=False)
    want = np.where((ids > 0)[..., None], PF.blend(image, colours[np.maximum(ids, 1) - 1], 77), image)
    assert np.array_equal(overlay, want)


def test_min_score_is_strict():
    image, masks, scores, colours = _three_masks()
    ids, overlay = IP.paint_reference(image, masks, scores, colours, min_score=0.5)           # the two slots AT 0.5 are not painted
    assert ids.tolist() == [[0, 0, 0, 0, 0], [0, 0, 2, 2, 2], [0, 0, 2, 2, 2], [0, 0, 0, 0, 0]]
    assert overlay.tolist() == _grid([[I] * 5, [I, I, C1, C1, C1], [I, I, C1, C1, C1], [I] * 5]).tolist()
    ids, _ = IP.paint_reference(image, masks, scores, colours, min_score=np.nextafter(0.5, 0.0))
    assert (ids == 1).any() and (ids == 3).any()
    ids, overlay = IP.paint_reference(image, masks, scores, colours, min_score=0.9)
    assert not ids.any() and np.array_equal(overlay, image)
    assert IP.paint_order([0.5, np.nan, 0.9, 0.5, -1.0], 0.0) == [2, 0, 3]                    # a NaN score is never painted


def test_the_colour_table():
    c = IP.instance_colours(100)
    assert c.shape == (100, 3) and c.dtype == np.uint8 and c.flags.c_contiguous
    assert c[:8].tolist() == [[255, 25, 25], [20, 210, 74], [100, 16, 165], [255, 220, 25], [20, 184, 210], [165, 16, 102], [94, 255, 25],
                              [20, 23, 210]]
    assert len({tuple(x) for x in c.tolist()}) == 100
    assert len({tuple(x) for x in IP.instance_colours(1080).tolist()}) == 1080                # what the docstring promises
    assert IP.instance_colours(0).shape == (0, 3) and np.array_equal(IP.instance_colours(300)[:100], c)


# ------------------------------------------------------------------------------------------------------------------ predict_from_files
class _Net:
    """What predict_from_files looks at before it touches a device."""

    def __init__(self, n):
        self.text_embeddings = torch.zeros((n, 4))

    def _get_engine(self):
        raise AssertionError("validation must come before any device work")

    def predict(self, **kw):
        raise AssertionError("validation must come before any device work")

    def predict_instances_painted(self, *a, **kw):
        raise AssertionError("validation must come before any device work")


def test_the_instance_pictures_are_validated_before_device_work(tmp_path):
    out = str(tmp_path / "out")
    for flags in (dict(instance_map=True), dict(instance_overlay=True), dict(instance_map=True, instance_overlay=True)):
        with pytest.raises(ValueError, match="instance=True"):
            PF.predict_from_files(_Net(7), ["a.jpg"], out_dir=out, **flags)
    with pytest.raises(ValueError, match="needs a palette"):
        PF.predict_from_files(_Net(7), ["a.jpg"], out_dir=out, instance=True, instance_overlay=True, instance_colours="category")
    with pytest.raises(ValueError, match="no colour for label 6"):
        PF.predict_from_files(_Net(7), ["a.jpg"], out_dir=out, semantic=False, instance=True, instance_overlay=True, instance_colours="category",
                              palette={i: (i, i, i) for i in range(6)})
    with pytest.raises(ValueError, match="instance_colours"):
        PF.predict_from_files(_Net(7), ["a.jpg"], out_dir=out, instance=True, instance_overlay=True, instance_colours="rainbow")
    with pytest.raises(ValueError, match="instance_colours"):
        PF.predict_from_files(_Net(7), ["a.jpg"], out_dir=out, instance=True, instance_overlay=True, instance_colours=np.zeros((5, 4)))
    with pytest.raises(ValueError, match="instance_min_score"):
        PF.predict_from_files(_Net(7), ["a.jpg"], out_dir=out, instance=True, instance_map=True, instance_min_score="high")
    with pytest.raises(ValueError, match="alpha"):
        PF.predict_from_files(_Net(7), ["a.jpg"], out_dir=out, instance=True, instance_overlay=True, alpha=300)
    # b's label map (given explicitly) on a's id map; and on a's instance overlay
    with pytest.raises(ValueError, match="b.jpg and a.jpg map to one output path"):
        PF.predict_from_files(_Net(7), ["a.jpg", "b.jpg"], out_paths=[out + "/a.png", out + "/a_instances.png"], instance=True, instance_map=True)
    with pytest.raises(ValueError, match="map to one output path"):
        PF.predict_from_files(_Net(7), ["a.jpg", "b.jpg"], out_paths=[out + "/a.png", out + "/sub/../a_instances_overlay.png"], instance=True,
                              instance_overlay=True)
    # the pictures need a place even when no label map is written
    with pytest.raises(ValueError, match="exactly one"):
        PF.predict_from_files(_Net(7), ["a.jpg"], semantic=False, instance=True, instance_map=True)
    with pytest.raises(ValueError, match="map to one output path"):
        PF.predict_from_files(_Net(7), ["x/a.jpg", "y/a.jpg"], out_dir=out, semantic=False, instance=True, instance_map=True)
    assert not os.path.exists(out)                                                # nothing was created on the way to a refusal
    with pytest.raises(AssertionError, match="device work"):                      # everything in order: the first device step is reached
        PF.predict_from_files(_Net(257), ["a.jpg"], out_dir=out, semantic=False, instance=True, instance_map=True, instance_overlay=True)


def test_the_paths_of_the_pictures_sit_beside_the_label_map(tmp_path):
    images = ["/data/a/im0.jpg", "/data/b/deep.name.jpeg"]
    labels, _ = PF.resolve_output_paths(images, str(tmp_path), None)
    maps, overlays = PF.resolve_instance_paths(images, labels, [labels, None], True, True)
    assert maps == [str(tmp_path / "im0_instances.png"), str(tmp_path / "deep.name_instances.png")]
    assert overlays == [str(tmp_path / "im0_instances_overlay.png"), str(tmp_path / "deep.name_instances_overlay.png")]
    assert PF.resolve_instance_paths(images, labels, [None, None], False, True) == (None, overlays)
    # the semantic overlay of "x_instances" and the instance overlay of "x" are one file
    labels, sem_overlays = PF.resolve_output_paths(["x.jpg", "x_instances.jpg"], "out", None, overlay=True)
    with pytest.raises(ValueError, match="x_instances.jpg and x.jpg map to one output path"):
        PF.resolve_instance_paths(["x.jpg", "x_instances.jpg"], labels, [labels, sem_overlays], False, True)


def test_an_empty_list_gives_the_new_keys_only_when_asked(tmp_path):
    got = PF.predict_from_files(_Net(7), [], out_dir=str(tmp_path / "o"), semantic=False, instance=True, instance_map=True)
    assert got == {"label_paths": None, "overlay_paths": None, "instance_predictions": [], "n_images": 0, "instance_map_paths": [],
                   "instance_overlay_paths": None, "instance_ids": []}
    got = PF.predict_from_files(_Net(7), [], out_dir=str(tmp_path / "o"), instance=True)
    assert sorted(got) == ["instance_predictions", "label_paths", "n_images", "overlay_paths"]


def test_the_new_arguments_are_keyword_only_with_the_documented_defaults():
    p = inspect.signature(PF.predict_from_files).parameters
    want = {"instance_map": False, "instance_overlay": False, "instance_colours": "instance", "instance_min_score": 0.0, "instance_outline": True}
    for name, default in want.items():
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == default, name


# ------------------------------------------------------------------------------------------------------------------ the binding
def test_header_declares_the_entry_and_the_binding_exists():
    from zutis_amd import ops
    e = _lib.entries()["zh_instance_paint"]
    assert [n for _, n in e.params] == ["masks", "bits", "index", "score", "count", "colours", "alpha", "outline", "min_score", "packed", "desc",
                                        "ids_out", "id_format", "overlay_out", "B", "Q", "H", "W", "workspace", "workspace_bytes", "stream"]
    assert dict((n, t) for t, n in e.params)["score"] == "const double*" and dict((n, t) for t, n in e.params)["min_score"] == "double"
    assert e.plannable and "zh_instance_paint_workspace_size" in _lib.entries()
    assert _lib.header_abi_version() >= 235
    assert callable(ops.instance_paint) and callable(ops.instance_paint_workspace_size)


def test_the_visualiser_method_has_the_reference_signature():
    p = inspect.signature(IP.visualise_instance_predictions).parameters
    assert list(p) == ["self", "image", "predictions", "label_id_to_rgb", "confidence_threshold", "fp", "instance_mode"]
    assert p["label_id_to_rgb"].default is None and p["confidence_threshold"].default == 0.75 and p["fp"].default is None

    class Visualiser:
        visualise_instance_predictions = IP.visualise_instance_predictions
    assert inspect.ismethod(Visualiser().visualise_instance_predictions)


def test_the_float_image_is_converted_as_numpy_to_pil_does():
    rng = np.random.default_rng(1)
    x = rng.normal(0.0, 1.5, (3, 5, 6)).astype(np.float32)                       # well beyond [0, 1] after de-normalisation: the clip matters
    want = x * np.array((0.229, 0.224, 0.225))[:, None, None]
    want = np.clip((want + np.array((0.485, 0.456, 0.406))[:, None, None]) * 255.0, 0, 255).astype(np.uint8).transpose(1, 2, 0)
    got = IP._image_bytes(x)
    assert got.dtype == np.uint8 and got.shape == (5, 6, 3) and np.array_equal(got, want)
    assert (got == 0).any() and (got == 255).any()
    from PIL import Image
    assert np.array_equal(IP._image_bytes(Image.fromarray(want)), want)
