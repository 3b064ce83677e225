"""The device PNG encoder's stream as zutis_amd/png_device.py defines it in NumPy (no GPU): zlib reads it back, Pillow opens the framed
file, the token edges give the length the greedy rule says, and the worst case is the bound.  The drivers' png_encoder keyword."""
import inspect
import io
import zlib

import numpy as np
import pytest
from PIL import Image

from tests import _png_case as C
from zutis_amd import _lib
from zutis_amd import png_device as P

S = P.SEGMENT_BYTES


def test_segment_constant_is_the_headers():
    assert _lib.constants()["ZH_PNG_SEGMENT_BYTES"] == S == 16384
    from zutis_amd import ops
    assert ops.PNG_SEGMENT_BYTES == S


@pytest.mark.parametrize("c", [1, 3])
def test_stream_inflates_to_the_filtered_bytes(c):
    """zlib.decompress checks the Adler-32 as well."""
    for a in C.images(c):
        f = P.filtered(a)
        rows = a.reshape(a.shape[0], -1).astype(np.int64)
        want = np.concatenate([np.full((a.shape[0], 1), 2), (rows - np.vstack([np.zeros_like(rows[:1]), rows[:-1]])) % 256], 1)
        assert np.array_equal(f, want.reshape(-1).astype(np.uint8))
        s = P.deflate_np(a)
        assert s[:2] == b"\x78\x01" and zlib.decompress(s) == f.tobytes(), a.shape
        assert len(s) == C.stream_length(f) <= P.stream_bound(a.shape[0], a.shape[1], c), a.shape


@pytest.mark.parametrize("name", list(C.edge_sequences()))
def test_token_edges_round_trip_at_the_closed_form_length(name):
    d = C.edge_sequences()[name]
    s = P.deflate_filtered(d)
    assert zlib.decompress(s) == d.tobytes()
    assert len(s) == C.stream_length(d), name


def test_run_tokens_are_the_greedy_ones():
    """A run of L <= 3 is L literals; else one literal, matches of 258 while 3 or more bytes are left, then at most 2 literals."""
    for n in C.RUN_LENGTHS + (16384,):
        val, bits = P.run_tokens(np.full(n, 200, np.uint8))
        left = n - 1
        want = [9]
        while left >= 3:
            take = min(258, left)
            want.append(C._match_bits(take))
            left -= take
        want += [9] * left
        assert bits.tolist() == want, n
    val, bits = P.run_tokens(np.arange(256, dtype=np.uint8))
    assert bits.tolist() == [8] * 144 + [9] * 112 and len(set(zip(val.tolist(), bits.tolist()))) == 256


def test_bound_is_reached_by_a_segment_without_runs_of_bytes_from_144():
    d = C.edge_sequences()["worst"]
    n = d.size
    assert n == S + 40 and d.min() >= 144 and (d[1:] != d[:-1]).all()
    s = P.deflate_filtered(d)
    # as a one-row image of n - 1 pixels the filtered bytes would be n long: the bound's arithmetic, on the sequence itself
    assert len(s) == 2 + P.segment_bound(S) + P.segment_bound(40) + 6
    assert P.stream_bound(1, n - 1, 1) == len(s)
    assert P.stream_bound(1, S - 1, 1) == 2 + P.segment_bound(S) + 6 and P.segment_bound(S) == 18438
    rng = np.random.default_rng(0)
    for h, w, c in [(1, 1, 1), (1, 1, 3), (41, 401, 1), (28, 401, 3), (64, 255, 1)]:
        a = rng.integers(0, 256, (h, w) if c == 1 else (h, w, 3)).astype(np.uint8)
        assert len(P.deflate_np(a)) <= P.stream_bound(h, w, c)
        assert P.segments(h, w, c) == -(-(h * (w * c + 1)) // S)


def test_framed_files_open_in_pillow():
    rng = np.random.default_rng(3)
    lab = C.blocky(83, 401, 5)
    pal = bytes(int(v) for v in rng.integers(0, 256, 3 * 21))
    rgb = rng.integers(0, 256, (28, 401, 3)).astype(np.uint8)
    for a, mode, pb in [(lab, "L", None), (lab, "P", pal), (rgb, "RGB", None), (np.full((1, 1), 9, np.uint8), "L", None),
                        (np.arange(300, dtype=np.uint8).reshape(1, 300), "L", None)]:
        with Image.open(io.BytesIO(P.encode_np(a, mode, pb))) as im:
            im.load()
            assert im.mode == mode and im.size == (a.shape[1], a.shape[0])
            assert np.array_equal(np.asarray(im), a)
            if mode == "P":
                assert bytes(im.getpalette()[:len(pal)]) == pal
    with pytest.raises(ValueError):
        P.frame(b"", 4, 4, "L", pal)
    with pytest.raises(ValueError):
        P.frame(b"", 4, 4, "P")
    with pytest.raises(ValueError):
        P.frame(b"", 4, 4, "RGBA")
    with pytest.raises(ValueError):
        P.encode_np(rgb, "L")


def test_png_encoder_keyword_of_the_drivers(tmp_path):
    from zutis_amd import annotation_labels, predict_files
    for fn in (predict_files.predict_from_files, annotation_labels.write_semantic_masks):
        p = inspect.signature(fn).parameters["png_encoder"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "host"
    gt = {"images": [{"id": 1, "height": 8, "width": 8, "file_name": "a.jpg"}], "categories": [{"id": 1}],
          "annotations": [{"id": 1, "image_id": 1, "category_id": 1, "segmentation": [[1, 1, 6, 1, 6, 6, 1, 6]], "iscrowd": 0}]}
    for route in ("host", "device"):
        with pytest.raises(ValueError, match="png_encoder"):
            annotation_labels.write_semantic_masks(gt, str(tmp_path / "x"), route=route, png_encoder="gpu")
    with pytest.raises(ValueError, match="route"):
        annotation_labels.write_semantic_masks(gt, str(tmp_path / "y"), route="host", png_encoder="device")
    assert not (tmp_path / "x").exists() and not (tmp_path / "y").exists()                    # refused before any work
    got = annotation_labels.write_semantic_masks(gt, str(tmp_path / "z"), route="host")          # the default still writes with Pillow
    assert np.asarray(Image.open(got["paths"][0])).sum() > 0
    with pytest.raises(ValueError, match="png_encoder"):
        predict_files.predict_from_files(object(), ["a.png"], out_dir=str(tmp_path / "w"), png_encoder="zlib")
    assert not (tmp_path / "w").exists()
