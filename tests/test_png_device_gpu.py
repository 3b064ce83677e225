"""-m gpu: the device PNG encoder.  zh_png_deflate (csrc/png.hip) against zutis_amd/png_device.deflate_np byte for byte — token edges,
segment edges, ragged batches, inside guard bands — and the file drivers with png_encoder="device" against their "host" form: every
written file decodes to the same pixels, mode and palette."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import _guard as G
from tests import _label_paint_case as LC
from tests import _png_case as C
from tests.test_predict_files_gpu import FILE_HW, MAX_SIZE, MEAN, N_CAT, N_MANY, PALETTE, STD, VARIANTS, _build, _no_threads, images  # noqa: F401  (images: the corpus fixture)
from zutis_amd import png_device as P

pytestmark = pytest.mark.gpu

_REFERENCE = {}


def _reference(c):
    """[(image, deflate_np(image))] of the case images of c channels: computed once, shared, never written."""
    if c not in _REFERENCE:
        _REFERENCE[c] = [(a, P.deflate_np(a)) for a in C.images(c)]
        for a, _ in _REFERENCE[c]:
            a.setflags(write=False)
    return _REFERENCE[c]


def _deflate(dev, imgs, c, order=None):
    """ops.png_deflate over `imgs` as ONE ragged batch, inputs and outputs carved out of guard arenas -> (streams, lengths)."""
    from zutis_amd import ops
    order = list(range(len(imgs))) if order is None else order
    sizes = [imgs[i].shape[:2] for i in order]
    img_off = np.concatenate(([0], np.cumsum([imgs[i].size for i in order]))).astype(np.int64)
    out_off = np.concatenate(([0], np.cumsum([P.stream_bound(h, w, c) for h, w in sizes]))).astype(np.int64)
    max_segments = max(P.segments(h, w, c) for h, w in sizes)
    ws_bytes = ops._lib.load(raw=True).zh_png_deflate_workspace_size(len(order), max_segments)
    ain, aout = G.Arena(G.IN_FILL, dev), G.Arena(G.OUT_FILL, dev)
    v_img = ain.add("images", torch.uint8, 1, int(img_off[-1]), tail_rows=0)
    v_out = aout.add("out", torch.uint8, 1, int(out_off[-1]), tail_rows=0)
    v_len = aout.add("lengths", torch.int32, 1, len(order), tail_rows=0)
    v_ws = aout.workspace("workspace", ws_bytes)
    v_img.put(torch.from_numpy(np.concatenate([imgs[i].reshape(-1) for i in order])).to(dev))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    ops.png_deflate(v_img.m2.reshape(-1), up(img_off[:-1]), up(np.asarray(sizes, np.int32)), c, v_out.m2.reshape(-1), up(out_off[:-1]),
                    v_len.m2.reshape(-1), max_segments, workspace=v_ws.m2.reshape(-1))
    torch.cuda.synchronize()
    G.assert_untouched(aout)                                               # nothing outside out, lengths and the workspace
    flat, lengths = v_out.get().numpy().reshape(-1), v_len.get().numpy().reshape(-1)
    streams = []
    for k in range(len(order)):
        n = int(lengths[k])
        assert 0 < n <= out_off[k + 1] - out_off[k], (k, n)
        streams.append(flat[out_off[k]:out_off[k] + n].tobytes())
        assert (flat[out_off[k] + n:out_off[k + 1]] == G.OUT_FILL).all(), f"image {k}: bytes behind its stream were written"
    return streams, lengths


@pytest.mark.parametrize("c", [1, 3])
def test_kernel_equals_the_definition_one_image_a_launch(dev, c):
    ref = _reference(c)
    for k, (a, want) in enumerate(ref):
        (got,), (n,) = _deflate(dev, [a], c)
        assert n == len(want) and got == want, (k, a.shape, n, len(want))


@pytest.mark.parametrize("c", [1, 3])
def test_kernel_equals_the_definition_in_one_ragged_batch(dev, c):
    """Mixed sizes in one launch (the grid is as wide as the largest image), in an order that puts a three-segment image first and a 1 x 1
    image between larger ones; twice: the bytes are the same every time."""
    ref = _reference(c)
    order = sorted(range(len(ref)), key=lambda i: (-(i % 3), -ref[i][0].size))
    first, lengths = _deflate(dev, [a for a, _ in ref], c, order)
    for k, i in enumerate(order):
        assert lengths[k] == len(ref[i][1]) and first[k] == ref[i][1], (i, ref[i][0].shape)
    again, _ = _deflate(dev, [a for a, _ in ref], c, order)
    assert again == first


def test_an_image_that_does_not_fit_is_left_alone(dev):
    """Too few segments in the grid, a stream bound outside out, bytes outside images: length -1, nothing written, neighbours whole."""
    from zutis_amd import ops
    a = np.ascontiguousarray(C.blocky(83, 401, 2))                           # three segments
    small = np.full((3, 5), 7, np.uint8)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)          # noqa: E731
    images_dev = up(np.concatenate([small.reshape(-1), a.reshape(-1)]))
    bounds = [P.stream_bound(3, 5, 1), P.stream_bound(83, 401, 1)]
    hw = up(np.asarray([[3, 5], [83, 401]], np.int32))
    for case, (img_off, out_bytes, max_segments) in {"grid": ([0, 15], sum(bounds), 2), "out": ([0, 15], sum(bounds) - 1, 3),
                                                     "images": ([0, 16], sum(bounds), 3)}.items():
        out = torch.full((sum(bounds),), G.OUT_FILL, dtype=torch.uint8, device=dev)
        lengths = torch.full((2,), 77, dtype=torch.int32, device=dev)
        ops.png_deflate(images_dev, up(np.asarray(img_off, np.int64)), hw, 1, out[:out_bytes], up(np.asarray([0, bounds[0]], np.int64)), lengths, max_segments)
        got, flat = lengths.cpu().numpy(), out.cpu().numpy()
        want = P.deflate_np(small)
        assert got.tolist() == [len(want), -1], case
        assert flat[:len(want)].tobytes() == want and (flat[len(want):] == G.OUT_FILL).all(), case
    with pytest.raises(ops._lib.ZutisHipError):
        ops.png_deflate(images_dev, up(np.asarray([0, 15], np.int64)), hw, 2, out, up(np.asarray([0, bounds[0]], np.int64)), lengths, 3)


# ---- the drivers

def _pixels(path):
    with Image.open(path) as im:
        return im.mode, np.asarray(im).copy(), (im.getpalette() if im.mode == "P" else None)


def _same_pictures(host_paths, device_paths, mode, palette_bytes=None):
    """... and every device-encoded file is the definition's file of the host arm's pixels, byte for byte: a stream cut too long still
    decodes, only this pins the lengths."""
    assert len(host_paths) == len(device_paths) > 0
    for a, b in zip(host_paths, device_paths):
        (ma, pa, la), (mb, pb, lb) = _pixels(a), _pixels(b)
        assert ma == mb == mode and pa.shape == pb.shape and np.array_equal(pa, pb), b
        assert la == lb or (la[:3 * N_CAT] == lb[:3 * N_CAT] and len(lb) >= 3 * N_CAT), b          # the palette as given (Pillow pads its own to 256)
        assert os.path.basename(a) == os.path.basename(b)
        assert open(b, "rb").read() == P.encode_np(pa, mode, palette_bytes), b


@pytest.fixture(scope="module")
def nets(dev):
    return {N_CAT: _build(dev, N_CAT), N_MANY: _build(dev, N_MANY)}


def _predict(nets, images, out_dir, variant, png_encoder, **kw):      # noqa: F811
    from zutis_amd import predict_files
    n, fmt, pal, _ = VARIANTS[variant]
    got = predict_files.predict_from_files(nets[n], images, out_dir=str(out_dir), label_format=fmt, palette=pal, max_size=MAX_SIZE, mean=MEAN, std=STD,
                                           batch_size=4, n_workers=6, png_encoder=png_encoder, **kw)
    assert _no_threads()
    return got


@pytest.mark.parametrize("variant", ["u8", "rg16"])
def test_label_files_decode_to_the_host_encoders_pixels(dev, nets, images, tmp_path, variant):      # noqa: F811
    n, fmt, _, mode = VARIANTS[variant]
    host = _predict(nets, images, tmp_path / "host", variant, "host")
    device = _predict(nets, images, tmp_path / "device", variant, "device", compress_level=9)       # unused with "device"
    _same_pictures(host["label_paths"], device["label_paths"], mode)
    assert device["overlay_paths"] is None and device["instance_predictions"] == [] and device["n_images"] == len(images)
    assert sorted(os.listdir(tmp_path / "device")) == sorted(os.listdir(tmp_path / "host"))
    sizes = [sum(os.path.getsize(p) for p in r["label_paths"]) for r in (host, device)]
    print(f"{variant}: {sizes[0]} bytes from the host encoder, {sizes[1]} from the device encoder")
    if variant == "u8":                                                     # the device-encoded files are ground truth to the evaluator
        from zutis_amd import evaluate
        ev = evaluate.evaluate_from_files(nets[n], images, device["label_paths"], n, gt_format=fmt, max_size=MAX_SIZE, mean=MEAN, std=STD, batch_size=4)
        cm = ev["confusion_matrix"]
        assert np.array_equal(cm, np.diag(np.diag(cm))) and np.trace(cm) == sum(h * w for h, w in FILE_HW) and ev["scores"]["Pixel Acc"] == 1.0


def test_every_picture_of_a_call_decodes_to_the_host_encoders_pixels(dev, nets, images, tmp_path):      # noqa: F811
    """Mode P label map with its palette, semantic overlay, instance id map and instance overlay in one call, and the returned dict."""
    kw = dict(overlay=True, alpha=96, instance=True, image_ids=list(range(len(images))), instance_map=True, instance_overlay=True)
    host = _predict(nets, images, tmp_path / "host", "u8-palette", "host", **kw)
    device = _predict(nets, images, tmp_path / "device", "u8-palette", "device", **kw)
    _same_pictures(host["label_paths"], device["label_paths"], "P", bytes(v for k in range(N_CAT) for v in PALETTE[k]))
    with Image.open(device["label_paths"][0]) as im:
        assert im.getpalette()[:3 * N_CAT] == [v for k in range(N_CAT) for v in PALETTE[k]]
    _same_pictures(host["overlay_paths"], device["overlay_paths"], "RGB")
    _same_pictures(host["instance_map_paths"], device["instance_map_paths"], "L")
    _same_pictures(host["instance_overlay_paths"], device["instance_overlay_paths"], "RGB")
    strip = lambda r, root: {k: ([os.path.relpath(p, root) for p in v] if k.endswith("_paths") and v is not None else v) for k, v in r.items()}      # noqa: E731
    a, b = strip(host, tmp_path / "host"), strip(device, tmp_path / "device")
    assert a.keys() == b.keys() and len(a["instance_predictions"]) > 0
    for k in a:
        if k != "instance_predictions":
            assert a[k] == b[k], k
    for p, q in zip(a["instance_predictions"], b["instance_predictions"]):
        assert p.keys() == q.keys() and all(np.array_equal(p[k], q[k]) if k != "segmentation" else p[k]["counts"] == q[k]["counts"] for k in p)
    assert len(os.listdir(tmp_path / "device")) == 4 * len(images)


def test_a_writer_failure_reaches_the_caller_and_the_device_stays_usable(dev, nets, images, tmp_path):      # noqa: F811
    from zutis_amd import predict_files
    net = nets[N_CAT]
    os.makedirs(tmp_path / "b" / "im01.png")                                 # a writer's target is a directory
    with pytest.raises(OSError):
        predict_files.predict_from_files(net, images[:5], out_dir=str(tmp_path / "b"), max_size=MAX_SIZE, batch_size=1, n_workers=4, png_encoder="device")
    assert _no_threads()
    (tmp_path / "plain_file").write_bytes(b"not a directory")
    with pytest.raises(OSError):
        predict_files.predict_from_files(net, images[:3], out_dir=str(tmp_path / "plain_file" / "sub"), max_size=MAX_SIZE, png_encoder="device")
    torch.cuda.synchronize()
    host = predict_files.predict_from_files(net, images[:3], out_dir=str(tmp_path / "h"), max_size=MAX_SIZE, mean=MEAN, std=STD, batch_size=1, n_workers=4)
    device = predict_files.predict_from_files(net, images[:3], out_dir=str(tmp_path / "d"), max_size=MAX_SIZE, mean=MEAN, std=STD, batch_size=1, n_workers=4,
                                              png_encoder="device")
    _same_pictures(host["label_paths"], device["label_paths"], "L")
    assert _no_threads()


def test_write_semantic_masks_files_decode_to_the_host_encoders(dev, tmp_path):
    """Polygon annotations on images of two sizes (one of two segments), several ragged launches."""
    from zutis_amd import annotation_labels as AL
    rng = np.random.default_rng(11)
    b = LC.Builder()
    for k in range(7):
        h, w = ((150, 200), (90, 130))[k % 2]
        i = b.image(h, w)
        for _ in range(int(rng.integers(0, 6))):
            x0, y0 = int(rng.integers(0, w - 8)), int(rng.integers(0, h - 8))
            b.add(i, LC.CATEGORIES[int(rng.integers(0, 4))], [LC.rect(x0, y0, x0 + int(rng.integers(4, 90)), y0 + int(rng.integers(4, 70)))])
    gt = b.done()
    host = AL.write_semantic_masks(gt, str(tmp_path / "host"), device=dev, n_workers=4, paint_bytes=70000)
    device = AL.write_semantic_masks(gt, str(tmp_path / "device"), device=dev, n_workers=4, paint_bytes=70000, png_encoder="device")
    assert device["stats"]["launches"] == host["stats"]["launches"] > 2
    want = AL.labels_np(AL.paint_plan(gt))
    assert len({m.shape for m in want}) == 2 and sum(int(m.any()) for m in want) >= 4
    for a, p, m in zip(host["paths"], device["paths"], want):
        assert os.path.basename(a) == os.path.basename(p)
        with Image.open(p) as f:
            assert f.mode == "L" and np.array_equal(np.asarray(f), m), p
        assert open(p, "rb").read() == P.encode_np(m, "L")                   # the file is the definition's, byte for byte
    assert not [t for t in __import__("threading").enumerate() if t.name.startswith("zutis-write")]
