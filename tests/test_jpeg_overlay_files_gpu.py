"""-m gpu: predict_from_files(overlay_format="jpeg") on the tiny drop-in ZUTIS and the corpus of tests/test_predict_files_gpu.py: the .jpg
overlays of jpeg_encoder="device" and "host" are the same bytes, each the definition's file (jpeg_device.encode_np) of the PNG overlay
the default call writes for the image; label maps, id maps and predictions are those of the default call; a picture whose scan does not
fit its slot goes through the host arm, is counted, and is the same bytes still."""
import os

import numpy as np
import pytest
from PIL import Image

from tests import _jpeg_enc_case as E
from tests.test_predict_files_gpu import MAX_SIZE, MEAN, N_CAT, PALETTE, STD, _build, _no_threads, images  # noqa: F401  (images: the corpus fixture)
from zutis_amd import jpeg_device as J

pytestmark = pytest.mark.gpu

HOST_ARM = E.pillow_has_restart_blocks()           # without it the host-arm comparison is skipped: encode_np carries the test


@pytest.fixture(scope="module")
def net(dev):
    return _build(dev, N_CAT)


def _predict(net, paths, out_dir, **kw):
    from zutis_amd import predict_files
    got = predict_files.predict_from_files(net, paths, out_dir=str(out_dir), palette=PALETTE, max_size=MAX_SIZE, mean=MEAN, std=STD, batch_size=4, n_workers=6,
                                           overlay=True, instance=True, image_ids=list(range(len(paths))), instance_map=True, instance_overlay=True, **kw)
    assert _no_threads()
    return got


def _rgb(path):
    with Image.open(path) as im:
        assert im.mode == "RGB", path
        return np.asarray(im).copy()


def _same_predictions(a, b):
    assert len(a) == len(b) > 0
    for p, q in zip(a, b):
        assert p.keys() == q.keys() and all(np.array_equal(p[k], q[k]) if k != "segmentation" else p[k]["counts"] == q[k]["counts"] for k in p)


def _check_against_default(default, got, quality, subsampling, root_default, root_got):
    """The .jpg overlays are encode_np of the default call's PNG overlays; every other file and the predictions are the default call's."""
    for key in ("overlay_paths", "instance_overlay_paths"):
        assert len(got[key]) == len(default[key]) > 0
        for png, jpg in zip(default[key], got[key]):
            assert os.path.basename(jpg) == os.path.splitext(os.path.basename(png))[0] + ".jpg"
            assert open(jpg, "rb").read() == J.encode_np(_rgb(png), quality, subsampling), jpg
    for key in ("label_paths", "instance_map_paths"):
        for a, b in zip(default[key], got[key]):
            assert os.path.relpath(a, root_default) == os.path.relpath(b, root_got) and open(a, "rb").read() == open(b, "rb").read(), b
    _same_predictions(default["instance_predictions"], got["instance_predictions"])
    assert got["instance_ids"] == default["instance_ids"] and got["n_images"] == default["n_images"]
    assert set(got) == set(default) | {"jpeg_host_fallbacks"}
    assert len(os.listdir(root_got)) == 4 * got["n_images"] and not [f for f in os.listdir(root_got) if f.endswith("overlay.png")]


def test_jpeg_overlays_of_both_encoders_are_the_definitions_files(dev, net, images, tmp_path):      # noqa: F811
    default = _predict(net, images, tmp_path / "png")
    assert "jpeg_host_fallbacks" not in default
    device = _predict(net, images, tmp_path / "device", overlay_format="jpeg", jpeg_encoder="device")
    _check_against_default(default, device, 90, "4:2:0", tmp_path / "png", tmp_path / "device")
    assert device["jpeg_host_fallbacks"] == 0
    sizes = [sum(os.path.getsize(p) for p in r["overlay_paths"] + r["instance_overlay_paths"]) for r in (default, device)]
    print(f"overlays: {sizes[0]} bytes as PNG, {sizes[1]} as JPEG")
    if HOST_ARM:
        host = _predict(net, images, tmp_path / "host", overlay_format="jpeg", jpeg_encoder="host")
        _check_against_default(default, host, 90, "4:2:0", tmp_path / "png", tmp_path / "host")
        assert host["jpeg_host_fallbacks"] == 0
        for key in ("overlay_paths", "instance_overlay_paths"):
            for a, b in zip(host[key], device[key]):
                assert open(a, "rb").read() == open(b, "rb").read(), b


def test_jpeg_overlays_beside_the_device_png_encoder(dev, net, images, tmp_path):      # noqa: F811
    """png_encoder="device" with either JPEG encoder: the .jpg files are the same, the PNGs decode to the default call's pixels."""
    default = _predict(net, images[:5], tmp_path / "png")
    for jpeg_encoder in ("device",) + (("host",) if HOST_ARM else ()):
        got = _predict(net, images[:5], tmp_path / jpeg_encoder, overlay_format="jpeg", jpeg_encoder=jpeg_encoder, png_encoder="device", jpeg_quality=75,
                       jpeg_subsampling="4:4:4")
        for key in ("overlay_paths", "instance_overlay_paths"):
            for png, jpg in zip(default[key], got[key]):
                assert open(jpg, "rb").read() == J.encode_np(_rgb(png), 75, "4:4:4"), jpg
        for key in ("label_paths", "instance_map_paths"):
            for a, b in zip(default[key], got[key]):
                with Image.open(a) as x, Image.open(b) as y:
                    assert x.mode == y.mode and np.array_equal(np.asarray(x), np.asarray(y)), b
        assert got["jpeg_host_fallbacks"] == 0


def test_a_scan_that_overflows_its_slot_goes_through_the_host_arm(dev, net, images, tmp_path):      # noqa: F811
    """Noise at quality 100 and 4:4:4 with alpha = 0 (the overlays are the image): its JPEG is larger than its pixels."""
    noise = str(tmp_path / "noise.png")
    Image.fromarray(np.random.default_rng(5).integers(0, 256, (64, 96, 3), dtype=np.uint8)).save(noise)
    paths = images[:3] + [noise]                                             # 64 x 96 like images[0] and [2]: it shares their batch
    kw = dict(alpha=0, instance_outline=False)
    default = _predict(net, paths, tmp_path / "png", **kw)
    assert len(J.scan_np(_rgb(default["overlay_paths"][3]), 100, "4:4:4")) > J.scan_slot(64, 96)      # checked on the CPU first
    got = _predict(net, paths, tmp_path / "device", overlay_format="jpeg", jpeg_encoder="device", jpeg_quality=100, jpeg_subsampling="4:4:4", **kw)
    _check_against_default(default, got, 100, "4:4:4", tmp_path / "png", tmp_path / "device")
    too_long = 0
    for key in ("overlay_paths", "instance_overlay_paths"):
        for jpg in got[key]:
            with Image.open(jpg) as im:
                w, h = im.size
            too_long += os.path.getsize(jpg) - len(J.header_bytes(h, w, 100, "4:4:4")) - 2 > J.scan_slot(h, w)
    assert got["jpeg_host_fallbacks"] == too_long >= 2
