"""-m gpu: the file drivers with decoder="device" against their decoder="host" form: baseline JPEG files cross to the device as file
bytes and zh_jpeg_decode makes the pixels; a progressive file, a PNG and a file with a damaged scan take the host route.  The
embeddings are torch.equal, the label PNGs byte-equal: results never depend on the decoder."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import _jpeg_case as C
from tests import _preprocess_case as PC
from tests.test_predict_files_gpu import MAX_SIZE, MEAN, N_CAT, STD, _build, _no_threads, _photo
from tests.test_preprocess_gpu import _tower
from zutis_amd import jpeg_device as J

pytestmark = pytest.mark.gpu


def _photo_array(h, w, seed):
    return np.asarray(_photo(h, w, seed))


@pytest.fixture(scope="module")
def seven(tmp_path_factory):
    """Five files the device serves (three samplings, restart markers, greyscale; mixed sizes), one progressive file, one PNG."""
    d = tmp_path_factory.mktemp("jpeg_files")
    specs = [(60, 91, dict(quality=90)), (75, 50, dict(quality=90, subsampling=0)), (64, 43, dict(quality=75, subsampling=1, optimize=True)),
             (53, 47, dict(quality=90, restart_marker_blocks=3)), (42, 42, dict(quality=85, grey=True))]
    paths = []
    for k, (h, w, kw) in enumerate(specs):
        p = d / f"served{k}.jpg"
        p.write_bytes(C.encode(_photo_array(h, w, 40 + k), **kw))
        assert J.parse(p.read_bytes()) is not None
        paths.append(str(p))
    _photo(70, 58, 50).save(d / "progressive.jpg", quality=90, progressive=True)
    _photo(48, 66, 51).save(d / "plain.png")
    assert J.parse((d / "progressive.jpg").read_bytes()) is None
    return paths[:2] + [str(d / "progressive.jpg")] + paths[2:] + [str(d / "plain.png")]


def _cut_scan(data: bytes) -> bytes:
    """The file with its scan cut at a third and EOI put back: parse() serves it, every decoder finds it truncated."""
    plan = J.parse(data)
    lo, hi = int(plan.segments[0, 0]), int(plan.segments[-1, 1])
    return data[:lo] + data[lo:lo + (hi - lo) // 3] + b"\xff\xd9"


def test_extract_image_embeddings_do_not_depend_on_the_decoder(dev, seven):
    """Seven files, batch_size 4: the embeddings of decoder="device" are torch.equal to decoder="host"; the device decoder ran once per
    batch and two files of the seven were decoded on the host."""
    from zutis_amd import _lib
    from zutis_amd import preprocess as P
    E = PC.dropin()
    _, sd = _tower(dev)
    host = E.extract_image_embeddings(seven, model_name="ViT-B/16", device=dev, batch_size=4, n_workers=4, state_dict=sd)
    counts = {}
    _lib.COUNTER = counts
    try:
        device = E.extract_image_embeddings(seven, model_name="ViT-B/16", device=dev, batch_size=4, n_workers=4, state_dict=sd, decoder="device")
    finally:
        _lib.COUNTER = None
    assert counts.get("zh_jpeg_decode") == 2 and counts.get("zh_resize_crop_normalize_u8") == 2
    assert list(device) == list(host) == [os.path.basename(p) for p in seven]
    bad = [k for k in host if not torch.equal(host[k], device[k])]
    assert not bad, bad
    batches = list(P.BatchLoader(seven, 42, 4, 4, E.resize_crop_box, decoder="device"))
    assert sum(b.n_host_decoded for b in batches) == 2
    assert [os.path.basename(p) for b in batches for p in b.host_decoded_paths] == ["progressive.jpg", "plain.png"]
    with pytest.raises(ValueError, match="decoder"):
        E.extract_image_embeddings(seven, model_name="ViT-B/16", device=dev, state_dict=sd, decoder="gpu")


@pytest.fixture(scope="module")
def net(dev):
    return _build(dev, N_CAT)


@pytest.fixture(scope="module")
def four(tmp_path_factory):
    """Four JPEG files of two shapes, every side a multiple of the 16-pixel patch."""
    d = tmp_path_factory.mktemp("jpeg_predict")
    paths = []
    for k, ((h, w), kw) in enumerate([((64, 96), dict(quality=90)), ((80, 64), dict(quality=90, subsampling=0)),
                                      ((64, 96), dict(quality=85, restart_marker_blocks=4)), ((80, 64), dict(quality=75, subsampling=1))]):
        p = d / f"im{k}.jpg"
        p.write_bytes(C.encode(_photo_array(h, w, 60 + k), **kw))
        paths.append(str(p))
    return paths


def _predict(net, paths, out_dir, decoder):
    from zutis_amd import predict_files
    got = predict_files.predict_from_files(net, paths, out_dir=str(out_dir), max_size=MAX_SIZE, mean=MEAN, std=STD, batch_size=4, n_workers=6,
                                           decoder=decoder)
    assert _no_threads()
    return got


def test_predict_from_files_writes_the_same_label_files(dev, net, four, tmp_path):
    host = _predict(net, four, tmp_path / "host", "host")
    device = _predict(net, four, tmp_path / "device", "device")
    assert len(host["label_paths"]) == len(device["label_paths"]) == 4
    for a, b in zip(host["label_paths"], device["label_paths"]):
        assert os.path.basename(a) == os.path.basename(b) and open(a, "rb").read() == open(b, "rb").read(), b
    labels = [np.asarray(Image.open(p)) for p in device["label_paths"]]
    assert {m.shape for m in labels} == {(64, 96), (80, 64)}


def test_a_damaged_file_among_good_ones_ends_as_on_the_host(dev, net, four, tmp_path):
    """A scan cut at a third (EOI put back): the device reports it and Pillow decodes that file on the calling thread, so the call ends as
    the host decoder's does — the same exception, or (libjpeg pads a premature end and only warns) the same label files byte for byte;
    and the device decoder did report it: the definition refuses the scan."""
    from zutis_amd import predict_files
    bad = tmp_path / "cut.jpg"
    bad.write_bytes(_cut_scan(open(four[0], "rb").read()))
    assert J.parse(bad.read_bytes()) is not None
    with pytest.raises(J.DamagedScan):
        J.decode_np(bad.read_bytes())
    paths = [four[0], str(bad), four[2]]
    raised, results = {}, {}
    for decoder in ("host", "device"):
        try:
            results[decoder] = predict_files.predict_from_files(net, paths, out_dir=str(tmp_path / decoder), max_size=MAX_SIZE, mean=MEAN, std=STD,
                                                                batch_size=4, n_workers=4, decoder=decoder)
            raised[decoder] = None
        except Exception as e:      # noqa: BLE001  (whatever the host path raises is what the device path must raise)
            raised[decoder] = type(e)
        assert _no_threads()
    assert raised["device"] is raised["host"], raised
    if raised["host"] is None:
        assert len(results["device"]["label_paths"]) == 3
        for a, b in zip(results["host"]["label_paths"], results["device"]["label_paths"]):
            assert os.path.basename(a) == os.path.basename(b) and open(a, "rb").read() == open(b, "rb").read(), b
    torch.cuda.synchronize()
    again = _predict(net, four, tmp_path / "after", "device")             # the device stays usable
    assert again["n_images"] == 4
