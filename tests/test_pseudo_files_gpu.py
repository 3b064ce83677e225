"""-m gpu: pseudo-label generation from image files — the rectangular Pillow-exact resize + normalise kernel (csrc/preprocess.hip,
ops.resize_normalize) against Pillow + the torch normalisation of MaskDataset, bitwise, and the file-fed driver
(pseudo_masks.generate_pseudo_masks_from_files, the adapter's loader="threads") against the existing tensor-fed drivers, byte for byte.

The end-to-end comparisons feed the existing driver the SAME groups the loader forms (preprocess.bucket_batches): how many images share
a SelfMask call can move a mask pixel (the long-sequence key split), so identity across different groupings is data-dependent and is
not asserted."""
import os
import threading

import numpy as np
import pytest
import torch
from PIL import Image

from tests import _preprocess_case as PC
from zutis_amd import preprocess as P

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)      # MaskDataset's defaults, datasets/index_dataset.py:393-394
PIL_FILTER = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}


def _host_transform(path, image_size, filter="bilinear"):
    """MaskDataset.__getitem__ (datasets/index_dataset.py:405-411) on the host: Pillow's resize, then to_tensor and normalize as torch
    computes them (byte / 255, (x - mean) / std, all fp32)."""
    im = Image.open(path).convert("RGB")
    nw, nh = P.mask_dataset_size(*im.size, image_size)
    if (nw, nh) != im.size:
        im = im.resize((nw, nh), PIL_FILTER[filter])
    x = torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    return (x - torch.tensor(MEAN)[:, None, None]) / torch.tensor(STD)[:, None, None]


def _lut(dev):
    return torch.from_numpy(P.normalise_table(MEAN, STD)).to(dev)


def _kernel_over_files(paths, image_size, batch_size, dev, filter="bilinear", n_workers=4, window=512, kmax_from_batch=True):
    """The loader's batches through the kernel: ({index: fp32 [3, oh, ow] on the host}, batch sizes, images resized on the host)."""
    from zutis_amd import ops
    lut, out, sizes, n_host = _lut(dev), {}, [], 0
    for batch in P.ShapeBucketLoader(paths, image_size, batch_size, n_workers, window=window, filter=filter):
        packed, desc = P.split_staging(batch.staging.to(dev), len(batch.paths))
        y = ops.resize_normalize(packed, desc, *batch.out_hw, lut, filter=filter, kmax=batch.kmax if kmax_from_batch else None).cpu()
        assert y.shape == (len(batch.paths), 3) + tuple(batch.out_hw) and y.dtype == torch.float32
        for i, t in zip(batch.indices, y):
            out[i] = t
        sizes.append(len(batch.paths))
        n_host += batch.n_host
    return out, sizes, n_host


def _differing(got, paths, image_size, filter="bilinear"):
    bad = []
    for i, p in enumerate(paths):
        ref = _host_transform(p, image_size, filter)
        if got[i].shape != ref.shape or not torch.equal(got[i], ref):
            bad.append((os.path.basename(p), tuple(got[i].shape), tuple(ref.shape)))
    print(f"{len(paths)} images [{filter}, image_size {image_size}]: {len(bad)} differ from Pillow + torch {bad[:6]}")
    return bad


def _files(d, shapes, seed0):
    return [PC.write_rgb(d, f"k{seed0}_{k:02d}_{h}x{w}.png", h, w, seed=seed0 + k) for k, (h, w) in enumerate(shapes)]


# ---------------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("filter", ["bilinear", "bicubic"])
def test_kernel_equals_pillow_on_ragged_batches_at_512(dev, tmp_path, filter):
    """Photograph-sized sources of four different shapes per output shape, 512 on the shorter side: ONE launch per output shape
    (512 x 682: up- and down-scaling in one batch; 682 x 512), once with the batch's own tap bound and once with the kernel's largest."""
    land = [(375, 500), (480, 640), (1200, 1600), (150, 200)]                           # all -> 512 x 682
    port = [(500, 375), (640, 480), (2000, 1500), (200, 150)]                           # all -> 682 x 512
    paths = _files(tmp_path, [s for pair in zip(land, port) for s in pair], 100)
    assert {P.mask_dataset_size(w, h, 512) for h, w in land} == {(682, 512)} and {P.mask_dataset_size(w, h, 512) for h, w in port} == {(512, 682)}
    for from_batch in (True, False):
        got, sizes, n_host = _kernel_over_files(paths, 512, 8, dev, filter, kmax_from_batch=from_batch)
        assert sizes == [4, 4] and n_host == 0
        assert not _differing(got, paths, 512, filter)


@pytest.mark.parametrize("filter", ["bilinear", "bicubic"])
def test_kernel_on_the_restated_shapes_and_identity_passes(dev, tmp_path, filter):
    """The shapes of tests/_preprocess_case.py at image_size 64 (17 x 900 -> 64 x 3388 and its transpose among them), plus sources whose
    shorter side already is 64: both passes are then the identity, as Pillow skips them."""
    shapes = [(h, w) for h, w, _ in PC.SHAPES if h * w <= 500 * 700] + [(900, 17), (64, 64), (64, 85), (85, 64), (64, 3388)]
    paths = _files(tmp_path, shapes, 200)
    got, sizes, n_host = _kernel_over_files(paths, 64, 8, dev, filter)
    assert n_host == 0 and sum(sizes) == len(paths)
    assert not _differing(got, paths, 64, filter)
    for i, (h, w) in enumerate(shapes):
        if min(h, w) == 64:                                                             # identity: the table over the file's own bytes
            assert tuple(got[i].shape) == (3, h, w)


def test_kernel_single_image_and_batch_of_37(dev, tmp_path):
    shapes = [(48, 64), (96, 128), (375, 500), (30, 40), (64, 85), (120, 160), (333, 444)]      # all -> 64 x 85
    base = _files(tmp_path, shapes, 300)
    assert {P.mask_dataset_size(w, h, 64) for h, w in shapes} == {(85, 64)}
    got, sizes, n_host = _kernel_over_files(base[:1], 64, 1, dev)
    assert sizes == [1] and n_host == 0 and not _differing(got, base[:1], 64)
    many = [base[(5 * k) % len(base)] for k in range(37)]                                # 37 images of mixed sources, one launch
    got, sizes, n_host = _kernel_over_files(many, 64, 37, dev)
    assert sizes == [37] and n_host == 0 and not _differing(got, many, 64)


@pytest.mark.parametrize("filter", ["bilinear", "bicubic"])
def test_kernel_equals_the_numpy_restatement_one_axis_unchanged(dev, filter):
    """No file, no loader: arrays packed by hand (the second at a non-zero 16-byte-aligned offset) against pil_resize_reference + the
    table; the first changes only its height (the horizontal pass is Pillow's skipped one), the second only its width."""
    from zutis_amd import ops
    a, b = PC.pixels(40, 50, seed=77), PC.pixels(64, 31, seed=78)
    off = -(-a.size // 16) * 16 + 32
    packed = np.zeros(off + b.size, np.uint8)
    packed[:a.size], packed[off:] = a.reshape(-1), b.reshape(-1)
    desc = np.array([[0, 50, 40, 50, 64, 0, 0, 0], [off // 16, 31, 64, 50, 64, 0, 0, 0]], np.int32)
    lut = P.normalise_table(MEAN, STD)
    out = ops.resize_normalize(torch.from_numpy(packed).to(dev), torch.from_numpy(desc).to(dev), 64, 50, torch.from_numpy(lut).to(dev), filter=filter)
    for k, src in enumerate((a, b)):
        r = P.pil_resize_reference(src, 50, 64, filter)
        assert np.array_equal(r, np.asarray(Image.fromarray(src).resize((50, 64), PIL_FILTER[filter])))
        ref = np.stack([lut[c][r[..., c]] for c in range(3)])
        bad = int((out[k].cpu().numpy() != ref).sum())
        print(f"[{filter}] image {k}: {bad} of {ref.size} values differ from the NumPy restatement")
        assert bad == 0


def test_descriptor_that_does_not_fit_gives_nan_and_is_not_read(dev):
    """Bytes outside the packed buffer, another output size than the launch's, a crop, more taps than the launch's kmax: NaN, no read."""
    from zutis_amd import _lib, ops
    a = PC.pixels(60, 91, seed=3)
    packed = torch.from_numpy(a.reshape(-1).copy()).to(dev)
    good = [0, 91, 60, 48, 32, 0, 0, 0]
    rows = [good, [4, 91, 60, 48, 32, 0, 0, 0],                                        # 64 bytes further on: ends past the buffer
            [0, 91, 60, 49, 32, 0, 0, 0], [0, 91, 60, 48, 33, 0, 0, 0],                # resized to something else than out_w x out_h
            [0, 91, 60, 48, 32, 1, 0, 0], [0, 91, 60, 48, 32, 0, -1, 0], good]
    desc = torch.tensor(rows, dtype=torch.int32, device=dev)
    out = ops.resize_normalize(packed, desc, 32, 48, _lut(dev))
    assert torch.equal(out[0], out[6]) and bool(torch.isfinite(out[0]).all())
    assert all(bool(torch.isnan(out[k]).all()) for k in range(1, 6))
    ref = np.asarray(Image.fromarray(a).resize((48, 32), Image.BILINEAR))
    lut = P.normalise_table(MEAN, STD)
    assert np.array_equal(out[0].cpu().numpy(), np.stack([lut[c][ref[..., c]] for c in range(3)]))
    out = ops.resize_normalize(packed, desc[:1], 32, 48, _lut(dev), kmax=3)             # 91 -> 48 needs 5 taps
    assert bool(torch.isnan(out).all())
    with pytest.raises(_lib.ZutisHipError):
        ops.resize_normalize(packed, desc[:1], 32, 48, _lut(dev), filter="bicubic", kmax=3)   # bicubic never has fewer than 5
    with pytest.raises(_lib.ZutisHipError):
        ops.resize_normalize(packed, desc[:1], 32, 48, _lut(dev), filter="lanczos")


def test_image_outside_the_envelope_goes_through_the_host_fallback(dev, tmp_path):
    """THE designated image (tests/test_pseudo_files_cpu.py): 200 x 160 at image_size 2 needs 161 / 201 taps per output pixel."""
    big = PC.write_rgb(tmp_path, "big.png", 160, 200, seed=9)
    small = PC.write_rgb(tmp_path, "small.png", 4, 5, seed=10)
    got, sizes, n_host = _kernel_over_files([big, small], 2, 2, dev)
    assert sizes == [2] and n_host == 1 and not _differing(got, [big, small], 2)


# ------------------------------------------------------------------------------------------------------------------- files -> JSON
IMAGE_SIZE = 64
# (h, w) of the files: upscaled against what SelfMask sees, as test_pseudo_mask_pipeline_matches_sequential sizes its cases; the last
# shape's shorter side already is IMAGE_SIZE (no resize on the way in, none on the way out)
FILE_SHAPES = [(128, 179), (128, 128), (160, 112), (96, 130), (64, 90)]


def _photo(path, h, w, seed):
    rng = np.random.default_rng(seed)
    low = rng.integers(0, 256, (max(2, h // 16), max(2, w // 16), 3), dtype=np.uint8)
    a = np.asarray(Image.fromarray(low).resize((w, h), Image.BICUBIC), np.float32) + rng.normal(0.0, 6.0, (h, w, 3)).astype(np.float32)
    Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)).save(path, compress_level=1)
    return path


@pytest.fixture(scope="module")
def engine(dev):
    from zutis_amd import detgen
    from zutis_amd.engine import SelfMaskEngine
    return SelfMaskEngine({k: torch.from_numpy(v).to(dev) for k, v in detgen.selfmask_state_dict().items()})


@pytest.fixture(scope="module")
def photos(tmp_path_factory):
    """13 seeded files of 5 source shapes in a fixed mixed order: (paths, (H, W) of each)."""
    d = tmp_path_factory.mktemp("photos")
    order = [0, 1, 2, 0, 3, 1, 4, 0, 2, 3, 1, 0, 4]
    hw = [FILE_SHAPES[k] for k in order]
    return [_photo(str(d / f"p{i:02d}.png"), h, w, 700 + i) for i, (h, w) in enumerate(hw)], hw


def _read(paths):
    return [open(p, "rb").read() for p in paths]


def _reference_by_groups(engine, paths, hw, out_paths, groups, dev, batch_size):
    """The existing tensor-fed driver over host-made tensors, one call per group of the loader."""
    from zutis_amd import pseudo_masks
    for g in groups:
        imgs = [_host_transform(paths[i], IMAGE_SIZE).to(dev) for i in g]
        pseudo_masks.generate_pseudo_masks_batched(engine, imgs, [hw[i] for i in g], [out_paths[i] for i in g], batch_size=batch_size)


@pytest.mark.parametrize("batch_size,n_workers", [(4, 4), (8, 16), (3, 1)])
def test_files_in_json_out_equals_the_tensor_fed_driver(dev, engine, photos, tmp_path, batch_size, n_workers):
    from zutis_amd import _lib, pseudo_masks
    paths, hw = photos
    groups = P.bucket_batches([P.mask_dataset_size(w, h, IMAGE_SIZE) for h, w in hw], batch_size, 512)
    assert max(len(g) for g in groups) > 1 and len({hw[g[0]] for g in groups}) >= 4
    pa = [str(tmp_path / "files" / f"{i}.json") for i in range(len(paths))]
    pb = [str(tmp_path / "tensors" / f"{i}.json") for i in range(len(paths))]
    counts = {}
    _lib.COUNTER = counts
    try:
        ret = pseudo_masks.generate_pseudo_masks_from_files(engine, paths, pa, image_size=IMAGE_SIZE, mean=MEAN, std=STD,
                                                            batch_size=batch_size, n_workers=n_workers)
    finally:
        _lib.COUNTER = None
    assert ret == pa and counts.get("zh_resize_normalize_u8") == len(groups)            # one launch per batch, paths in input order
    _reference_by_groups(engine, paths, hw, pb, groups, dev, batch_size)
    a, b = _read(pa), _read(pb)
    bad = [i for i in range(len(paths)) if a[i] != b[i]]
    print(f"batch_size {batch_size}, {len(groups)} batches {[len(g) for g in groups]}: {len(bad)} of {len(paths)} JSON files differ {bad}")
    assert not bad
    import json
    from zutis_amd import rle
    assert all(list(rle.decode(json.loads(x)).shape) == list(s) for x, s in zip(a, hw))   # each mask at its file's own size
    assert not [t for t in threading.enumerate() if t.name.startswith(("zutis-rle", "zutis-decode"))]


def test_batch_size_one_equals_the_one_stream_loop(dev, engine, photos, tmp_path):
    from zutis_amd import pseudo_masks
    paths, hw = photos
    pa = [str(tmp_path / "files" / f"{i}.json") for i in range(len(paths))]
    pb = [str(tmp_path / "loop" / f"{i}.json") for i in range(len(paths))]
    pseudo_masks.generate_pseudo_masks_from_files(engine, paths, pa, image_size=IMAGE_SIZE, mean=MEAN, std=STD, batch_size=1, n_workers=4)
    pseudo_masks.generate_pseudo_masks(engine, [_host_transform(p, IMAGE_SIZE).to(dev) for p in paths], hw, pb, n_streams=1)
    assert _read(pa) == _read(pb)
    pc = [str(tmp_path / "nosolver_files" / f"{i}.json") for i in range(4)]
    pd = [str(tmp_path / "nosolver_loop" / f"{i}.json") for i in range(4)]
    pseudo_masks.generate_pseudo_masks_from_files(engine, paths[:4], pc, image_size=IMAGE_SIZE, mean=MEAN, std=STD, bilateral_solver=False,
                                                  batch_size=1, n_workers=2)
    pseudo_masks.generate_pseudo_masks(engine, [_host_transform(p, IMAGE_SIZE).to(dev) for p in paths[:4]], hw[:4], pd, bilateral_solver=False,
                                       n_streams=1)
    assert _read(pc) == _read(pd)


# ---------------------------------------------------------------------------------------------------------------------- the adapter
class _MaskDataset(torch.utils.data.Dataset):
    """MaskDataset (datasets/index_dataset.py:388-411) restated with Pillow + torch (torchvision is not a dependency of the tests)."""

    def __init__(self, p_images, image_size=IMAGE_SIZE, mean=MEAN, std=STD):
        self.p_images, self.image_size, self.mean, self.std = p_images, image_size, mean, std

    def __len__(self):
        return len(self.p_images)

    def __getitem__(self, i):
        return {"image": _host_transform(self.p_images[i], self.image_size), "p_image": self.p_images[i]}


@pytest.fixture(scope="module")
def network(dev):
    """The drop-in SelfMask module, as the adapter gets it from the reference's factory."""
    import sys
    if PC.DROPIN not in sys.path:
        sys.path.insert(0, PC.DROPIN)
    from networks.selfmask.selfmask import SelfMask
    from zutis_amd import detgen
    net = SelfMask()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in detgen.selfmask_state_dict().items()}, strict=True)
    return net.to(dev)


class _Owner:
    def __init__(self, dev, out_dir):
        self.device, self.out_dir = dev, out_dir

    def _convert_p_image_to_p_pseudo_mask(self, p_image):
        return os.path.join(self.out_dir, os.path.basename(p_image).replace(".png", ".json"))


def test_adapter_threads_mode_writes_the_files_of_the_function(dev, network, photos, tmp_path):
    from zutis_amd import pseudo_masks
    paths, _ = photos
    owner = _Owner(dev, str(tmp_path / "adapter"))
    pseudo_masks.dataset_generate_pseudo_masks(owner, paths, str(tmp_path), 4, True, batch_size=4, network=network, mask_dataset_cls=_MaskDataset,
                                               loader="threads")
    pa = [str(tmp_path / "direct" / f"{i}.json") for i in range(len(paths))]
    pseudo_masks.generate_pseudo_masks_from_files(network._get_engine(), paths, pa, image_size=IMAGE_SIZE, mean=MEAN, std=STD, batch_size=4, n_workers=4)
    assert _read([owner._convert_p_image_to_p_pseudo_mask(p) for p in paths]) == _read(pa)


def test_adapter_dataset_mode_is_unchanged_and_other_networks_are_refused(dev, network, photos, tmp_path):
    """loader="dataset" (the default) through the existing injection points: the files of generate_pseudo_masks_batched over the
    DataLoader's tensors in path order (consecutive images of one shape grouped), as before."""
    from zutis_amd import pseudo_masks
    paths, hw = photos
    for k, kw in enumerate(({}, {"loader": "dataset"})):
        owner = _Owner(dev, str(tmp_path / f"adapter{k}"))
        pseudo_masks.dataset_generate_pseudo_masks(owner, paths, str(tmp_path), 0, True, batch_size=4, network=network, mask_dataset_cls=_MaskDataset, **kw)
        pb = [str(tmp_path / f"batched{k}" / f"{i}.json") for i in range(len(paths))]
        pseudo_masks.generate_pseudo_masks_batched(network._get_engine(), [_host_transform(p, IMAGE_SIZE).to(dev) for p in paths], hw, pb, batch_size=4)
        assert _read([owner._convert_p_image_to_p_pseudo_mask(p) for p in paths]) == _read(pb)
    for mode in ("dataset", "threads"):
        with pytest.raises(TypeError, match="no torch / CPU fallback"):
            pseudo_masks.dataset_generate_pseudo_masks(_Owner(dev, str(tmp_path / "no")), paths, str(tmp_path), 0, True, network=torch.nn.Linear(2, 2),
                                                       mask_dataset_cls=_MaskDataset, loader=mode)
    with pytest.raises(ValueError):
        pseudo_masks.dataset_generate_pseudo_masks(_Owner(dev, str(tmp_path / "no")), paths, str(tmp_path), 0, True, network=network,
                                                   mask_dataset_cls=_MaskDataset, loader="processes")


# ------------------------------------------------------------------------------------------------------------------------ failures
def test_failures_reach_the_caller_and_leave_the_device_usable(dev, engine, photos, tmp_path):
    """A writer's exception (an output directory that cannot be made: its parent is a regular file) and a missing image are raised by
    the call; no thread is left behind, the missing image gets no JSON, and the next call works."""
    from zutis_amd import pseudo_masks
    paths, hw = photos
    blocker = tmp_path / "blocker"
    blocker.write_text("a file where a directory is wanted")
    out = [str(tmp_path / "ok" / f"{i}.json") for i in range(6)]
    out[3] = str(blocker / "sub" / "3.json")
    with pytest.raises(OSError):
        pseudo_masks.generate_pseudo_masks_from_files(engine, paths[:6], out, image_size=IMAGE_SIZE, mean=MEAN, std=STD, batch_size=2, n_workers=4)
    assert not [t for t in threading.enumerate() if t.name.startswith(("zutis-rle", "zutis-decode"))]
    with_missing = paths[:3] + [str(tmp_path / "missing.png")] + paths[3:6]
    out = [str(tmp_path / "miss" / f"{i}.json") for i in range(7)]
    with pytest.raises(FileNotFoundError):
        pseudo_masks.generate_pseudo_masks_from_files(engine, with_missing, out, image_size=IMAGE_SIZE, mean=MEAN, std=STD, batch_size=2, n_workers=4)
    assert not os.path.exists(out[3])
    assert not [t for t in threading.enumerate() if t.name.startswith(("zutis-rle", "zutis-decode"))]
    torch.cuda.synchronize()
    good = [str(tmp_path / "after" / f"{i}.json") for i in range(3)]
    ref = [str(tmp_path / "after_ref" / f"{i}.json") for i in range(3)]
    pseudo_masks.generate_pseudo_masks_from_files(engine, paths[:3], good, image_size=IMAGE_SIZE, mean=MEAN, std=STD, batch_size=1, n_workers=4)
    pseudo_masks.generate_pseudo_masks(engine, [_host_transform(p, IMAGE_SIZE).to(dev) for p in paths[:3]], hw[:3], ref, n_streams=1)
    assert _read(good) == _read(ref)
    with pytest.raises(ValueError):
        pseudo_masks.generate_pseudo_masks_from_files(engine, paths[:2], good, image_size=IMAGE_SIZE)
