"""CPU: the host side of the device pre-processing of embedding extraction (zutis_amd/preprocess.py) — the NumPy restatement of
Pillow's resampler against the installed Pillow (zero differing bytes), the normalisation table against the drop-in's `_preprocess`
(bitwise), and the threaded loader's packing (no GPU: offsets, descriptor rows, order, modes, errors)."""
import numpy as np
import pytest
import torch
from PIL import Image

from tests import _preprocess_case as PC
from zutis_amd import preprocess as P


def _resized(h, w, n_px):
    E = PC.dropin()
    return E.resize_crop_box(w, h, n_px)


@pytest.mark.parametrize("h,w,n_px", PC.SHAPES)
def test_pil_resize_reference_equals_pillow_byte_for_byte(h, w, n_px):
    """The oracle of the GPU tests IS Pillow's resampler: no tolerance.  The installed Pillow decides — a build that resamples
    differently fails here first."""
    a = PC.pixels(h, w, seed=h * 10007 + w)
    (nw, nh), _ = _resized(h, w, n_px)
    ref = np.asarray(Image.fromarray(a).resize((nw, nh), Image.BICUBIC))
    got = P.pil_resize_reference(a, nw, nh)
    assert got.shape == ref.shape and got.dtype == np.uint8
    bad = int((got != ref).sum())
    assert bad == 0, f"{h}x{w} -> {nh}x{nw}: {bad} of {ref.size} bytes differ from Pillow {Image.__version__}"


def test_ksize_and_envelope():
    assert P.ksize(500, 448) == 7 and P.ksize(336, 336) == 5 and P.ksize(200, 336) == 5 and P.ksize(8192, 224) == 149
    for n_px in (224, 336):
        assert P.device_supported(8192, 8192, n_px) and P.device_supported(8192, 300, n_px) and P.device_supported(17, 900, n_px)
    assert not P.device_supported(9000, 9000, 224) and P.ksize(9000, 224) > P.KMAX
    kk, bounds = P.pil_coefficients(336, 336)                 # an unchanged axis: one unit tap — the identity
    assert all(int(kk[i, :bounds[i, 1]].sum()) == 1 << 22 and int((kk[i] != 0).sum()) == 1 for i in range(336))


@pytest.mark.parametrize("h,w,n_px", [(375, 500, 336), (640, 427, 224), (60, 91, 42)])
def test_normalise_table_gathers_to_preprocess(tmp_path, h, w, n_px):
    E = PC.dropin()
    p = PC.write_rgb(tmp_path, "a.png", h, w, seed=5)
    (nw, nh), (left, top) = E.resize_crop_box(w, h, n_px)
    crop = np.asarray(Image.open(p).convert("RGB").resize((nw, nh), Image.BICUBIC))[top:top + n_px, left:left + n_px]
    lut = P.normalise_table(E._MEAN, E._STD)
    assert lut.shape == (3, 256) and lut.dtype == np.float32
    got = np.stack([lut[c][crop[..., c]] for c in range(3)])
    assert np.array_equal(got, E._preprocess(p, n_px))


@pytest.mark.parametrize("n_workers", [1, 4])
def test_loader_packs_batches_in_order(tmp_path, n_workers):
    E = PC.dropin()
    sizes = [(64, 43), (50, 75), (42, 42), (91, 60), (47, 53), (333, 17), (5, 400)]           # (w, h)
    paths = [PC.write_rgb(tmp_path, f"i{k}.png", h, w, seed=k) for k, (w, h) in enumerate(sizes)] + PC.write_modes(tmp_path)
    loader = P.BatchLoader(paths, 42, 4, n_workers, E.resize_crop_box, pin=False)
    assert len(loader) == 3 and loader.n_threads == n_workers
    seen = []
    for batch in loader:
        B = len(batch.paths)
        assert batch.desc.shape == (B, 8) and batch.desc.dtype == torch.int32 and batch.packed.dtype == torch.uint8
        assert batch.staging.numel() == 32 * B + batch.packed.numel() and batch.n_host == 0
        end, kmax = 0, 5
        for p, row in zip(batch.paths, batch.desc.tolist()):
            with Image.open(p) as im:
                w, h = im.size
                ref = np.asarray(im.convert("RGB"))
            (nw, nh), (left, top) = E.resize_crop_box(w, h, 42)
            assert row[1:] == [w, h, nw, nh, left, top, 0]
            off = row[0] * 16
            assert off >= end                                    # 16-byte aligned by construction, not overlapping
            end = off + 3 * w * h
            assert end <= batch.packed.numel()
            got = batch.packed.numpy()[off:end].reshape(h, w, 3)
            assert np.array_equal(got, ref), p
            kmax = max(kmax, P.ksize(w, nw), P.ksize(h, nh))
        assert batch.kmax == kmax
        seen += batch.paths
    assert seen == paths


def test_loader_threads_capped_and_missing_file_raises(tmp_path):
    E = PC.dropin()
    paths = [PC.write_rgb(tmp_path, f"i{k}.png", 40 + k, 50, seed=k) for k in range(3)]
    assert P.BatchLoader(paths, 42, 2, 64, E.resize_crop_box, pin=False).n_threads == 16
    paths.insert(2, str(tmp_path / "missing.png"))
    with pytest.raises(FileNotFoundError):
        for _ in P.BatchLoader(paths, 42, 2, 4, E.resize_crop_box, pin=False):
            pass
    assert list(P.BatchLoader([], 42, 2, 4, E.resize_crop_box, pin=False)) == []


def test_loader_resizes_on_the_host_outside_the_envelope(tmp_path):
    """A 1700 x 1600 source at n_px = 42 needs 155 taps per output pixel (> KMAX): its worker hands over Pillow's own 42 x 42 crop
    and a descriptor whose two passes are the identity."""
    E = PC.dropin()
    big = PC.write_rgb(tmp_path, "big.png", 1600, 1700, seed=9)
    small = PC.write_rgb(tmp_path, "small.png", 60, 91, seed=10)
    assert not P.device_supported(1700, 1600, 42) and P.device_supported(91, 60, 42)
    (batch,) = list(P.BatchLoader([big, small], 42, 2, 2, E.resize_crop_box, pin=False))
    assert batch.n_host == 1 and batch.desc[0].tolist() == [0, 42, 42, 42, 42, 0, 0, 0] and batch.kmax == 7
    (nw, nh), (left, top) = E.resize_crop_box(1700, 1600, 42)
    ref = np.asarray(Image.open(big).convert("RGB").resize((nw, nh), Image.BICUBIC).crop((left, top, left + 42, top + 42)))
    assert np.array_equal(batch.packed.numpy()[:3 * 42 * 42].reshape(42, 42, 3), ref)
