"""-m gpu: the device pre-processing of embedding extraction (csrc/preprocess.hip) against Pillow + NumPy, bitwise.

The reference of every comparison is the drop-in's host `_preprocess` (Pillow's bicubic resize, crop, NumPy fp32 normalisation) on
the same files; fp32 outputs are compared with torch.equal, so every check is on bits.  One case also goes against the NumPy
restatement of the resampler (zutis_amd.preprocess.pil_resize_reference), so that a disagreement names its side."""
import os
import pickle

import numpy as np
import pytest
import torch

from tests import _preprocess_case as PC
from zutis_amd import preprocess as P

pytestmark = pytest.mark.gpu


def _lut(E, dev):
    return torch.from_numpy(P.normalise_table(E._MEAN, E._STD)).to(dev)


def _run_batches(E, paths, n_px, batch_size, dev, n_workers=4, kmax_from_batch=True):
    """The loader's batches through the kernel: (fp32 [N, 3, n_px, n_px] on the host, images resized on the host)."""
    from zutis_amd import ops
    lut, outs, n_host = _lut(E, dev), [], 0
    for batch in P.BatchLoader(paths, n_px, batch_size, n_workers, E.resize_crop_box):
        packed, desc = P.split_staging(batch.staging.to(dev), len(batch.paths))
        outs.append(ops.resize_crop_normalize(packed, desc, n_px, lut, kmax=batch.kmax if kmax_from_batch else None).cpu())
        n_host += batch.n_host
    return torch.cat(outs), n_host


def _reference(E, paths, n_px):
    return torch.from_numpy(np.stack([E._preprocess(p, n_px) for p in paths]))


def _report(got, ref, paths):
    bad = [(os.path.basename(p), int((g != r).sum())) for p, g, r in zip(paths, got, ref) if not torch.equal(g, r)]
    print(f"{len(paths)} images, {len(bad)} differ: {bad[:8]}")
    return bad


@pytest.fixture(scope="module")
def shape_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("shapes")
    return [PC.write_rgb(d, f"s{k:02d}_{h}x{w}.png", h, w, seed=1000 + k) for k, (h, w, _) in enumerate(PC.SHAPES)]


@pytest.mark.parametrize("n_px", [336, 224])
def test_kernel_equals_pillow_on_a_ragged_batch(dev, shape_files, n_px):
    """All fourteen source shapes in ONE launch (up- and down-scaling, identity passes, 17 x 900, 2000 x 1500), once with the
    batch's own tap bound and once with the kernel's largest."""
    E = PC.dropin()
    ref = _reference(E, shape_files, n_px)
    for from_batch in (True, False):
        got, n_host = _run_batches(E, shape_files, n_px, len(shape_files), dev, kmax_from_batch=from_batch)
        assert n_host == 0 and got.dtype == torch.float32 and got.shape == ref.shape
        assert not _report(got, ref, shape_files) and torch.equal(got, ref)


def test_kernel_single_image_and_batch_of_37(dev, shape_files):
    E = PC.dropin()
    one = [shape_files[0]]
    got, n_host = _run_batches(E, one, 336, 1, dev)
    assert n_host == 0 and torch.equal(got, _reference(E, one, 336))
    small = [p for p, (h, w, _) in zip(shape_files, PC.SHAPES) if h * w <= 480 * 640]
    many = [small[(5 * k) % len(small)] for k in range(37)]                      # 37 copies of mixed sizes, one launch
    got, n_host = _run_batches(E, many, 224, 37, dev)
    ref1 = {p: torch.from_numpy(E._preprocess(p, 224)) for p in set(many)}
    assert n_host == 0 and got.shape[0] == 37
    assert all(torch.equal(g, ref1[p]) for p, g in zip(many, got))


def test_kernel_equals_the_numpy_restatement(dev):
    """No file, no loader: an array packed by hand (at a non-zero 16-byte-aligned offset) against pil_resize_reference + the table."""
    from zutis_amd import ops
    E = PC.dropin()
    h, w, n_px = 427, 640, 224
    a = PC.pixels(h, w, seed=77)
    (nw, nh), (left, top) = E.resize_crop_box(w, h, n_px)
    off = 48
    packed = np.zeros(off + a.size, np.uint8)
    packed[off:] = a.reshape(-1)
    desc = np.array([[off // 16, w, h, nw, nh, left, top, 0]], np.int32)
    lut = P.normalise_table(E._MEAN, E._STD)
    out = ops.resize_crop_normalize(torch.from_numpy(packed).to(dev), torch.from_numpy(desc).to(dev), n_px, torch.from_numpy(lut).to(dev))
    crop = P.pil_resize_reference(a, nw, nh)[top:top + n_px, left:left + n_px]
    ref = np.stack([lut[c][crop[..., c]] for c in range(3)])[None]
    bad = int((out.cpu().numpy() != ref).sum())
    print(f"kernel vs NumPy restatement: {bad} of {ref.size} values differ")
    assert bad == 0


def test_descriptor_that_does_not_fit_gives_nan_and_is_not_read(dev):
    """An image whose bytes would lie outside the packed buffer, or that needs more taps than the launch's kmax: NaN, no read."""
    from zutis_amd import ops
    E = PC.dropin()
    a = PC.pixels(60, 91, seed=3)
    packed = torch.from_numpy(a.reshape(-1).copy()).to(dev)
    (nw, nh), (left, top) = E.resize_crop_box(91, 60, 42)
    good = [0, 91, 60, nw, nh, left, top, 0]
    outside = [4, 91, 60, nw, nh, left, top, 0]                                   # 64 bytes further on: ends past the buffer
    desc = torch.tensor([good, outside, good], dtype=torch.int32, device=dev)
    out = ops.resize_crop_normalize(packed, desc, 42, _lut(E, dev))
    assert torch.equal(out[0], out[2]) and bool(torch.isfinite(out[0]).all()) and bool(torch.isnan(out[1]).all())
    out = ops.resize_crop_normalize(packed, desc[:1], 42, _lut(E, dev), kmax=5)   # 91 -> 63 needs 7 taps
    assert bool(torch.isnan(out).all())


def test_image_outside_the_envelope_goes_through_the_host_fallback(dev, tmp_path):
    E = PC.dropin()
    big = PC.write_rgb(tmp_path, "big.png", 1600, 1700, seed=9)                   # 155 taps per output pixel at 42 px
    small = PC.write_rgb(tmp_path, "small.png", 60, 91, seed=10)
    got, n_host = _run_batches(E, [big, small], 42, 2, dev)
    assert n_host == 1 and torch.equal(got, _reference(E, [big, small], 42))


def _tower(dev):
    from zutis_amd import detgen
    cfg = detgen.ZutisConfig(width=128, layers=2, patch=14, grid=3, embed_dim=64)       # 42 px tower
    sd = {k.replace("encoder.", "visual."): torch.from_numpy(v) for k, v in detgen.zutis_state_dict(cfg).items() if k.startswith("encoder.")}
    return cfg, sd


def _mixed_files(tmp_path):
    sizes = [(64, 43), (50, 75), (42, 42), (91, 60), (47, 53), (333, 17), (200, 150)]            # (w, h)
    return [PC.write_rgb(tmp_path, f"i{k}.png", h, w, seed=k) for k, (w, h) in enumerate(sizes)] + PC.write_modes(tmp_path)


def test_extract_image_embeddings_end_to_end_bitwise(dev, tmp_path):
    """Ten files of mixed sizes and modes, batch_size 4 (ragged last batch), n_workers 1 and 4: every embedding equals
    encode_image of the host-preprocessed batch bit for bit, the pickle equals the dict, the kernel is launched once per batch, and
    neither a second run nor the worker count changes a byte."""
    from zutis_amd import _lib
    from zutis_amd.engine import ClipImageEncoder
    E = PC.dropin()
    cfg, sd = _tower(dev)
    paths = _mixed_files(tmp_path)
    assert len(paths) >= 9
    enc = ClipImageEncoder({k: v.float().to(dev) for k, v in sd.items()}, cfg.patch, prefix="visual.", precision="exact")
    ref = torch.cat([enc.encode_image(_reference(E, paths[i:i + 4], 42).to(dev)).cpu() for i in range(0, len(paths), 4)])
    runs = []
    for n_workers in (1, 4, 4):
        fp = str(tmp_path / f"emb_{len(runs)}.pkl")
        counts = {}
        _lib.COUNTER = counts
        try:
            out = E.extract_image_embeddings(paths, model_name="ViT-B/16", fp=fp, device=dev, batch_size=4, n_workers=n_workers,
                                             state_dict=sd)
        finally:
            _lib.COUNTER = None
        assert counts.get("zh_resize_crop_normalize_u8") == 3
        assert list(out) == [os.path.basename(p) for p in paths]                  # insertion order = order of the paths
        bad = [k for k, r in zip(out, ref) if not torch.equal(out[k], r)]
        print(f"n_workers={n_workers}: {len(bad)} of {len(out)} embeddings differ from the host path {bad}")
        assert not bad
        disk = pickle.load(open(fp, "rb"))
        assert list(disk) == list(out) and all(torch.equal(disk[k], out[k]) for k in out)
        runs.append(torch.stack([out[k] for k in out]))
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[1], runs[2])


def test_extract_image_embeddings_missing_file_raises(dev, tmp_path):
    E = PC.dropin()
    _, sd = _tower(dev)
    paths = _mixed_files(tmp_path)[:5] + [str(tmp_path / "missing.png")]
    with pytest.raises(FileNotFoundError):
        E.extract_image_embeddings(paths, model_name="ViT-B/16", device=dev, batch_size=2, n_workers=4, state_dict=sd)
