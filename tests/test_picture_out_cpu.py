"""CPU: the output side of the drivers that write pictures (zutis_amd/picture_out.py) — the layout of a batch's output buffer as properties
of its regions, and the writer stage with the host encoder on CPU tensors: which batch is handed to the writers when, what the files
decode to, where a writer's failure surfaces.  Nothing here sleeps."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
from PIL import Image

from zutis_amd import picture_out as PO
from zutis_amd import png_device as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PALETTE = bytes(range(30))                                               # ten (r, g, b) entries

UNIFORM = ([(5, 7)] * 3, [(1, "P", PALETTE), (3, "RGB", None), (1, "L", None), (3, "RGB", None)])
RAGGED = [(3, 5), (83, 401), (1, 1)]                                     # 83 x 401 x 3: several 16 KiB segments
CASES = {"uniform": UNIFORM, "ragged-1": (RAGGED, [(1, "L", None)]), "ragged-1-3": (RAGGED, [(1, "L", None), (3, "RGB", None)])}


def _write_threads():
    return [t for t in threading.enumerate() if t.name.startswith("zutis-write")]


# ------------------------------------------------------------------------------------------------------------------ the layout
@pytest.mark.parametrize("case", sorted(CASES))
def test_layout_regions_are_disjoint_ordered_and_of_their_pictures_sizes(case):
    sizes, kinds = CASES[case]
    lay = PO.Layout(sizes, kinds)
    B, K = len(sizes), len(kinds)
    order = [(k, b) for k in range(K) for b in range(B)]                 # kind-major, image-minor: picture (k, b) is number k * B + b
    assert [(h, w, c, mode) for h, w, c, mode, _ in lay.pictures] == [(*sizes[b], *kinds[k][:2]) for k, b in order]
    assert lay.raw_at[0] == 0 and len(lay.raw_at) == len(lay.stream_at) == B * K + 1
    for i, (k, b) in enumerate(order):                                   # raw: back to back in that order, h * w * c bytes each
        assert lay.raw_at[i + 1] - lay.raw_at[i] == sizes[b][0] * sizes[b][1] * kinds[k][0], (k, b)
        # streams: in the same order, none shorter than its bound, none overlapping its successor
        assert lay.stream_at[i] >= 0 and lay.stream_at[i + 1] - lay.stream_at[i] >= P.stream_bound(*sizes[b], kinds[k][0]), (k, b)
    assert lay.raw_bytes == lay.raw_at[-1] == lay.host_bytes["host"]
    for k in range(K):                                                   # a kind's span: from its first picture to its last one's end
        assert lay.span(lay.raw_at, k) == slice(lay.raw_at[k * B], lay.raw_at[k * B + B])
        assert lay.span(lay.stream_at, k) == slice(lay.stream_at[k * B], lay.stream_at[k * B + B])
    end = int(lay.stream_at[-1])
    assert end <= lay.lengths_at < end + 4 and lay.lengths_at % 4 == 0   # the length words: 4-byte aligned, right behind the last stream,
    assert lay.host_bytes["device"] == lay.lengths_at + 4 * B * K        # one per picture, in picture order
    assert lay.max_segments == tuple(max(P.segments(h, w, c) for h, w in sizes) for c, _, _ in kinds)
    assert case == "uniform" or lay.max_segments[-1] > 1


def test_a_uniform_kind_is_one_contiguous_block():
    import torch
    sizes, kinds = UNIFORM
    lay = PO.Layout(sizes, kinds)
    raw = torch.arange(lay.raw_bytes, dtype=torch.int32).to(torch.uint8)
    for k, ((c, _, _), view) in enumerate(zip(kinds, lay.views(raw))):
        span = lay.span(lay.raw_at, k)
        assert span.stop - span.start == 3 * 5 * 7 * c and tuple(view.shape) == ((3, 5, 7) if c == 1 else (3, 5, 7, 3))
        assert [int(lay.raw_at[k * 3 + i]) for i in range(3)] == [span.start + i * 5 * 7 * c for i in range(3)]
        assert view.data_ptr() == raw.data_ptr() + span.start and torch.equal(view.reshape(-1), raw[span])
    with pytest.raises(ValueError):
        PO.Layout(RAGGED, [(1, "L", None)]).views(raw)


def test_the_module_imports_without_torch():
    code = "import sys; import zutis_amd.picture_out; assert 'torch' not in sys.modules, 'torch was imported'"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True).returncode == 0


# ------------------------------------------------------------------------------------------------------------------ the stage
KINDS = [(1, "L", None), (1, "P", PALETTE), (3, "RGB", None)]
BATCHES = [[(6, 9)] * 3, [(4, 5)], [(2, 2), (7, 3)], [(7, 3), (11, 8), (2, 2), (5, 5)]]      # slot 0 goes on to a smaller layout, slot 1 to a larger


def _pictures(rng, sizes):
    return [[rng.integers(0, 10 if mode == "P" else 256, (h, w) if c == 1 else (h, w, c), dtype=np.uint8) for h, w in sizes] for c, mode, _ in KINDS]


def _step(tmp_path, stage, k, before_commit=None):
    """Batch k through the stage: take, fill the raw buffer picture by picture, commit -> {path: (kind, pixels)}."""
    import torch
    sizes, pics = BATCHES[k], _pictures(np.random.default_rng(k), BATCHES[k])
    lay = PO.Layout(sizes, KINDS)
    paths = [str(tmp_path / f"b{k}_k{j}_{b}.png") for j in range(len(KINDS)) for b in range(len(sizes))]
    raw = stage.take(k, lay, paths)
    assert raw.numel() == lay.raw_bytes and raw.device.type == "cpu"
    for i, a in enumerate(a for kind in pics for a in kind):
        raw[lay.raw_at[i]:lay.raw_at[i + 1]] = torch.from_numpy(a.reshape(-1))
    if len(set(sizes)) == 1:                                             # a batch of one size: the kinds as the kernels see them
        assert all(np.array_equal(v.numpy(), np.stack(p)) for v, p in zip(lay.views(raw), pics))
    if before_commit:
        before_commit()
    stage.commit()
    return {paths[j * len(sizes) + b]: (KINDS[j], pics[j][b]) for j in range(len(KINDS)) for b in range(len(sizes))}


def test_stage_hands_batch_k_minus_1_over_at_commit_k_and_the_last_at_exit(tmp_path, monkeypatch):
    submitted, want = [], {}
    real = PO.write_png
    monkeypatch.setattr(PO, "write_png", lambda path, *a: (submitted.append(os.path.basename(path)), real(path, *a)))      # on a writer thread
    with PO.PictureStage("host", False, 3, compress_level=1) as stage:
        def handed_over():
            stage.ring.drain()                                           # whatever was handed over has run now
            return sorted({name.split("_")[0] for name in submitted})

        def one_behind(k):
            assert handed_over() == [f"b{i}" for i in range(k - 1)]      # batch k - 1 waits for commit k
        for k in range(len(BATCHES)):
            want.update(_step(tmp_path, stage, k, before_commit=lambda: one_behind(k)))
            assert handed_over() == [f"b{i}" for i in range(k)]          # commit k: batch k - 1, and never batch k
            assert len(submitted) == 3 * sum(len(b) for b in BATCHES[:k])
    assert sorted(submitted) == sorted(os.path.basename(p) for p in want) and not _write_threads()
    for path, ((c, mode, palette), a) in want.items():
        with Image.open(path) as im:
            assert im.mode == mode and np.array_equal(np.asarray(im), a), path
            assert mode != "P" or bytes(im.getpalette()[:len(PALETTE)]) == palette


def test_a_failing_writer_surfaces_at_the_next_take_of_its_slot_or_at_exit(tmp_path, monkeypatch):
    def fails(path, *a):
        if os.path.basename(path) in ("b0_k1_2.png", "b3_k0_0.png"):
            raise OSError(f"no room for {os.path.basename(path)}")
    monkeypatch.setattr(PO, "write_png", fails)
    reached = []
    with pytest.raises(OSError, match="no room for b0_k1_2.png"):
        with PO.PictureStage("host", False, 2) as stage:
            _step(tmp_path, stage, 0)
            _step(tmp_path, stage, 1)                                    # commit 1 hands batch 0 over
            reached.append("take 2")
            _step(tmp_path, stage, 2)                                    # slot 0 again: its writers' failure is raised here
            reached.append("commit 2")
    assert reached == ["take 2"] and not _write_threads()
    with pytest.raises(OSError, match="no room for b3_k0_0.png"):
        with PO.PictureStage("host", False, 2) as stage:
            _step(tmp_path, stage, 3)
            reached.append("exit")                                       # the only batch is handed over and waited for on the way out
    assert reached == ["take 2", "exit"] and not _write_threads()


def test_the_device_encoder_without_a_gpu_is_an_error_not_a_fallback():
    from zutis_amd import _lib
    with pytest.raises(_lib.ZutisHipError):
        PO.PictureStage("device", False, 1)
    assert not _write_threads()
