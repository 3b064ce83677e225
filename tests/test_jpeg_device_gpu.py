"""-m gpu: the device JPEG decoder.  zh_jpeg_decode (csrc/jpeg.hip over csrc/jpeg_codec.h) against zutis_amd/jpeg_device.decode_np byte
for byte — every size of tests/_jpeg_case.py with its 16 variants in ONE ragged launch, a launch mixing sizes, samplings, optimised
tables and restart markers — with the RGB output, the workspace and the status array inside guard bands; damaged scans last, on the
bytes the host twin of the codec has been run over under the host sanitizers (tools/host/jpeg_host_check.cpp)."""
import numpy as np
import pytest
import torch

from tests import _guard as G
from tests import _jpeg_case as C
from zutis_amd import jpeg_device as J

pytestmark = pytest.mark.gpu

_REFERENCE = {}


def _reference(name, data):
    """(plan, decode_np) of a corpus file: computed once, shared, never written."""
    if name not in _REFERENCE:
        plan = J.parse(data)
        a = J.decode_np(data, plan)
        a.setflags(write=False)
        _REFERENCE[name] = (plan, a)
    return _REFERENCE[name]


def _decode(dev, plans, datas):
    """ops.jpeg_decode over one launch's arrays, outputs carved out of guard arenas -> (images, status)."""
    from zutis_amd import ops
    packed = J.pack(plans, datas)
    B = len(plans)
    ws_bytes = ops._lib.load(raw=True).zh_jpeg_decode_workspace_size(B, packed.n_blocks)
    ain, aout = G.Arena(G.IN_FILL, dev), G.Arena(G.OUT_FILL, dev)
    v_scan = ain.add("scan", torch.uint8, 1, packed.scan.size, tail_rows=0)
    v_out = aout.add("out", torch.uint8, 1, packed.out_bytes, tail_rows=0)
    v_status = aout.add("status", torch.int32, 1, B, tail_rows=0)
    v_ws = aout.workspace("workspace", ws_bytes)
    v_scan.put(torch.from_numpy(packed.scan).to(dev))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    ops.jpeg_decode(v_scan.m2.reshape(-1), up(packed.segments), up(packed.images), up(packed.tables), packed.n_blocks, packed.max_image_blocks,
                    packed.max_image_pixels, v_out.m2.reshape(-1), v_status.m2.reshape(-1), workspace=v_ws.m2.reshape(-1))
    torch.cuda.synchronize()
    G.assert_untouched(aout)                                               # nothing outside out, status and the workspace
    flat = v_out.get().numpy().reshape(-1)
    for b, (h, w) in enumerate(packed.shapes):                             # nor between the images of out
        lo = int(packed.out_off[b]) + 3 * h * w
        hi = int(packed.out_off[b + 1]) if b + 1 < B else packed.out_bytes
        assert (flat[lo:hi] == G.OUT_FILL).all(), f"image {b}: bytes behind its pixels were written"
    return J.unpack(packed, flat), v_status.get().numpy().reshape(-1), flat, packed


@pytest.mark.parametrize("hw", C.SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_kernel_equals_the_definition_per_size(dev, hw):
    """All 16 variants of a size — 4:2:0, 4:4:4, 4:2:2, optimised tables, q100, q30, restart markers, greyscale; noise and smooth — in one
    ragged launch."""
    names, datas = zip(*C.variants(*hw))
    refs = [_reference(n, d) for n, d in zip(names, datas)]
    images, status, _, _ = _decode(dev, [p for p, _ in refs], datas)
    assert not status.any(), status.tolist()
    for n, got, (_, want) in zip(names, images, refs):
        assert got.shape == want.shape and np.array_equal(got, want), (n, int((got != want).sum()))


def test_one_launch_mixes_sizes_samplings_tables_and_restarts(dev):
    """Five sizes, three samplings, an optimised-table file and restart files side by side, the largest neither first nor last; twice:
    the bytes are the same every time."""
    picks = [(9, 5, "q90-422", "noise"), (64, 48, "q90-rst", "smooth"), (1, 1, "q90-444", "noise"), (37, 53, "q75-opt", "smooth"),
             (33, 64, "q90-420", "noise"), (37, 53, "q90-rst", "noise"), (64, 48, "q85-grey", "smooth"), (9, 5, "q100-420", "smooth")]
    names = [f"{h}x{w}-{s}-{k}" for h, w, s, k in picks]
    datas = [C.file_bytes(*p) for p in picks]
    refs = [_reference(n, d) for n, d in zip(names, datas)]
    images, status, first, packed = _decode(dev, [p for p, _ in refs], datas)
    assert not status.any() and packed.tables.shape[0] >= 4 and len(packed.segments) > len(picks)
    for n, got, (_, want) in zip(names, images, refs):
        assert np.array_equal(got, want), n
    _, _, again, _ = _decode(dev, [p for p, _ in refs], datas)
    assert np.array_equal(first, again)


def test_damaged_scans_are_reported_and_their_neighbours_exact(dev):
    """The five damaged scans of tests/_jpeg_case.py, each between good files in ONE launch: a non-zero status for each of them, zero for
    the good files, whose pixels are exact; the guards stay intact (checked in _decode)."""
    good = [("16x16-q90-444-noise", C.file_bytes(16, 16, "q90-444", "noise")), ("33x64-q90-rst-smooth", C.file_bytes(33, 64, "q90-rst", "smooth"))]
    refs = [_reference(n, d) for n, d in good]
    plans, datas, bad = [refs[0][0]], [good[0][1]], []
    for kind in C.DAMAGED:
        plan, data = C.damaged(kind)
        bad.append(len(plans))
        plans += [plan, refs[len(bad) % 2][0]]
        datas += [data, good[len(bad) % 2][1]]
    images, status, _, _ = _decode(dev, plans, datas)
    for b in range(len(plans)):
        if b in bad:
            assert status[b] != 0, (b, C.DAMAGED[bad.index(b)])
        else:
            want = refs[0][1] if plans[b] is refs[0][0] else refs[1][1]
            assert status[b] == 0 and np.array_equal(images[b], want), b
