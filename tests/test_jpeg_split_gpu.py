"""-m gpu: the device JPEG decoder with every scan split among lanes.  zh_jpeg_decode_split (csrc/jpeg.hip over csrc/jpeg_codec.h)
against zutis_amd/jpeg_device.decode_np byte for byte and against its host twin status for status — every size of tests/_jpeg_case.py
with its 16 variants in ONE ragged launch, at 16-byte chunks (hundreds of chunks, several sequences) and at the shipped chunk size; a
launch mixing sizes, samplings, table sets, restart files and multi-sequence files; one synchronising pass where two are needed; damaged
scans between good files; a loader batch through decode_staged — with the RGB output, the workspace and the status array inside guard
bands."""
import numpy as np
import pytest
import torch

from tests import _guard as G
from tests import _jpeg_case as C
from zutis_amd import jpeg_device as J

pytestmark = pytest.mark.gpu

_REFERENCE = {}
UNSYNCED = J.STATUS.get("unsynced", 0)


def _reference(name, data):
    """(plan, decode_np) of a corpus file: computed once, shared, never written."""
    if name not in _REFERENCE:
        plan = J.parse(data)
        a = J.decode_np(data, plan)
        a.setflags(write=False)
        _REFERENCE[name] = (plan, a)
    return _REFERENCE[name]


def _decode(dev, plans, datas, chunk_bytes, passes=None):
    """ops.jpeg_decode_split over one launch's arrays, outputs carved out of guard arenas -> (images, status, host twin's status, packed);
    passes None: as many as the launch has sequences (always enough)."""
    from zutis_amd import ops
    packed = J.pack(plans, datas, chunk_bytes=chunk_bytes)
    passes = J.sequences(packed) if passes is None else passes
    B = len(plans)
    ws_bytes = ops._lib.load(raw=True).zh_jpeg_decode_split_workspace_size(B, packed.n_blocks, len(packed.chunks))
    ain, aout = G.Arena(G.IN_FILL, dev), G.Arena(G.OUT_FILL, dev)
    v_scan = ain.add("scan", torch.uint8, 1, packed.scan.size, tail_rows=0)
    v_chunks = ain.add("chunks", torch.int32, len(packed.chunks), J.CHUNK_WORDS, tail_rows=0)
    v_out = aout.add("out", torch.uint8, 1, packed.out_bytes, tail_rows=0)
    v_status = aout.add("status", torch.int32, 1, B, tail_rows=0)
    v_ws = aout.workspace("workspace", ws_bytes)
    v_scan.put(torch.from_numpy(packed.scan).to(dev))
    v_chunks.put(torch.from_numpy(packed.chunks).to(dev))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    ops.jpeg_decode_split(v_scan.m2.reshape(-1), up(packed.segments), v_chunks.m2, up(packed.images), up(packed.tables), packed.n_blocks,
                          packed.max_image_blocks, packed.max_image_pixels, v_out.m2.reshape(-1), v_status.m2.reshape(-1), chunk_bytes=chunk_bytes,
                          passes=passes, workspace=v_ws.m2.reshape(-1))
    torch.cuda.synchronize()
    G.assert_untouched(aout)                                               # nothing outside out, status and the workspace
    flat = v_out.get().numpy().reshape(-1)
    for b, (h, w) in enumerate(packed.shapes):                             # nor between the images of out
        lo = int(packed.out_off[b]) + 3 * h * w
        hi = int(packed.out_off[b + 1]) if b + 1 < B else packed.out_bytes
        assert (flat[lo:hi] == G.OUT_FILL).all(), f"image {b}: bytes behind its pixels were written"
    _, twin = J.decode_split_host(packed, passes=passes)
    return J.unpack(packed, flat), v_status.get().numpy().reshape(-1), twin, packed


@pytest.mark.parametrize("chunk_bytes", [16, J.CHUNK_BYTES if hasattr(J, "CHUNK_BYTES") else 128], ids=["16", "default"])
@pytest.mark.parametrize("hw", C.SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_kernel_equals_the_definition_per_size(dev, hw, chunk_bytes):
    """All 16 variants of a size in one ragged launch: the definition's pixels, and the host twin's status (zero)."""
    names, datas = zip(*C.variants(*hw))
    refs = [_reference(n, d) for n, d in zip(names, datas)]
    images, status, twin, _ = _decode(dev, [p for p, _ in refs], datas, chunk_bytes)
    assert np.array_equal(status, twin) and not status.any(), (status.tolist(), twin.tolist())
    for n, got, (_, want) in zip(names, images, refs):
        assert got.shape == want.shape and np.array_equal(got, want), (n, int((got != want).sum()))


MIXED = [(9, 5, "q90-422", "noise"), (64, 48, "q90-rst", "smooth"), (64, 48, "q90-444", "noise"), (1, 1, "q90-444", "noise"), (37, 53, "q75-opt", "smooth"),
         (33, 64, "q90-420", "noise"), (37, 53, "q90-rst", "noise"), (64, 48, "q100-420", "noise"), (64, 48, "q85-grey", "smooth"), (9, 5, "q100-420", "smooth")]


def test_one_launch_mixes_sizes_samplings_tables_restarts_and_long_scans(dev):
    """Five sizes, three samplings, an optimised-table file, restart files and two files of more than one sequence each (64 x 48 noise at
    4:4:4 and at q100) side by side at 16-byte chunks; twice: the bytes are the same every time."""
    names = [f"{h}x{w}-{s}-{k}" for h, w, s, k in MIXED]
    datas = [C.file_bytes(*p) for p in MIXED]
    refs = [_reference(n, d) for n, d in zip(names, datas)]
    images, status, twin, packed = _decode(dev, [p for p, _ in refs], datas, 16)
    assert packed.tables.shape[0] >= 4 and len(packed.segments) > len(MIXED) and J.sequences(packed) >= 4
    for k in (2, 7):
        alone = J.pack([refs[k][0]], [datas[k]], chunk_bytes=16)
        assert J.sequences(alone) >= 2, names[k]
    assert np.array_equal(status, twin) and not status.any(), (status.tolist(), twin.tolist())
    for n, got, (_, want) in zip(names, images, refs):
        assert np.array_equal(got, want), n
    again, _, _, _ = _decode(dev, [p for p, _ in refs], datas, 16)
    for a, b in zip(images, again):
        assert np.array_equal(a, b)


def test_one_pass_reports_the_unsynced_images_the_host_twin_reports(dev):
    """passes = 1 on the mixed launch: a sequence that starts inside a segment starts from a guess, so images come back UNSYNCED — the very
    images, with the very status words, the host twin reports; every image whose status is zero has exact pixels."""
    names = [f"{h}x{w}-{s}-{k}" for h, w, s, k in MIXED]
    datas = [C.file_bytes(*p) for p in MIXED]
    refs = [_reference(n, d) for n, d in zip(names, datas)]
    images, status, twin, _ = _decode(dev, [p for p, _ in refs], datas, 16, passes=1)
    assert np.array_equal(status, twin), (status.tolist(), twin.tolist())
    assert (status & UNSYNCED).any() and not status.all(), status.tolist()
    for n, got, st, (_, want) in zip(names, images, status, refs):
        assert st != 0 or np.array_equal(got, want), n


@pytest.mark.parametrize("chunk_bytes", [16, 128])
def test_damaged_scans_are_reported_and_their_neighbours_exact(dev, chunk_bytes):
    """The five damaged scans of tests/_jpeg_case.py, each between good files in ONE launch: a non-zero status for each of them — the host
    twin's —, zero for the good files, whose pixels are exact; the guards stay intact (checked in _decode)."""
    good = [("16x16-q90-444-noise", C.file_bytes(16, 16, "q90-444", "noise")), ("33x64-q90-rst-smooth", C.file_bytes(33, 64, "q90-rst", "smooth"))]
    refs = [_reference(n, d) for n, d in good]
    plans, datas, bad = [refs[0][0]], [good[0][1]], []
    for kind in C.DAMAGED:
        plan, data = C.damaged(kind)
        bad.append(len(plans))
        plans += [plan, refs[len(bad) % 2][0]]
        datas += [data, good[len(bad) % 2][1]]
    images, status, twin, _ = _decode(dev, plans, datas, chunk_bytes)
    assert np.array_equal(status, twin), (status.tolist(), twin.tolist())
    for b in range(len(plans)):
        if b in bad:
            assert status[b] != 0, (b, C.DAMAGED[bad.index(b)])
        else:
            want = refs[0][1] if plans[b] is refs[0][0] else refs[1][1]
            assert status[b] == 0 and np.array_equal(images[b], want), b


def test_a_loader_batch_through_decode_staged_equals_the_host_decoder(dev, tmp_path):
    """One batch of four files: BatchLoader(decoder="device-split") -> decode_staged gives, byte for byte, the staging buffer the host
    decoder's loader fills."""
    from zutis_amd import preprocess as P
    from zutis_amd.dropin.utils.extract_image_embeddings import resize_crop_box
    paths = []
    for k, (h, w, s, kind) in enumerate([(64, 48, "q100-420", "noise"), (37, 53, "q90-444", "smooth"), (33, 64, "q90-rst", "smooth"), (16, 16, "q85-grey", "noise")]):
        p = tmp_path / f"im{k}.jpg"
        p.write_bytes(C.file_bytes(h, w, s, kind))
        paths.append(str(p))
    (host,) = list(P.BatchLoader(paths, 24, 4, 2, resize_crop_box, pin=False))
    (batch,) = list(P.BatchLoader(paths, 24, 4, 2, resize_crop_box, pin=False, decoder="device-split"))
    assert batch.jpeg.chunks is not None and batch.jpeg.kept == [0, 1, 2, 3] and batch.n_host_decoded == 0
    staged = batch.staging.to(dev)
    full = torch.empty(host.staging.numel(), dtype=torch.uint8, device=dev)
    got = P.decode_staged(batch, staged, full)
    torch.cuda.synchronize()
    got, want = got.cpu().numpy(), host.staging.numpy()
    head = 32 * 4
    assert np.array_equal(got[:head], want[:head])
    for i in range(4):
        o, w, h = int(host.desc[i, 0]) * 16 + head, int(host.desc[i, 1]), int(host.desc[i, 2])
        assert np.array_equal(got[o:o + 3 * w * h], want[o:o + 3 * w * h]), paths[i]
