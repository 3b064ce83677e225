"""CPU: the device JPEG decoder with every scan split among lanes (decoder "device-split").  The chunk rows of jpeg_device.chunk_rows
against a byte-by-byte count; the host twin of the kernels (zh_jpeg_decode_split_host: the passes of zh_jpeg_decode_split with the
functions of csrc/jpeg_codec.h, lanes as loops) against jpeg_device.decode_np on the whole corpus; one synchronising pass where two are
needed; damaged scans and lying chunk rows inside a sentinel-filled buffer; the loader's decoder="device-split" staging decoded by the
host twin."""
import ctypes
import dataclasses

import numpy as np
import pytest

from tests import _jpeg_case as C
from zutis_amd import build
from zutis_amd import jpeg_device as J

PAD = 4096


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)        # hipcc cross-compiles gfx950 without a GPU; the host entry needs none
    from zutis_amd import _lib
    return _lib.load(raw=True)


@pytest.fixture(scope="module")
def reference():
    """{name: (file bytes, plan, decode_np)} of the whole corpus: computed once, shared, never written."""
    out = {}
    for name, data in C.corpus():
        plan = J.parse(data)
        a = J.decode_np(data, plan)
        a.setflags(write=False)
        out[name] = (data, plan, a)
    return out


def _split(lib, packed, chunks, chunk_bytes, passes):
    """zh_jpeg_decode_split_host with the output and the status array carved out of sentinel-filled buffers -> (images, status); asserts
    that the call returned 0 and that no byte outside the images' pixels and the status words was written."""
    B = len(packed.shapes)
    buf = np.full(packed.out_bytes + 2 * PAD, 0xA5, np.uint8)
    status = np.full(B + 2, 0x5A5A5A5A, np.int32)
    chunks = np.ascontiguousarray(chunks, np.int32)
    ptr = lambda a, off=0: ctypes.c_void_p(a.ctypes.data + off)      # noqa: E731
    rc = lib.zh_jpeg_decode_split_host(ptr(packed.scan), packed.scan.size, ptr(packed.segments), len(packed.segments), ptr(chunks), len(chunks),
                                       chunk_bytes, passes, ptr(packed.images), B, ptr(packed.tables), len(packed.tables), packed.n_blocks,
                                       ptr(buf, PAD), packed.out_bytes, ptr(status, 4))
    assert rc == 0
    assert status[0] == 0x5A5A5A5A and status[-1] == 0x5A5A5A5A
    assert (buf[:PAD] == 0xA5).all() and (buf[-PAD:] == 0xA5).all()
    flat = buf[PAD:PAD + packed.out_bytes]
    for b, (h, w) in enumerate(packed.shapes):
        lo = int(packed.out_off[b]) + 3 * h * w
        hi = int(packed.out_off[b + 1]) if b + 1 < B else packed.out_bytes
        assert (flat[lo:hi] == 0xA5).all(), f"image {b}: bytes behind its pixels were written"
    return J.unpack(packed, flat), status[1:-1].copy()


def _segments_only(scan: bytes, segments):
    """A Packed that holds nothing but scan bytes and segment rows: what chunk_rows reads."""
    return J.Packed(np.frombuffer(scan, np.uint8), np.asarray(segments, np.int32).reshape(-1, J.SEGMENT_WORDS), np.zeros((0, J.IMAGE_WORDS), np.int32),
                    np.zeros((0, J.TABLE_SET_BYTES), np.uint8), np.zeros(0, np.int64), 0, 0, [])


def test_chunk_rows_equal_a_count_byte_by_byte(reference):
    assert (J.CHUNK_WORDS, J.CHUNK_BYTES_MIN, J.SPLIT_LANES) == (4, 16, 256) and J.CHUNK_BYTES % 16 == 0 and 1 <= J.SPLIT_PASSES <= 64
    moved = 0
    for h, w in C.SIZES:
        names = [n for n, _ in C.variants(h, w)]
        for cb in (16, J.CHUNK_BYTES):
            packed = J.pack([reference[n][1] for n in names], [reference[n][0] for n in names], chunk_bytes=cb)
            assert packed.chunk_bytes == cb and packed.chunks.dtype == np.int32
            assert np.array_equal(packed.chunks, J.chunk_rows_np(packed, cb)), (h, w, cb)
            assert np.array_equal(packed.chunks, J.chunk_rows(packed, cb))
            lo = packed.segments[packed.chunks[:, 0], 1]
            moved += int(((packed.chunks[:, 1] - lo) % cb != 0).sum())
            assert J.pack([reference[n][1] for n in names], [reference[n][0] for n in names]).chunks is None
    assert moved > 0                                                    # cuts that fell on a stuffed byte occur in the corpus as well
    # crafted: FF 00 across the first cut (the 00 is byte 16), a pair inside a chunk, FF as a segment's last byte in front of a segment
    # that begins with 00 (no pair), a segment without bytes, a last chunk of one byte
    a = bytes(range(1, 16)) + b"\xff\x00" + bytes(range(20, 30)) + b"\xff\x00" + bytes(range(40, 44)) + b"\xff"
    b = b"\x00" + bytes(range(50, 66))
    packed = _segments_only(a + b, [[0, 0, len(a), 0], [1, len(a), len(a) + len(b), 0], [2, len(a) + len(b), len(a) + len(b), 0]])
    rows = J.chunk_rows(packed, 16)
    assert rows.tolist() == [[0, 0, 0, 1], [0, 17, 8 * 16, 0], [0, 32, 8 * 30, 0],
                             [1, 34, 0, 1], [1, 50, 8 * 16, 0],
                             [2, 51, 0, 1]]
    assert np.array_equal(rows, J.chunk_rows_np(packed, 16))
    for bad in (8, 24, 4112, 16.5):
        with pytest.raises(ValueError, match="chunk_bytes"):
            J.chunk_rows(packed, bad)


def test_first_chunk_flags_and_short_last_chunks(reference):
    data, plan, _ = reference["37x53-q90-rst-smooth"]
    packed = J.pack([plan], [data], chunk_bytes=16)
    assert len(packed.segments) == 4
    rows = packed.chunks
    firsts = np.flatnonzero(rows[:, 3])
    assert rows[firsts, 0].tolist() == [0, 1, 2, 3] and (rows[firsts, 2] == 0).all()
    assert np.array_equal(rows[firsts, 1], packed.segments[:, 1])
    assert (np.diff(rows[:, 0]) >= 0).all() and set(rows[:, 3].tolist()) == {0, 1}
    lengths = packed.segments[:, 2] - packed.segments[:, 1]
    assert np.array_equal(np.bincount(rows[:, 0]), -(-lengths // 16))
    assert (lengths % 16 != 0).any()                                     # a last chunk shorter than chunk_bytes
    for s in np.flatnonzero(lengths % 16):
        last = rows[rows[:, 0] == s][-1]
        assert 0 < packed.segments[s, 2] - last[1] < 16


def test_host_twin_equals_the_definition(lib, reference):
    """All 192 files, at the shipped chunk size and at 16 bytes.  With as many passes as the launch has sequences every state is the true
    one (after pass p the first p sequences of every segment are): status 0 and the definition's pixels, deterministically.  At the
    shipped pass count no file of the corpus may come back UNSYNCED either."""
    assert len(reference) == 192
    unsynced = []
    for name, (data, plan, want) in reference.items():
        for cb in (J.CHUNK_BYTES, 16):
            packed = J.pack([plan], [data], chunk_bytes=cb)
            (got,), status = _split(lib, packed, packed.chunks, cb, J.sequences(packed))
            assert status[0] == 0 and np.array_equal(got, want), (name, cb, int(status[0]))
            (got,), status = J.decode_split_host(packed)
            if status[0]:
                unsynced.append((name, cb, int(status[0])))
            else:
                assert np.array_equal(got, want), (name, cb)
    assert unsynced == []
    for h, w in C.SIZES:                                                 # the 16 variants of a size in one call, as the kernel gets them
        names = [n for n, _ in C.variants(h, w)]
        packed = J.pack([reference[n][1] for n in names], [reference[n][0] for n in names], chunk_bytes=16)
        images, status = _split(lib, packed, packed.chunks, 16, J.sequences(packed))
        assert not status.any(), (h, w, status.tolist())
        for n, got in zip(names, images):
            assert np.array_equal(got, reference[n][2]), n


def test_one_pass_leaves_a_two_sequence_file_unsynced(lib, reference):
    """64 x 48 noise at 4:4:4 is 360 chunks of 16 bytes: two sequences.  One pass starts the second from a guess that the hand-over check
    refuses; the second pass hands it the first sequence's last state."""
    data, plan, want = reference["64x48-q90-444-noise"]
    packed = J.pack([plan], [data], chunk_bytes=16)
    assert J.sequences(packed) == 2 and len(packed.segments) == 1
    _, status = _split(lib, packed, packed.chunks, 16, 1)
    assert status[0] & J.STATUS["unsynced"] == 256
    (got,), status = _split(lib, packed, packed.chunks, 16, 2)
    assert status[0] == 0 and np.array_equal(got, want)


@pytest.mark.parametrize("chunk_bytes", [16, J.CHUNK_BYTES])
@pytest.mark.parametrize("kind", C.DAMAGED)
def test_damaged_scans_set_a_status_and_write_nothing_else(lib, reference, kind, chunk_bytes):
    """A damaged scan between two good files: a non-zero status for it, zero and exact pixels for its neighbours, not one byte outside
    the three images (checked in _split); unless the split decoder says UNSYNCED it reports every bit the serial decoder reports."""
    good = C.file_bytes(16, 16, "q90-444", "noise")
    plan, data = C.damaged(kind)
    packed = J.pack([J.parse(good), plan, J.parse(good)], [good, data, good], chunk_bytes=chunk_bytes)
    images, status = _split(lib, packed, packed.chunks, chunk_bytes, J.sequences(packed))
    assert status[0] == 0 and status[2] == 0 and status[1] != 0, status.tolist()
    want = reference["16x16-q90-444-noise"][2]
    assert np.array_equal(images[0], want) and np.array_equal(images[2], want)
    _, serial = J.decode_host(packed)
    assert serial[0] == 0 and serial[2] == 0 and serial[1] != 0
    if not status[1] & J.STATUS["unsynced"]:
        assert serial[1] & ~status[1] == 0, (kind, int(serial[1]), int(status[1]))


def test_lying_chunk_rows_are_refused(lib, reference):
    """A wrong offset, a wrong segment, an unstuffed count off by 8, a flag cleared on a first chunk or set inside a segment, a row
    left out: a non-zero status for the image (DESCRIPTOR where the row itself does not fit), zero and exact pixels for the others,
    nothing written elsewhere (checked in _split)."""
    names = ["16x16-q90-444-noise", "64x48-q90-420-noise", "33x64-q90-rst-smooth"]
    packed = J.pack([reference[n][1] for n in names], [reference[n][0] for n in names], chunk_bytes=16)
    rows = packed.chunks
    image_of = packed.segments[rows[:, 0], 0]
    mine = np.flatnonzero(image_of == 1)
    assert len(mine) > 8 and rows[mine[0], 3] == 1 and len(np.unique(rows[mine, 0])) == 1
    images, status = _split(lib, packed, rows, 16, J.sequences(packed))
    assert not status.any() and all(np.array_equal(g, reference[n][2]) for g, n in zip(images, names))
    other = int(rows[np.flatnonzero(image_of == 2)[0], 0])
    lies = {"offset": (mine[3], 1, rows[mine[3], 1] + 1), "offset far": (mine[3], 1, packed.scan.size + 5), "offset back": (mine[3], 1, rows[mine[2], 1]),
            "segment": (mine[3], 0, other), "segment outside": (mine[3], 0, len(packed.segments)), "unstuffed + 8": (mine[3], 2, rows[mine[3], 2] + 8),
            "unstuffed - 8": (mine[3], 2, rows[mine[3], 2] - 8), "unstuffed + 1": (mine[3], 2, rows[mine[3], 2] + 1), "first cleared": (mine[0], 3, 0),
            "first set": (mine[3], 3, 1), "flag 2": (mine[3], 3, 2)}
    for what, (i, col, value) in lies.items():
        bad = rows.copy()
        bad[i, col] = value
        images, status = _split(lib, packed, bad, 16, J.sequences(packed))
        assert status[1] != 0, what
        if what not in ("segment outside",):
            assert status[1] & J.STATUS["descriptor"], (what, int(status[1]))
        assert status[0] == 0 and np.array_equal(images[0], reference[names[0]][2]), what
        if what != "segment":                                             # (the row then claims a place in image 2's segment)
            assert status[2] == 0 and np.array_equal(images[2], reference[names[2]][2]), what
    images, status = _split(lib, packed, np.delete(rows, mine[-1], axis=0), 16, J.sequences(packed))      # the last chunk left out
    assert status[1] != 0 and status[0] == 0 and status[2] == 0
    images, status = _split(lib, packed, np.delete(rows, mine[3], axis=0), 16, J.sequences(packed))       # a chunk inside left out
    assert status[1] & J.STATUS["descriptor"] and status[0] == 0 and status[2] == 0
    for cb, passes in ((8, 1), (24, 1), (4112, 1), (16, 0), (16, 65)):                                    # arguments outside their ranges
        assert lib.zh_jpeg_decode_split_host(None, 0, None, 0, None, 0, cb, passes, None, 1, None, 1, 1, None, 0, None) != 0


def test_check_decoder_and_status_names():
    assert J.DECODERS == ("host", "device", "device-split") and J.check_decoder("x", "device-split") == "device-split"
    assert J.STATUS["unsynced"] == 256 and len(set(J.STATUS.values())) == len(J.STATUS)
    with pytest.raises(ValueError, match="decoder"):
        J.check_decoder("x", "split")


def test_loader_stages_chunk_rows_for_the_split_decoder(lib, tmp_path):
    """BatchLoader(decoder="device-split") on the CPU: the staging buffer holds what decoder="device" stages and, behind the scan bytes,
    the chunk rows at the shipped chunk size; the host twin over those very views gives every served image."""
    import torch
    from PIL import Image
    from zutis_amd import preprocess as P
    from zutis_amd.dropin.utils.extract_image_embeddings import resize_crop_box
    paths = []
    for k, (h, w, s) in enumerate([(37, 53, "q90-420"), (64, 48, "q100-420"), (33, 64, "q90-rst"), (16, 16, "q85-grey"), (9, 5, "q75-opt")]):
        p = tmp_path / f"im{k}.jpg"
        p.write_bytes(C.file_bytes(h, w, s, "noise"))
        paths.append(str(p))
    Image.fromarray(C.pixels(40, 30, "smooth")).save(tmp_path / "prog.jpg", quality=90, progressive=True)
    paths[2:2] = [str(tmp_path / "prog.jpg")]
    host = list(P.BatchLoader(paths, 24, 4, 3, resize_crop_box, pin=False))
    serial = list(P.BatchLoader(paths, 24, 4, 3, resize_crop_box, pin=False, decoder="device"))
    seen = 0
    for hb, sb, b in zip(host, serial, P.BatchLoader(paths, 24, 4, 3, resize_crop_box, pin=False, decoder="device-split")):
        B, j = len(b.paths), b.jpeg
        assert b.paths == hb.paths and b.packed is None and torch.equal(b.desc, hb.desc) and b.packed_bytes == hb.packed_bytes
        assert sb.jpeg.chunks is None and j.chunks is not None and j.kept == sb.jpeg.kept and j.scan == sb.jpeg.scan
        assert b.staging.numel() == 32 * B + j.staged_bytes and j.chunks[0] >= j.scan[0] + j.scan[1]
        pay = b.staging[32 * B:].numpy()
        part = lambda place, dtype, cols: pay[place[0]:place[0] + place[1]].view(dtype).reshape(-1, cols)      # noqa: E731
        out_off = part(j.images, np.int32, J.IMAGE_WORDS)[:, 9].astype(np.int64) * 16
        packed = J.Packed(pay[j.scan[0]:j.scan[0] + j.scan[1]].copy(), part(j.segments, np.int32, J.SEGMENT_WORDS).copy(),
                          part(j.images, np.int32, J.IMAGE_WORDS).copy(), part(j.tables, np.uint8, J.TABLE_SET_BYTES).copy(), out_off, b.packed_bytes,
                          j.n_blocks, [(int(b.desc[i, 2]), int(b.desc[i, 1])) for i in j.kept], j.max_image_blocks, j.max_image_pixels)
        chunks = part(j.chunks, np.int32, J.CHUNK_WORDS).copy()
        assert np.array_equal(chunks, J.chunk_rows(packed, J.CHUNK_BYTES))
        packed = dataclasses.replace(packed, chunks=chunks, chunk_bytes=J.CHUNK_BYTES)
        images, status = J.decode_split_host(packed)
        assert not status.any()
        want = hb.packed.numpy()
        for i, got in zip(j.kept, images):
            o, w, h = int(b.desc[i, 0]) * 16, int(b.desc[i, 1]), int(b.desc[i, 2])
            assert np.array_equal(got.reshape(-1), want[o:o + 3 * w * h]), b.paths[i]
        for i, at, n, slot in j.host:
            assert np.array_equal(pay[at:at + n], want[slot:slot + n]), b.paths[i]
        seen += b.n_host_decoded
    assert seen == 1
