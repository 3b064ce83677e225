"""CPU: the device JPEG decoder's definition (zutis_amd/jpeg_device.py) against Pillow, the host twin of the kernels
(zh_jpeg_decode_host: the codec of csrc/jpeg_codec.h on the CPU) against the definition, what parse() refuses, the launch arrays of
pack(), damaged scans through the host codec, and the loader's decoder="device" staging decoded by the host twin."""
import dataclasses
import io

import numpy as np
import pytest
from PIL import Image, features

from tests import _jpeg_case as C
from zutis_amd import build
from zutis_amd import jpeg_device as J


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
        assert plan is not None, name
        a = J.decode_np(data, plan)
        a.setflags(write=False)
        out[name] = (data, plan, a)
    return out


def test_definition_equals_pillow(reference):
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("Pillow is not built on libjpeg-turbo: its decoder's arithmetic is not the one the definition restates")
    assert len(reference) == 16 * len(C.SIZES)
    for name, (data, plan, got) in reference.items():
        want = C.pillow(data)
        assert got.shape == want.shape and got.dtype == np.uint8, name
        assert np.array_equal(got, want), (name, int((got != want).sum()))


def test_host_codec_equals_definition(lib, reference):
    """The 16 variants of a size in one call, as the kernel gets them; then every file on its own."""
    for h, w in C.SIZES:
        names = [n for n, _ in C.variants(h, w)]
        packed = J.pack([reference[n][1] for n in names], [reference[n][0] for n in names])
        images, status = J.decode_host(packed)
        assert not status.any(), (h, w, status.tolist())
        for n, got in zip(names, images):
            assert np.array_equal(got, reference[n][2]), n
    for name, (data, plan, want) in reference.items():
        (got,), status = J.decode_host(J.pack([plan], [data]))
        assert status[0] == 0 and np.array_equal(got, want), name


def _save(a, fmt="JPEG", **kw):
    buf = io.BytesIO()
    a.save(buf, fmt, **kw)
    return buf.getvalue()


def test_parse_refuses_what_the_device_does_not_serve():
    rgb = Image.fromarray(C.pixels(24, 40, "smooth"))
    good = _save(rgb, quality=90)
    assert J.parse(good) is not None
    assert J.parse(_save(rgb, quality=90, progressive=True)) is None
    assert J.parse(_save(rgb, "PNG")) is None
    assert J.parse(_save(rgb.convert("CMYK"), quality=90)) is None
    assert J.parse(b"") is None and J.parse(b"\xff\xd8") is None and J.parse(good[:len(good) // 2]) is None
    # 4:4:0 (luma sampling (1, 2)): Pillow's encoder does not offer it, so a 4:2:2 file's frame header is rewritten
    sof = good.index(b"\xff\xc0")
    assert good[sof + 11] in (0x22, 0x21, 0x11)
    f440 = _save(rgb, quality=90, subsampling=1)
    sof = f440.index(b"\xff\xc0")
    assert f440[sof + 11] == 0x21
    assert J.parse(f440[:sof + 11] + b"\x12" + f440[sof + 12:]) is None
    # an Adobe APP14 behind the JFIF segment
    app0_end = 4 + ((good[4] << 8) | good[5])
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01"
    assert J.parse(good[:app0_end] + adobe + good[app0_end:]) is None
    # a 16-bit quantisation table, a second scan, a DNL: each leaves the file to the host
    dqt = good.index(b"\xff\xdb")
    assert J.parse(good[:dqt + 4] + bytes([good[dqt + 4] | 0x10]) + good[dqt + 5:]) is None
    assert J.parse(good[:-2] + b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00" + b"\x00\xff\xd9") is None
    assert J.parse(good[:-2] + b"\xff\xdc\x00\x04\x00\x18\xff\xd9") is None


def test_table_sets_deduplicate_and_restarts_make_segments():
    datas = [C.file_bytes(h, w, s, k) for h, w in [(16, 16), (37, 53), (64, 48)] for s in ("q90-420", "q90-444", "q90-422", "q90-rst") for k in C.KINDS]
    plans = [J.parse(d) for d in datas]
    packed = J.pack(plans, datas)
    assert packed.tables.shape == (1, J.TABLE_SET_BYTES) and not packed.images[:, 7].any()
    assert packed.kept == list(range(len(plans)))
    lengths = packed.segments[:, 2] - packed.segments[:, 1]
    assert (np.diff(lengths) <= 0).all() and lengths.sum() == packed.scan.size          # longest first, the scan bytes are theirs
    both = J.pack(plans[:2] + [J.parse(C.file_bytes(16, 16, "q75-opt", "noise"))], datas[:2] + [C.file_bytes(16, 16, "q75-opt", "noise")])
    assert both.tables.shape[0] == 2 and both.images[:, 7].tolist() == [0, 0, 1]
    for h, w in C.SIZES:
        plan = J.parse(C.file_bytes(h, w, "q90-rst", "smooth"))
        assert plan.restart_interval == (3 if plan.n_mcus > 3 else plan.restart_interval)
        want = -(-plan.n_mcus // plan.restart_interval) if plan.restart_interval else 1
        assert len(plan.segments) == want and plan.segments[:, 2].tolist() == [k * plan.restart_interval for k in range(want)], (h, w)
    assert len(J.parse(C.file_bytes(37, 53, "q90-rst", "smooth")).segments) == 4          # 12 MCUs of 16 x 16, a marker every 3


def test_pack_leaves_out_what_exceeds_a_launch():
    """More distinct table sets than a launch holds: an error, or — as the loader asks — the surplus images left to the host."""
    base = J.parse(C.file_bytes(8, 9, "q90-444", "noise"))
    data = C.file_bytes(8, 9, "q90-444", "noise")
    plans = []
    for k in range(J.MAX_TABLE_SETS + 3):
        q = base.quant.copy()
        q[0, 63] = 1 + k
        plans.append(dataclasses.replace(base, quant=q))
    with pytest.raises(ValueError, match="table sets"):
        J.pack(plans, [data] * len(plans))
    packed = J.pack(plans + [plans[0]], [data] * (len(plans) + 1), skip_overflow=True)
    assert packed.kept == list(range(J.MAX_TABLE_SETS)) + [len(plans)] and packed.tables.shape[0] == J.MAX_TABLE_SETS
    assert packed.images.shape[0] == len(packed.kept) and packed.images[-1, 7] == 0


@pytest.mark.parametrize("kind", C.DAMAGED)
def test_damaged_scans_set_a_status_and_write_nothing_else(lib, kind):
    """The host codec on a damaged scan between two good files: a non-zero status for it, zero and exact pixels for its neighbours,
    no exception, and not one byte outside the three images (the output is carved out of a sentinel-filled buffer)."""
    import ctypes
    good = C.file_bytes(16, 16, "q90-444", "noise")
    plan, data = C.damaged(kind)
    with pytest.raises(J.DamagedScan):
        J.decode_np(data, plan)
    packed = J.pack([J.parse(good), plan, J.parse(good)], [good, data, good])
    pad = 4096
    buf = np.full(packed.out_bytes + 2 * pad, 0xA5, np.uint8)
    status = np.full(3 + 2, 0x5A5A5A5A, np.int32)
    ptr = lambda a, off=0: ctypes.c_void_p(a.ctypes.data + off)      # noqa: E731
    rc = lib.zh_jpeg_decode_host(ptr(packed.scan), packed.scan.size, ptr(packed.segments), len(packed.segments), ptr(packed.images), 3,
                                 ptr(packed.tables), len(packed.tables), packed.n_blocks, ptr(buf, pad), packed.out_bytes, ptr(status, 4))
    assert rc == 0
    assert status[0] == 0x5A5A5A5A and status[4] == 0x5A5A5A5A and status[1] == 0 and status[3] == 0 and status[2] != 0, status.tolist()
    assert (buf[:pad] == 0xA5).all() and (buf[-pad:] == 0xA5).all()
    images = J.unpack(packed, buf[pad:pad + packed.out_bytes])
    assert np.array_equal(images[0], C.pillow(good)) and np.array_equal(images[2], C.pillow(good))
    gap = buf[pad + int(packed.out_off[0]) + 3 * 16 * 16:pad + int(packed.out_off[1])]
    assert (gap == 0xA5).all()
    want = {"cut": "truncated", "ff00": "code", "marker": "marker", "zeros": "truncated", "dri": "incomplete"}[kind]
    assert status[2] & J.STATUS[want], (kind, int(status[2]))


def test_descriptors_that_do_not_fit_are_refused(lib):
    """Rows that lie about sizes, offsets, table sets, block ranges or segment ranges: DESCRIPTOR / SEGMENT, nothing written."""
    data = C.file_bytes(33, 64, "q90-420", "smooth")
    plan = J.parse(data)
    base = J.pack([plan], [data])
    for col, value in ((0, 65), (1, 0), (2, 2), (3, 3), (5, 1), (7, 1), (8, 1), (9, 1), (10, -1)):
        packed = dataclasses.replace(base, images=base.images.copy())
        packed.images[0, col] = value
        (got,), status = J.decode_host(packed)
        assert status[0] & J.STATUS["descriptor"] and not got.any(), (col, value)
    for col, value in ((1, -1), (2, base.scan.size + 1), (3, plan.n_mcus), (3, 1), (0, 1)):
        packed = dataclasses.replace(base, segments=base.segments.copy())
        packed.segments[0, col] = value
        _, status = J.decode_host(packed)
        assert status[0] != 0, (col, value)


def test_check_decoder():
    assert J.check_decoder("x", "host") == "host" and J.check_decoder("x", "device") == "device"
    with pytest.raises(ValueError, match="decoder"):
        J.check_decoder("x", "gpu")


def test_loader_stages_file_bytes_for_the_device_decoder(lib, tmp_path):
    """BatchLoader(decoder="device") on the CPU: the staging buffer holds the launch arrays of the served files and the pixels of the
    others; the host twin over those very views gives every served image, the host-decoded ones already lie in the staged bytes, and
    the descriptor rows are those of the host decoder's batch."""
    import torch
    from zutis_amd import preprocess as P
    from zutis_amd.dropin.utils.extract_image_embeddings import resize_crop_box
    paths = []
    for k, (h, w, s) in enumerate([(37, 53, "q90-420"), (64, 48, "q90-444"), (33, 64, "q90-rst"), (16, 16, "q85-grey"), (9, 5, "q75-opt")]):
        p = tmp_path / f"im{k}.jpg"
        p.write_bytes(C.file_bytes(h, w, s, "smooth"))
        paths.append(str(p))
    rgb = Image.fromarray(C.pixels(40, 30, "smooth"))
    rgb.save(tmp_path / "prog.jpg", quality=90, progressive=True)
    rgb.save(tmp_path / "plain.png")
    paths[2:2] = [str(tmp_path / "prog.jpg")]
    paths.append(str(tmp_path / "plain.png"))
    host = list(P.BatchLoader(paths, 24, 4, 3, resize_crop_box, pin=False))
    batches = P.BatchLoader(paths, 24, 4, 3, resize_crop_box, pin=False, decoder="device")
    seen = 0
    for hb, b in zip(host, batches):
        B, j = len(b.paths), b.jpeg
        assert b.paths == hb.paths and b.packed is None and torch.equal(b.desc, hb.desc) and b.packed_bytes == hb.packed_bytes and b.kmax == hb.kmax
        assert b.staging.numel() == 32 * B + j.staged_bytes
        pay = b.staging[32 * B:].numpy()
        part = lambda place, dtype, cols: pay[place[0]:place[0] + place[1]].view(dtype).reshape(-1, cols)      # noqa: E731
        out_off = part(j.images, np.int32, J.IMAGE_WORDS)[:, 9].astype(np.int64) * 16
        packed = J.Packed(pay[j.scan[0]:j.scan[0] + j.scan[1]].copy(), part(j.segments, np.int32, J.SEGMENT_WORDS).copy(),
                          part(j.images, np.int32, J.IMAGE_WORDS).copy(), part(j.tables, np.uint8, J.TABLE_SET_BYTES).copy(), out_off, b.packed_bytes,
                          j.n_blocks, [(int(b.desc[i, 2]), int(b.desc[i, 1])) for i in j.kept], j.max_image_blocks, j.max_image_pixels)
        images, status = J.decode_host(packed)
        assert not status.any()
        want = hb.packed.numpy()
        for i, got in zip(j.kept, images):
            o, w, h = int(b.desc[i, 0]) * 16, int(b.desc[i, 1]), int(b.desc[i, 2])
            assert np.array_equal(got.reshape(-1), want[o:o + 3 * w * h]), b.paths[i]
        for i, at, n, slot in j.host:
            assert np.array_equal(pay[at:at + n], want[slot:slot + n]), b.paths[i]
        assert sorted(j.kept + [i for i, _, _, _ in j.host]) == list(range(B))
        assert b.n_host_decoded == len(j.host) and b.host_decoded_paths == [b.paths[i] for i, _, _, _ in j.host]
        seen += b.n_host_decoded
    assert seen == 2
    with pytest.raises(ValueError, match="decoder"):
        P.BatchLoader(paths, 24, 4, 3, resize_crop_box, pin=False, decoder="gpu")
