"""CPU: the device JPEG encoder's definition (zutis_amd/jpeg_device.py encode_np) against Pillow's file byte for byte, the constructed
pictures' entropy edges, the file read back by the decoder's definition, scan_bound, the host twin of the kernels
(zh_jpeg_encode_host: the codec of csrc/jpeg_codec.h on the CPU) against the definition, the picture stage's host arm on CPU tensors
and the argument checks of predict_from_files."""
import os
import threading

import numpy as np
import pytest
from PIL import Image

from tests import _jpeg_case as C
from tests import _jpeg_enc_case as E
from zutis_amd import build
from zutis_amd import jpeg_device as J
from zutis_amd import picture_out as PO

needs_pillow = pytest.mark.skipif(not E.pillow_has_restart_blocks(), reason="the installed Pillow does not know restart_marker_blocks")


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)        # hipcc cross-compiles gfx950 without a GPU; the host entry needs none
    from zutis_amd import _lib
    return _lib.load(raw=True)


@needs_pillow
@pytest.mark.parametrize("subsampling", E.SUBSAMPLINGS)
@pytest.mark.parametrize("quality", E.QUALITIES)
def test_definition_equals_pillows_file(quality, subsampling):
    ref = E.cases(quality, subsampling)
    assert len(ref) >= 2 * (len(C.SIZES) + 1)
    for name, a, scan in ref:
        want = E.pillow_file(a, quality, subsampling)
        got = J.encode_np(a, quality, subsampling)
        assert got == want, (name, quality, subsampling, len(got), len(want))
        head = J.header_bytes(a.shape[0], a.shape[1], quality, subsampling)
        assert got == head + scan + b"\xff\xd9"


def test_the_wrap_sizes_have_more_than_eight_intervals():
    for subsampling, (h, w) in E.WRAP.items():
        scan = E.named(90, subsampling, f"{h}x{w}-smooth")[1]
        assert sum(scan.count(bytes([0xFF, 0xD0 + n])) > 0 for n in range(8)) == 8
        plan = J.parse(J.encode_np(C.pixels(h, w, "smooth"), 90, subsampling))
        assert len(plan.segments) > 9 and plan.restart_interval == J.ENC_INTERVAL_MCUS


def test_header_is_pillows_marker_order():
    head = J.header_bytes(40, 40, 90, "4:2:0")
    at, seen = 2, []
    while at < len(head):
        assert head[at] == 0xFF
        n = int.from_bytes(head[at + 2:at + 4], "big")
        seen.append((head[at + 1], n))
        at += 2 + n
    assert head[:2] == b"\xff\xd8" and at == len(head)
    assert seen == [(0xE0, 16), (0xDB, 67), (0xDB, 67), (0xC0, 17), (0xC4, 31), (0xC4, 181), (0xC4, 31), (0xC4, 181), (0xDD, 4), (0xDA, 12)]
    assert head[6:20] == b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"


def test_quant_tables_follow_libjpegs_scaling():
    base = J.quant_tables(50)
    assert base[0, :4].tolist() == [16, 11, 10, 16] and base[1, :4].tolist() == [17, 18, 24, 47]
    assert (J.quant_tables(100) == 1).all() and J.quant_tables(1).max() == 255 and J.quant_tables(1).min() == 255
    assert J.quant_tables(75)[0, 0] == (16 * 50 + 50) // 100 and J.quant_tables(25)[0, 1] == (11 * 200 + 50) // 100


def _blocks_of(a, quality, subsampling):
    """The zig-zag coefficient blocks of encode_np(a), read back by the decoder's definition: [MCUs, blocks per MCU, 64]."""
    data = J.encode_np(a, quality, subsampling)
    plan = J.parse(data)
    coef = np.asarray(J.decode_coefficients(plan, data)).reshape(-1, 64)[:, J.ZIGZAG]
    bpm = 6 if subsampling == "4:2:0" else 3
    assert np.array_equal(coef, J.encode_coefficients(a, quality, subsampling))
    return coef.reshape(-1, bpm, 64)


@pytest.mark.parametrize("subsampling", E.SUBSAMPLINGS)
def test_constructed_pictures_reach_the_entropy_edges(subsampling):
    pics = E.constructed()
    lum = 4 if subsampling == "4:2:0" else 1
    for name in ("black", "white"):                                          # every block is EOB, every DC difference 0 but the first
        a, q = pics[name]
        blocks = _blocks_of(a, q, subsampling)
        assert not blocks[:, :, 1:].any() and (blocks[:, :, 0] == blocks[0, :, 0]).all()
        scan = J.scan_np(a, q, subsampling, interval_mcus=65535)
        first = J.scan_np(a[:8 * (2 if lum == 4 else 1), :8 * (2 if lum == 4 else 1)], q, subsampling)
        assert len(scan) < len(first) + blocks.shape[0] * blocks.shape[1]   # DC category 0 and EOB: 2 + 4 bits a luma block, 2 + 2 a chroma block
    a, q = pics["checker"]
    blocks = _blocks_of(a, q, subsampling)
    luma = blocks[:, :lum].reshape(-1, 64)
    assert np.abs(np.diff(luma[:, 0])).max() >= 1024 and np.abs(luma[:, 1:]).max() >= 512      # DC category 11, AC category 10
    a, q = pics["ff"]
    assert b"\xff\x00" in J.scan_np(a, q, subsampling)
    a, q = pics["zrl"]
    blocks = _blocks_of(a, q, subsampling)
    (k,) = np.flatnonzero(blocks[0, 0, 1:]) + 1
    assert k >= 17 and blocks[0, 0, 63] == 0                                # a lone coefficient behind 16 or more zeros: ZRL, then EOB
    a, q = pics["coef63"]
    blocks = _blocks_of(a, q, subsampling)
    assert (np.flatnonzero(blocks[0, 0, 1:]) + 1).tolist() == [63]          # three ZRLs and no EOB


@needs_pillow
@pytest.mark.parametrize("subsampling", E.SUBSAMPLINGS)
def test_the_file_parses_as_defined_and_decodes_to_pillows_pixels(subsampling):
    for name, a, _ in E.cases(90, subsampling):
        data = J.encode_np(a, 90, subsampling)
        plan = J.parse(data)
        assert plan is not None and plan.restart_interval == J.ENC_INTERVAL_MCUS and plan.ncomp == 3, name
        assert (plan.width, plan.height) == (a.shape[1], a.shape[0]) and (plan.hs, plan.vs) == ((2, 2) if subsampling == "4:2:0" else (1, 1))
        assert np.array_equal(np.asarray(plan.quant).reshape(2, 64), J.quant_tables(90))
        assert [(tuple(c), bytes(v)) for c, v in plan.huff] == [(c, v) for c, v in J.ANNEX_K_HUFF]
        assert np.array_equal(J.decode_np(data, plan), C.pillow(data)), name


@pytest.mark.parametrize("subsampling", E.SUBSAMPLINGS)
def test_scan_bound_holds_and_is_nearly_reached(subsampling):
    for q in E.QUALITIES:
        for name, a, scan in E.cases(q, subsampling):
            assert len(scan) <= J.scan_bound(a.shape[0], a.shape[1], subsampling), (name, q)
    a, scan = E.overflow()
    assert J.scan_slot(64, 64) < len(scan) <= J.scan_bound(64, 64, "4:4:4")
    # the docstring's construction: DC alternating between -1024 and 1023, every AC +-1023, 40 MCUs (two full intervals and a part)
    bpm, lum = (6, 4) if subsampling == "4:2:0" else (3, 1)
    mcus = 40
    blocks = np.where(np.arange(64)[None, :] % 2 == 0, 1023, -1023) * np.ones((mcus * bpm, 1), np.int64)
    m, j = np.arange(mcus * bpm) // bpm, np.arange(mcus * bpm) % bpm
    blocks[:, 0] = np.where(np.where(j < lum, m * lum + j, m) % 2 == 0, -1024, 1023)       # alternating along every component's own sequence
    comp_dc = blocks.reshape(mcus, bpm, 64)[:, :, 0]
    assert (np.abs(np.diff(comp_dc[:, lum:], axis=0)) == 2047).all() and (np.abs(np.diff(comp_dc[:, :lum].reshape(-1))) == 2047).all()
    got = J.scan_of_blocks(blocks, subsampling)
    h, w = (16, 16 * mcus) if subsampling == "4:2:0" else (8, 8 * mcus)
    bound, markers = J.scan_bound(h, w, subsampling), 2 * 2
    unstuffed = len(got.replace(b"\xff\x00", b"\xff")) - markers
    assert len(got) <= bound and bound == 2 * sum(-(-1660 * m * bpm // 8) for m in (16, 16, 8)) + markers
    # scan_bound's docstring: 1658 bits a luma block, 1408 a chroma block, at most 6 bits an interval less
    assert unstuffed >= sum(-(-(m * (1658 * lum + 2 * 1408) - 6) // 8) for m in (16, 16, 8))
    assert unstuffed <= sum(-(-(m * (1658 * lum + 2 * 1408)) // 8) for m in (16, 16, 8))


def test_scan_slot_is_the_raw_picture_and_the_headers_extra():
    assert J.scan_slot(480, 640) == 480 * 640 * 3 + 1024 == 480 * 640 * 3 + J.ENC_SLOT_EXTRA


# ---- the host twin

@pytest.mark.parametrize("subsampling", E.SUBSAMPLINGS)
@pytest.mark.parametrize("quality", E.QUALITIES)
def test_host_twin_equals_the_definition(lib, quality, subsampling):
    ref = E.cases(quality, subsampling)
    out, lengths = J.scan_host([a for _, a, _ in ref], quality, subsampling)
    for k, (name, a, want) in enumerate(ref):
        n = min(len(want), out.shape[1])                                    # (noise at quality 100 is longer than the launch's slot)
        assert lengths[k] == len(want) and out[k, :n].tobytes() == want[:n], (name, lengths[k], len(want))
        assert (out[k, n:] == 0xA5).all(), name


def test_host_twin_reports_the_true_length_of_a_scan_that_overflows_and_refuses_what_does_not_fit(lib):
    import ctypes
    a, want = E.overflow()
    slot = J.scan_slot(64, 64)
    small, small_scan = E.named(100, "4:4:4", "9x5-smooth")
    out, lengths = J.scan_host([small, a, small], 100, "4:4:4", slot_bytes=slot)
    assert lengths.tolist() == [len(small_scan), len(want), len(small_scan)] and len(want) > slot
    assert out[1].tobytes() == want[:slot] and out[2, :len(small_scan)].tobytes() == small_scan and (out[2, len(small_scan):] == 0xA5).all()
    pixels, img_off, hw, out_off, slot, max_mcus = J.pack_pictures([small, a])
    quant = J.quant_tables(90).astype(np.uint16)
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    for case, (off1, out_bytes, mcus) in {"grid": (img_off[1], 2 * slot, 63), "out": (img_off[1], 2 * slot - 1, 64), "images": (img_off[1] + 1, 2 * slot, 64)}.items():
        buf, n = np.full(2 * slot, 0xA5, np.uint8), np.full(2, 77, np.int32)
        off = np.asarray([0, off1], np.int64)
        assert lib.zh_jpeg_encode_host(ptr(pixels), pixels.size, ptr(off), ptr(hw), 2, 0, mcus, ptr(quant), ptr(out_off), ptr(buf), out_bytes, slot, ptr(n)) == 0
        got = J.scan_np(small, 90, "4:4:4")
        assert n.tolist() == [len(got), -1] and buf[:len(got)].tobytes() == got and (buf[len(got):] == 0xA5).all(), case
    assert lib.zh_jpeg_encode_host(ptr(pixels), pixels.size, ptr(img_off), ptr(hw), 2, 1, max_mcus, ptr(quant), ptr(out_off), ptr(buf), 2 * slot, slot, ptr(n)) != 0


# ---- the picture stage's host arm and the arguments

def _write_threads():
    return [t for t in threading.enumerate() if t.name.startswith("zutis-write")]


@needs_pillow
def test_picture_stage_writes_jpeg_kinds_through_the_host_arm(tmp_path):
    """CPU tensors stand for the device's: a PNG label kind and a JPEG overlay kind in one layout, two batches."""
    import torch
    kinds = [(1, "L", None), (3, "JPEG", None)]
    want = {}
    with PO.PictureStage("host", False, 2, jpeg_encoder="host", jpeg_quality=80, jpeg_subsampling="4:4:4") as stage:
        for k, sizes in enumerate([[(9, 5), (9, 5)], [(33, 64)]]):
            lay = PO.Layout(sizes, kinds, "host")
            assert lay.host_bytes["host"] == lay.raw_bytes and lay.forms["host"] == ["raw"] * 2 * len(sizes) and lay.lengths["host"] is None
            paths = [str(tmp_path / f"b{k}_{b}{ext}") for ext in (".png", "_overlay.jpg") for b in range(len(sizes))]
            raw = stage.take(k, lay, paths)
            rng = np.random.default_rng(k)
            for i, (h, w, c, _, _) in enumerate(lay.pictures):
                a = rng.integers(0, 256, (h, w) if c == 1 else (h, w, c), dtype=np.uint8)
                raw[lay.raw_at[i]:lay.raw_at[i + 1]] = torch.from_numpy(a.reshape(-1))
                want[paths[i]] = a
            stage.commit()
    assert stage.jpeg_host_fallbacks == 0 and not _write_threads()
    assert sorted(os.listdir(tmp_path)) == sorted(os.path.basename(p) for p in want)
    for path, a in want.items():
        if path.endswith(".jpg"):
            assert open(path, "rb").read() == J.encode_np(a, 80, "4:4:4"), path
        else:
            with Image.open(path) as im:
                assert im.mode == "L" and np.array_equal(np.asarray(im), a)


def test_layout_lays_device_encoded_scans_out_at_scan_slot_stride():
    sizes, kinds = [(9, 5), (33, 64)], [(1, "L", None), (3, "JPEG", None), (3, "RGB", None)]
    plain = PO.Layout(sizes, [kinds[0], kinds[2]])
    assert plain.jpeg_encoder == "host" and plain.lengths["host"] is None and np.array_equal(plain.at["host"], plain.raw_at)
    lay = PO.Layout(sizes, kinds, "device")
    assert lay.forms["host"] == ["raw", "raw", "jpeg", "jpeg", "raw", "raw"] and lay.forms["device"] == ["png", "png", "jpeg", "jpeg", "png", "png"]
    for enc in ("host", "device"):
        widths = np.diff(lay.at[enc])
        assert widths[2:4].tolist() == [J.scan_slot(9, 5), J.scan_slot(33, 64)]
        assert lay.lengths[enc] % 4 == 0 and 0 <= lay.lengths[enc] - lay.at[enc][-1] < 4 and lay.host_bytes[enc] == lay.lengths[enc] + 4 * 6
    assert np.diff(PO.Layout(sizes, kinds, "host").at["device"])[2:4].tolist() == [9 * 5 * 3, 33 * 64 * 3]      # the host encodes: the raw bytes travel
    with pytest.raises(ValueError):
        PO.Layout(sizes, [(1, "JPEG", None)])


def test_the_device_jpeg_encoder_without_a_gpu_is_an_error_not_a_fallback():
    from zutis_amd import _lib
    with pytest.raises(_lib.ZutisHipError):
        PO.PictureStage("host", False, 1, jpeg_encoder="device")
    assert not _write_threads()


def test_arguments_are_refused_by_name_before_any_work(tmp_path):
    from zutis_amd import predict_files
    for kw, word in ((dict(overlay_format="jpg"), "overlay_format"), (dict(jpeg_quality=0), "jpeg_quality"), (dict(jpeg_quality=101), "jpeg_quality"),
                     (dict(jpeg_quality=90.5), "jpeg_quality"), (dict(jpeg_quality=True), "jpeg_quality"), (dict(jpeg_subsampling="4:2:2"), "jpeg_subsampling"),
                     (dict(jpeg_subsampling=2), "jpeg_subsampling"), (dict(jpeg_encoder="gpu"), "jpeg_encoder")):
        with pytest.raises(ValueError, match=word):
            predict_files.predict_from_files(None, ["missing.jpg"], out_dir=str(tmp_path / "never"), **kw)
    assert not os.path.exists(tmp_path / "never")
    for fn, args in ((J.encode_np, (np.zeros((8, 8, 3), np.uint8), 0)), (J.scan_np, (np.zeros((8, 8, 3), np.uint8), 90, "4:1:1")),
                     (J.encode_np, (np.zeros((8, 8), np.uint8),)), (J.encode_np, (np.zeros((8, 8, 3), np.float32),)), (J.header_bytes, (0, 8)),
                     (J.scan_np, (np.zeros((8, 8, 3), np.uint8), 90, "4:2:0", 0)), (J.scan_of_blocks, (np.zeros((5, 64), np.int16),)),
                     (J.scan_of_blocks, (np.full((3, 64), 1024, np.int16), "4:4:4"))):
        with pytest.raises(ValueError):
            fn(*args)
    assert J.pillow_writes_restart_blocks() == E.pillow_has_restart_blocks()
