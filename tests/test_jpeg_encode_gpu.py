"""-m gpu: the device JPEG encoder.  zh_jpeg_encode (csrc/jpeg_enc.hip) against zutis_amd/jpeg_device.scan_np byte for byte — every
size, content kind, quality and subsampling of tests/_jpeg_enc_case.py and its constructed pictures, one image a launch and five of
mixed sizes, inside guard bands —, the true length of a scan that overflows its slot, and jpeg_device.encode_device's files."""
import numpy as np
import pytest
import torch

from tests import _guard as G
from tests import _jpeg_enc_case as E
from zutis_amd import jpeg_device as J

pytestmark = pytest.mark.gpu


def _encode(dev, imgs, quality, subsampling, slot_bytes=None):
    """ops.jpeg_encode over `imgs` as ONE launch, inputs and outputs carved out of guard arenas -> (out u8 [B, slot], lengths)."""
    from zutis_amd import ops
    pixels, img_off, hw, out_off, slot, max_mcus = J.pack_pictures(imgs, slot_bytes)
    B, sub = len(imgs), J.SUBSAMPLINGS[subsampling]
    ws_bytes = ops._lib.load(raw=True).zh_jpeg_encode_workspace_size(B, max_mcus, sub)
    assert ws_bytes > 0
    ain, aout = G.Arena(G.IN_FILL, dev), G.Arena(G.OUT_FILL, dev)
    v_img = ain.add("images", torch.uint8, 1, pixels.size, tail_rows=0)
    v_out = aout.add("out", torch.uint8, 1, B * slot, tail_rows=0)
    v_len = aout.add("lengths", torch.int32, 1, B, tail_rows=0)
    v_ws = aout.workspace("workspace", ws_bytes)
    v_img.put(torch.from_numpy(pixels).to(dev))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    ops.jpeg_encode(v_img.m2.reshape(-1), up(img_off), up(hw), sub, J.quant_tensor(quality, dev), v_out.m2.reshape(-1), up(out_off), slot,
                    v_len.m2.reshape(-1), max_mcus, workspace=v_ws.m2.reshape(-1))
    torch.cuda.synchronize()
    G.assert_untouched(aout)                                               # nothing outside out, lengths and the workspace
    return v_out.get().numpy().reshape(B, slot), v_len.get().numpy().reshape(-1)


def _check(out, lengths, wants, names):
    for k, want in enumerate(wants):
        n, slot = int(lengths[k]), out.shape[1]
        assert n == len(want), (names[k], n, len(want))
        assert out[k, :min(n, slot)].tobytes() == want[:slot], names[k]
        assert (out[k, min(n, slot):] == G.OUT_FILL).all(), f"{names[k]}: bytes behind its scan were written"


@pytest.mark.parametrize("subsampling", E.SUBSAMPLINGS)
@pytest.mark.parametrize("quality", E.QUALITIES)
def test_kernel_equals_the_definition(dev, quality, subsampling):
    """Launches of five images of mixed sizes (the grids are as wide as the largest), the rest one image a launch; the first launch
    twice: the bytes are the same every time."""
    ref = E.cases(quality, subsampling)
    order = sorted(range(len(ref)), key=lambda i: (i % 5, -ref[i][1].size))      # a large image first, 1 x 1 between larger ones
    launches = [order[i:i + 5] for i in range(0, len(order) - len(order) % 5, 5)] + [[i] for i in order[len(order) - len(order) % 5:]] + [[order[0]]]
    assert {len(g) for g in launches} == {1, 5}
    for g in launches:
        out, lengths = _encode(dev, [ref[i][1] for i in g], quality, subsampling)
        _check(out, lengths, [ref[i][2] for i in g], [ref[i][0] for i in g])
    again, _ = _encode(dev, [ref[i][1] for i in launches[0]], quality, subsampling)
    first, _ = _encode(dev, [ref[i][1] for i in launches[0]], quality, subsampling)
    assert np.array_equal(again, first)


def test_a_scan_longer_than_its_slot_reports_its_true_length(dev):
    a, want = E.overflow()
    slot = J.scan_slot(*a.shape[:2])
    assert len(want) > slot                                                  # the case is one: checked on the CPU first
    small = E.named(100, "4:4:4", "9x5-smooth")
    out, lengths = _encode(dev, [small[0], a, small[0]], E.OVERFLOW["quality"], E.OVERFLOW["subsampling"], slot_bytes=slot)
    _check(out, lengths, [small[1], want, small[1]], ["9x5-smooth", "overflow", "9x5-smooth"])
    assert lengths[1] == len(want) > slot and out[1].tobytes() == want[:slot]


def test_an_image_that_does_not_fit_is_left_alone(dev):
    """Too few MCUs in the grid, a slot outside out, bytes outside images: length -1, nothing written, the neighbour whole."""
    from zutis_amd import ops
    (small, want), (big, _) = E.named(90, "4:2:0", "8x9-noise"), E.named(90, "4:2:0", "200x200-smooth")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)          # noqa: E731
    pixels, img_off, hw, out_off, slot, max_mcus = J.pack_pictures([small, big])
    assert max_mcus == 625 and len(want) < slot
    for case, (off1, out_bytes, mcus) in {"grid": (img_off[1], 2 * slot, 168), "out": (img_off[1], 2 * slot - 1, 169), "images": (img_off[1] + 1, 2 * slot, 169)}.items():
        out = torch.full((2 * slot,), G.OUT_FILL, dtype=torch.uint8, device=dev)
        lengths = torch.full((2,), 77, dtype=torch.int32, device=dev)
        ops.jpeg_encode(up(pixels), up(np.asarray([0, off1], np.int64)), up(hw), 2, J.quant_tensor(90, dev), out[:out_bytes], up(out_off), slot, lengths, mcus)
        got, flat = lengths.cpu().numpy(), out.cpu().numpy()
        assert got.tolist() == [len(want), -1], case
        assert flat[:len(want)].tobytes() == want and (flat[len(want):] == G.OUT_FILL).all(), case
    with pytest.raises(ops._lib.ZutisHipError):
        ops.jpeg_encode(up(pixels), up(img_off), up(hw), 1, J.quant_tensor(90, dev), out, up(out_off), slot, lengths, max_mcus)


@pytest.mark.parametrize("subsampling", E.SUBSAMPLINGS)
def test_encode_device_files_equal_the_definition(dev, subsampling):
    a, _ = E.overflow()
    batch = np.stack([E.named(90, subsampling, "64x48-smooth")[0], a[:, :48], np.zeros((64, 48, 3), np.uint8)])
    for quality in (90, 100):                                                # at 100 and 4:4:4 the noise image overflows its slot: encoded from the pixels
        files = J.encode_device(torch.from_numpy(batch).to(dev), quality, subsampling)
        assert files == [J.encode_np(x, quality, subsampling) for x in batch]
    assert J.encode_device(torch.zeros((0, 8, 8, 3), dtype=torch.uint8, device=dev)) == []
