"""CPU: the public surface of the device assignment mode (no kernel runs)."""
import ctypes

import pytest
import torch

from zutis_amd import _lib, build, ops


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


def test_bad_assignment_value_raises():
    from zutis_amd.criterion import HipCriterion
    te = torch.zeros(3, 8)
    assert HipCriterion(te).assignment == "host"                            # the default stays the host solve
    crit = HipCriterion(te, assignment="device")
    assert crit.assignment == "device"
    with pytest.raises(ValueError, match="assignment"):
        HipCriterion(te, assignment="gpu")
    with pytest.raises(ValueError, match="assignment"):
        crit.assignment = "scipy"
    assert crit.assignment == "device"
    with pytest.raises(TypeError):                                          # keyword-only: the reference's positional call is unaffected
        HipCriterion(te, 1.0, 1.0, 1.0, 1.0, 255, "device")


def test_dropin_keeps_the_reference_constructor_and_takes_the_mode_as_an_attribute(monkeypatch):
    from zutis_amd.dropin.criterion import Criterion
    te = torch.zeros(3, 8)
    crit = Criterion(te, 1.0, 2.0, 1.0, 1.0, 7)
    assert crit.assignment == "host" and crit.weight_mask_loss == 2.0 and crit.ignore_index == 7
    with pytest.raises(TypeError):                                          # the reference's constructor, argument for argument
        Criterion(te, assignment="device")
    crit.assignment = "device"
    assert crit.assignment == "device"
    with pytest.raises(ValueError, match="assignment"):
        crit.assignment = "gpu"
    monkeypatch.setattr(Criterion, "default_assignment", "device")
    assert Criterion(te).assignment == "device"


def test_device_mode_refuses_cpu_proposals():
    from zutis_amd.criterion import HipCriterion
    crit = HipCriterion(torch.zeros(3, 8), assignment="device")
    with pytest.raises(_lib.ZutisHipError, match="no CPU fallback"):
        crit(torch.zeros(1, 2, 4, 4), [torch.zeros(1, 8, 8, dtype=torch.uint8)], None, torch.zeros(1, 4, 4, 8),
             torch.zeros(1, 8, 8, dtype=torch.int64))


def test_header_declares_both_entries_and_their_argument_types(lib):
    vp, i, l, f, z = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_size_t
    e = _lib.entries()
    assert (e["zh_linear_assignment"].restype, e["zh_linear_assignment"].argtypes) == (i, [vp, vp, vp, i, i, i, i, i, vp, vp, vp, vp, vp, z, vp])
    assert (e["zh_linear_assignment_workspace_size"].restype, e["zh_linear_assignment_workspace_size"].argtypes) == (z, [i, i, i])
    assert (e["zh_pack_masks_u8"].restype, e["zh_pack_masks_u8"].argtypes) == (i, [vp, vp, i, i, l, vp, vp, vp])
    assert e["zh_linear_assignment"].plannable
    assert not e["zh_pack_masks_u8"].plannable          # host pointer / count tables: not replayable from a launch plan
    for name in ("zh_linear_assignment", "zh_linear_assignment_workspace_size", "zh_linear_assignment_max_dim", "zh_pack_masks_u8"):
        assert hasattr(lib, name) and list(getattr(lib, name).argtypes) == e[name].argtypes
    assert _lib.header_abi_version() >= 232


def test_cap_and_argument_checks_without_gpu(lib):
    assert lib.zh_linear_assignment_max_dim() == _lib.constants()["ZH_ASSIGN_MAX_DIM"] == ops.ASSIGN_MAX_DIM == 1024
    assert lib.zh_linear_assignment_workspace_size(8, 6, 80) == 8 * 6 * 8 + 6 * 80 * 4
    ok = (16, 16, 16, 1, 1)                                 # non-null dummies: the checks come before any launch
    rc = lib.zh_linear_assignment(*ok, ops.ASSIGN_MAX_DIM + 1, 2, 2, 16, 16, 16, 16, 16, 1 << 20, None)
    assert rc == -1 and b"exceeds the cap" in lib.zh_last_error()
    rc = lib.zh_linear_assignment(*ok, 7, ops.ASSIGN_MAX_DIM + 1, ops.ASSIGN_MAX_DIM + 1, 16, 16, 16, 16, 16, 1 << 30, None)
    assert rc == -1 and b"exceeds the cap" in lib.zh_last_error()
    rc = lib.zh_linear_assignment(*ok, 7, 2, 2, 16, 16, 16, 16, 16, 8, None)
    assert rc == -1 and b"workspace" in lib.zh_last_error()
    src, cnt = (ctypes.c_void_p * 1)(16), (ctypes.c_int * 1)(1)
    rc = lib.zh_pack_masks_u8(src, cnt, 1, 4, 576, 16, 16, None)
    assert rc == -1 and b"element size" in lib.zh_last_error()
    assert ops.assignment_pairs_capacity(3, 2, 7, 5, 7) == 2 * 7 and ops.assignment_pairs_capacity(3, 2, 3, 5, 12) == 2 * 9
