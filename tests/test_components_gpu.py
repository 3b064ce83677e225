"""GPU: zh_second_largest_component (csrc/components.hip) against its NumPy definition (zutis_amd/components.py), exactly — mask, filled
foreground, labels and stats, through the u8 and the f64 input, alone and batched, inside guard bands and at the workspace's exact
size; then the keywords built on it (the drop-in's postprocess="device", the pseudo-label drivers' component="second_largest")."""
import os
import sys

import numpy as np
import pytest
import torch

from zutis_amd import _lib, components as K

from _components_case import CASES, same_shape_triples, working_size_case
from _guard import OUT_FILL, Arena, assert_equal, assert_untouched

pytestmark = pytest.mark.gpu

_REF = {}
_BY_NAME = dict(CASES)


def _ref(name, a):
    """(mask u8, filled u8, labels int32, stats int32 [4]) of the definition, computed once per case."""
    if name not in _REF:
        m, f, l, s = K.components_np(a)
        _REF[name] = (m.astype(np.uint8), f.astype(np.uint8), l.astype(np.int32), s.astype(np.int32))
    return _REF[name]


def _soft_of(a, rng):
    """A float64 image whose `> 0.5` is `a`: foreground in (0.5, 2], background in [-1, 0.5], 0.5 itself included."""
    lo, hi = rng.uniform(-1.0, 0.5, a.shape), rng.uniform(0.5, 2.0, a.shape)
    hi[hi == 0.5] = 1.0
    soft = np.where(a > 0, hi, lo)
    soft[(a == 0) & (rng.random(a.shape) < 0.2)] = 0.5
    return soft


def _run(dev, x, workspace_delta=0, with_optional=True):
    """The C entry on x (u8 or f64, [B,H,W]) with every output and the workspace in one guarded arena.
    -> (rc, mask, filled, labels, stats, arena)."""
    B, H, W = x.shape
    L = _lib.load()
    need = B * int(L.zh_components_workspace_size(H, W))
    ar = Arena(OUT_FILL, dev)
    mask = ar.add("mask", torch.uint8, B, H * W, tail_rows=1)
    filled = ar.add("filled", torch.uint8, B, H * W, tail_rows=1)
    labels = ar.add("labels", torch.int32, B, H * W, tail_rows=1)
    stats = ar.add("stats", torch.int32, B, 4, tail_rows=1)
    ws = ar.workspace("workspace", need + workspace_delta)
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    soft, binary = (xd.data_ptr(), None) if xd.dtype == torch.float64 else (None, xd.data_ptr())
    rc = L.zh_second_largest_component(soft, binary, 0.5, B, H, W, mask.m2.data_ptr(), filled.m2.data_ptr() if with_optional else None,
                                       labels.m2.data_ptr() if with_optional else None, stats.m2.data_ptr(), ws.m2.data_ptr(),
                                       need + workspace_delta, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, mask, filled, labels, stats, ar


def _check(names, x, got, what):
    rc, mask, filled, labels, stats, ar = got
    B, H, W = x.shape
    assert rc == 0, (what, _lib.load().zh_last_error())
    assert_untouched(ar)
    for b, name in enumerate(names):
        m, f, l, s = _ref(name, _BY_NAME[name])
        assert_equal(stats.get()[0, 0, b], s, f"{what} {name}: stats")
        assert_equal(labels.get()[0, 0, b].view(H, W), l, f"{what} {name}: labels")
        assert_equal(filled.get()[0, 0, b].view(H, W), f, f"{what} {name}: filled")
        assert_equal(mask.get()[0, 0, b].view(H, W), m, f"{what} {name}: mask")


@pytest.mark.parametrize("name,a", CASES, ids=[n for n, _ in CASES])
def test_entry_equals_the_definition(dev, name, a):
    """Every case, ties included (the definition IS the stable rule), through the u8 input and through a float64 image with the same
    `> 0.5`; outputs and workspace (exactly the queried size) inside guard bands."""
    _check([name], a[None], _run(dev, a[None]), "binary")
    soft = _soft_of(a, np.random.default_rng(5))
    assert np.array_equal(soft > 0.5, a > 0)
    _check([name], a[None], _run(dev, soft[None]), "soft")


_TRIPLES = same_shape_triples()


@pytest.mark.parametrize("names,x", _TRIPLES, ids=["+".join(n) for n, _ in _TRIPLES])
def test_batch_of_three_different_cases(dev, names, x):
    _check(names, x, _run(dev, x), "binary B=3")
    rng = np.random.default_rng(6)
    _check(names, x, _run(dev, np.stack([_soft_of(a, rng) for a in x])), "soft B=3")


def test_short_workspace_is_refused_and_nothing_is_written(dev):
    a = _BY_NAME["corner_blobs_65x65"]
    rc, *_, ar = _run(dev, a[None], workspace_delta=-1)
    assert rc == _lib.constants()["ZH_ERR_WORKSPACE"] and b"workspace" in _lib.load().zh_last_error()
    assert_untouched(ar, views=[])


def test_optional_outputs_may_be_null(dev):
    name = "noise_p0.45_65x130_seed0"
    a = _BY_NAME[name]
    rc, mask, filled, labels, stats, ar = _run(dev, a[None], with_optional=False)
    assert rc == 0
    assert_untouched(ar, views=[mask, stats, ar.views[-1]])
    m, _, _, s = _ref(name, a)
    assert_equal(mask.get()[0, 0, 0].view(a.shape), m, "mask")
    assert_equal(stats.get()[0, 0, 0], s, "stats")


def test_two_runs_are_bitwise_identical(dev):
    x = np.stack([a for n, a in CASES if a.shape == (65, 130)][:3])
    one, two = _run(dev, x), _run(dev, x)
    for v, w in zip(one[1:5], two[1:5]):
        assert torch.equal(v.get(), w.get())


def test_nan_is_background(dev):
    name = "ring_in_ring_island"
    a = _BY_NAME[name]
    soft = _soft_of(a, np.random.default_rng(8))
    soft[a == 0] = np.where(np.random.default_rng(9).random(int((a == 0).sum())) < 0.5, np.nan, soft[a == 0])
    assert np.isnan(soft).sum() > 10
    _check([name], a[None], _run(dev, soft[None]), "soft with NaN")


def test_goldens_of_the_real_reference(dev, golden_dir):
    from zutis_amd import ops
    g = np.load(os.path.join(golden_dir, "bilateral.npz"))
    for tag in sorted(k[:-5] for k in g.files if k.endswith("_soft")):
        soft = torch.from_numpy(np.ascontiguousarray(g[f"{tag}_soft"])).to(dev)
        mask, stats = ops.second_largest_component(soft, stats=True)
        assert np.array_equal(mask.cpu().numpy().astype(bool), g[f"{tag}_binary"]), tag
        assert int(stats[3]) == (1 if tag == "z" else 0)


def test_working_size(dev):
    """512 x 683: W is no multiple of the tile, 16 x 22 tiles, 342 scan blocks; a blob with 0.1 % of its pixels flipped."""
    from zutis_amd import ops
    a = working_size_case()
    m, f, l, s = _ref("working_size", a)
    mask, stats, filled, labels = ops.second_largest_component(torch.from_numpy(a).to(dev), stats=True, filled=True, labels=True)
    assert_equal(stats, s, "stats")
    assert_equal(labels, l, "labels")
    assert_equal(filled, f, "filled")
    assert_equal(mask, m, "mask")
    soft = torch.from_numpy(_soft_of(a, np.random.default_rng(3))).to(dev)
    ws = torch.empty(ops.components_workspace_size(512, 683), dtype=torch.uint8, device=dev)
    out = torch.empty(512 * 683, dtype=torch.uint8, device=dev)
    got = ops.second_largest_component(soft, workspace=ws, out=out)
    assert got.data_ptr() == out.data_ptr() and got.shape == (512, 683)
    assert_equal(got, m, "mask from soft, caller buffers")
    with pytest.raises(_lib.ZutisHipError, match="workspace"):
        ops.second_largest_component(soft, workspace=ws[:-1])


def _dropin():
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zutis_amd", "dropin")
    if d not in sys.path:
        sys.path.insert(0, d)
    from utils import bilateral_solver
    return bilateral_solver


def test_dropin_postprocess_device_equals_host(dev, golden_dir):
    from PIL import Image
    from zutis_amd import detgen
    B = _dropin()
    g = np.load(os.path.join(golden_dir, "bilateral.npz"))
    h, w, seed = (int(v) for v in g["c_hw"])
    img = Image.fromarray(detgen.selfmask_like_rgb(h, w, seed=seed))
    soft_h, mask_h = B.bilateral_solver_output(img, g["c_target"])
    soft_d, mask_d = B.bilateral_solver_output(img, g["c_target"], postprocess="device")
    assert soft_d.dtype == np.float64 and mask_d.dtype == np.bool_ and mask_d.shape == soft_d.shape == (h, w)
    assert not K.has_tie(soft_h)
    assert np.array_equal(soft_h, soft_d) and np.array_equal(mask_h, mask_d) and np.array_equal(mask_d, g["c_binary"])
    x = torch.from_numpy(detgen.images(1, h, w, seed=2))[0].to(dev)
    t = torch.from_numpy(np.ascontiguousarray(g["c_target"])).to(dev)
    s1, m1 = B.bilateral_solver_output_from_tensor(x, t)
    s2, m2 = B.bilateral_solver_output_from_tensor(x, t, postprocess="device")
    assert np.array_equal(s1, s2) and m2.dtype == np.bool_ and np.array_equal(m2, K.postprocess_np(s1))
    assert not K.has_tie(s1) and np.array_equal(m1, m2)           # seed 2: counts 2869 / 1101 / 47 ..., far from a tie


def test_pseudo_masks_batch_component(dev):
    """component="second_largest" = the definition applied to the solver's soft output at solver resolution, then the nearest resize;
    component=None = what the driver returned before the keyword existed (`> 0.5`, resized)."""
    from zutis_amd import detgen, ops, pseudo_masks
    from zutis_amd.engine import SelfMaskEngine
    eng = SelfMaskEngine({k: torch.from_numpy(v).to(dev) for k, v in detgen.selfmask_state_dict().items()})
    x = torch.from_numpy(detgen.images(2, 72, 100, seed=40)).to(dev)
    sizes = [(145, 200), (72, 100)]
    dts = eng.forward(x.contiguous(), inference=True)["dts"]
    rgb = torch.stack([ops.denormalize_u8(x[b].contiguous()) for b in range(2)])
    soft, _ = ops.bilateral_solve(rgb, dts.contiguous())
    soft = soft.cpu().numpy()
    got = pseudo_masks.pseudo_masks_batch(eng, x, sizes, component="second_largest")
    plain = pseudo_masks.pseudo_masks_batch(eng, x, sizes, component=None)
    default = pseudo_masks.pseudo_masks_batch(eng, x, sizes)
    for b, (h, w) in enumerate(sizes):
        want = torch.from_numpy(K.postprocess_np(soft[b]).astype(np.uint8)).to(dev)
        thr = torch.from_numpy((soft[b] > 0.5).astype(np.uint8)).to(dev)
        if (h, w) != (72, 100):
            want, thr = ops.resize_nearest_u8(want, h, w), ops.resize_nearest_u8(thr, h, w)
        assert got[b].dtype == torch.uint8 and got[b].shape == (h, w)
        assert_equal(got[b], want, f"component image {b}")
        assert_equal(plain[b], thr, f"plain image {b}")
        assert torch.equal(plain[b], default[b])
    with pytest.raises(ValueError):
        pseudo_masks.pseudo_masks_batch(eng, x, sizes, bilateral_solver=False, component="second_largest")
