"""CPU: zutis_amd/components.py (the NumPy definition of the device mask post-processing) against scipy.ndimage and the reference's
restatement (oracle.bilateral_ref.postprocess, utils/bilateral_solver.py:185-193), exactly, on the shared case list; the stable tie rule;
the reference's own goldens; the keywords of the drivers and the drop-in; the header."""
import os
import sys

import numpy as np
import pytest
from scipy import ndimage

from zutis_amd import _lib, components as K
from oracle import bilateral_ref as R

from _components_case import CASES, TIE_FREE, TIES, working_size_case


def test_case_list_is_what_the_suites_rely_on():
    names = [n for n, _ in CASES]
    assert len(set(names)) == len(names) and len(TIES) == 2 and len(TIE_FREE) == len(CASES) - 2
    assert all(a.dtype == np.uint8 and a.ndim == 2 and a.max(initial=0) <= 1 for _, a in CASES)
    shapes = {a.shape for _, a in CASES}
    assert {(1, 1), (1, 7), (7, 1), (37, 53), (65, 130)} <= shapes
    # ZERO tie-free cases are skipped below: each of them really is tie-free, and the two tie cases really are ties
    assert [n for n, a in TIE_FREE if K.has_tie(a)] == []
    assert [n for n, a in TIES if not K.has_tie(a)] == []


@pytest.mark.parametrize("name,a", TIE_FREE, ids=[n for n, _ in TIE_FREE])
def test_definition_equals_scipy_and_the_reference(name, a):
    mask, filled, labels, stats = K.components_np(a)
    want_filled = ndimage.binary_fill_holes(a > 0)
    want_labels, want_nr = ndimage.label(want_filled)
    assert filled.dtype == np.bool_ and np.array_equal(filled, want_filled)
    assert np.array_equal(K.fill_holes_np(a), want_filled)
    got_labels, got_nr = K.label_np(want_filled)
    assert got_nr == want_nr == int(stats[0]) and labels.dtype == np.int32
    assert np.array_equal(labels, want_labels) and np.array_equal(got_labels, want_labels)
    raw_labels, raw_nr = ndimage.label(a)                                           # labelling alone, on the unfilled image too
    assert K.label_np(a)[1] == raw_nr and np.array_equal(K.label_np(a)[0], raw_labels)
    want = R.postprocess(a.astype(np.float64))                                      # soft = the mask itself: soft > 0.5 == a
    assert mask.dtype == np.bool_ and np.array_equal(mask, want)
    assert np.array_equal(K.postprocess_np(a.astype(np.float64)), want) and np.array_equal(K.postprocess_np(a), want)
    if stats[3]:
        assert want.all() and list(stats) == [0, -1, a.size, 1]
    else:
        assert int(stats[2]) == int((labels == stats[1]).sum()) == int(mask.sum())


def test_named_properties_of_the_cases():
    by = dict(CASES)
    assert K.postprocess_np(by["all_zeros"]).all() and K.postprocess_np(by["1x1_zero"]).all()            # the fallback
    m, _, _, st = K.components_np(by["all_ones"])
    assert not m.any() and list(st) == [1, 0, 0, 0]                                                    # counts [0, HW]: label 0, nothing
    m, f, _, st = K.components_np(by["blob_over_half"])
    assert st[1] == 0 and np.array_equal(m, ~f)                                                        # the background is selected
    _, f, l, st = K.components_np(by["plus"])
    assert st[0] == 1 and f.sum() == 5 and ndimage.label(by["plus"])[1] == 4                            # four components fused by the filling
    _, f, _, _ = K.components_np(by["diagonal_pocket"])
    assert f[1, 1] and not f[0, 0]
    _, f, _, _ = K.components_np(by["hole_open_to_border"])
    assert np.array_equal(f, by["hole_open_to_border"] > 0)
    _, _, l, _ = K.components_np(by["comb_late_merge"])
    assert l[0, 0] == 1 and l[0, 2] == 1 and l[0, -2] == 2                                             # late merges keep the first pixel's number
    assert K.components_np(by["tie_second_capacity"])[3][0] == (by["tie_second_capacity"].size + 1) // 2


@pytest.mark.parametrize("name,a", TIES, ids=[n for n, _ in TIES])
def test_ties_follow_the_stable_rule(name, a):
    filled = ndimage.binary_fill_holes(a > 0)
    labels, nr = ndimage.label(filled)
    counts = np.bincount(labels.reshape(-1), minlength=nr + 1)
    chosen = sorted(range(nr + 1), key=lambda i: (counts[i], i))[-2]                 # second largest under the key (count, label)
    assert chosen == int(np.argsort(counts, kind="stable")[-2])
    mask, _, got_labels, stats = K.components_np(a)
    assert np.array_equal(got_labels, labels) and list(stats) == [nr, chosen, counts[chosen], 0]
    assert np.array_equal(mask, labels == chosen)


def test_float_input_threshold_and_nan():
    soft = np.array([[0.5, 0.500001, np.nan, 0.9], [0.2, 0.7, 0.7, -1.0]])
    with np.errstate(invalid="ignore"):
        assert np.array_equal(K._foreground(soft), np.array([[0, 1, 0, 1], [0, 1, 1, 0]], bool))
    assert np.array_equal(K.postprocess_np(soft), R.postprocess(np.nan_to_num(soft, nan=0.0)))
    with pytest.raises(ValueError):
        K.postprocess_np(np.zeros((2, 3, 4)))


def test_goldens_of_the_real_reference(golden_dir):
    """tests/golden/bilateral.npz was written by the reference itself: *_soft -> *_binary (z_ = the empty target: all True)."""
    g = np.load(os.path.join(golden_dir, "bilateral.npz"))
    tags = sorted(k[:-5] for k in g.files if k.endswith("_soft"))
    assert len(tags) == 4 and "z" in tags
    for tag in tags:
        assert not K.has_tie(g[f"{tag}_soft"]), tag
        assert np.array_equal(K.postprocess_np(g[f"{tag}_soft"]), g[f"{tag}_binary"]), tag
    assert g["z_binary"].all()


def test_working_size_case_is_tie_free_and_matches_the_reference():
    a = working_size_case()
    assert a.shape == (512, 683) and not K.has_tie(a)
    assert np.array_equal(K.postprocess_np(a), R.postprocess(a.astype(np.float64)))


def test_keywords_are_validated_without_a_gpu():
    from zutis_amd import pseudo_masks as P
    calls = [lambda **kw: P.pseudo_mask(None, None, **kw), lambda **kw: P.pseudo_masks_batch(None, None, **kw),
             lambda **kw: P.generate_pseudo_masks(None, [], [], [], **kw), lambda **kw: P.generate_pseudo_masks_batched(None, [], [], [], **kw),
             lambda **kw: P.generate_pseudo_masks_from_files(None, [], [], **kw), lambda **kw: P.dataset_generate_pseudo_masks(None, [], "", **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="neither None nor 'second_largest'"):
            call(component="largest")
        with pytest.raises(ValueError, match="bilateral_solver=True"):
            call(component="second_largest", bilateral_solver=False)
    assert P.generate_pseudo_masks_from_files(None, [], [], component="second_largest") == []
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zutis_amd", "dropin")
    if d not in sys.path:
        sys.path.insert(0, d)
    from utils.bilateral_solver import bilateral_solver_output, bilateral_solver_output_from_tensor
    with pytest.raises(ValueError, match="neither 'host' nor 'device'"):
        bilateral_solver_output(None, np.zeros((2, 2)), postprocess="gpu")
    with pytest.raises(ValueError, match="neither 'host' nor 'device'"):
        bilateral_solver_output_from_tensor(None, None, postprocess="gpu")


def test_header_declares_the_entry_and_the_tile_constants():
    e, c = _lib.entries(), _lib.constants()
    assert [t for t, _ in e["zh_components_workspace_size"].params] == ["int", "int"] and e["zh_components_workspace_size"].ret == "size_t"
    assert [n for _, n in e["zh_second_largest_component"].params] == ["soft", "binary", "threshold", "B", "H", "W", "mask_out", "filled_out",
                                                                      "labels_out", "stats", "workspace", "workspace_bytes", "stream"]
    assert e["zh_second_largest_component"].plannable
    assert c["ZH_CCL_TILE_H"] >= 8 and c["ZH_CCL_TILE_W"] >= 8 and c["ZH_ABI_VERSION"] >= 247


def test_entry_validates_its_arguments_without_a_gpu():
    from zutis_amd import build
    build.build(verbose=False)
    L = _lib.load(raw=True)
    assert L.zh_components_workspace_size(0, 5) == 0 and L.zh_components_workspace_size(1, 1) > 0
    need = L.zh_components_workspace_size(512, 683)
    assert need >= 512 * 683 * 9 + ((512 * 683 + 1) // 2 + 1) * 4
    err = _lib.constants()["ZH_ERR_ARG"]
    assert L.zh_second_largest_component(None, None, 0.5, 1, 4, 4, 256, None, None, 256, 256, 1 << 20, None) == err
    assert b"exactly one" in L.zh_last_error()
    assert L.zh_second_largest_component(256, 256, 0.5, 1, 4, 4, 256, None, None, 256, 256, 1 << 20, None) == err
    assert L.zh_second_largest_component(256, None, 0.5, 1, 0, 4, 256, None, None, 256, 256, 1 << 20, None) == err
    assert L.zh_second_largest_component(256, None, 0.5, 1, 4, 4, None, None, None, 256, 256, 1 << 20, None) == err
    assert L.zh_second_largest_component(256, None, 0.5, 1, 4, 4, 256, None, None, 256, 256, L.zh_components_workspace_size(4, 4) - 1,
                                         None) == _lib.constants()["ZH_ERR_WORKSPACE"]
    assert L.zh_second_largest_component(256, None, 0.5, 0, 4, 4, None, None, None, None, None, 0, None) == 0      # B = 0: nothing to do
