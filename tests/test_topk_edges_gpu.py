"""zh_topk_rows (ops.topk_rows, retrieval.merge_topk) on the cases of tests/_topk_case.py: indices equal to the contract's — every NaN
first, value descending with -0.0 == +0.0, column ascending — and values returned as the stored bits (signed zeros, NaN payloads).

Radix passes and the bucket their histogram walk stops in (pivot_buckets; 255 = at the first step, 0 = after all 256 buckets):

    pass  key byte            bucket 255                               bucket 0
    0     value byte 3        finite >= 2^127 and +inf                 < -2^127 and -inf
    1..3  value byte 2..0     rows sharing their top 1, 2, 3 bytes     the same rows, the k-th value's byte 0x00
    4     column byte 3       any row below 2^24 columns               (column >= 0xFF000000: out of reach)
    5     column byte 2       any row whose k-th column is < 65536     index_byte2_low: column >= 0xFF0000 (67 MB row)
    6     column byte 1       k-th column < 256                        k-th column 0xFF13 (ties in a window)
    7     column byte 0       k-th column 512                          k-th column 0x2FF

index_byte2 / index_byte3: the selected set crosses column 65536 / 2^24, so the selection is decided by that column byte.
"""
import time

import numpy as np
import pytest
import torch

from tests import _topk_case as K
from zutis_amd import ops, retrieval

pytestmark = pytest.mark.gpu

IDX_FILL = -7
VAL_FILL_BITS = 0xDEADBEEF


def _check(case, got_idx, got_val, idx_of=None):
    x, N, k, exp = case
    got_idx, got_val = got_idx.cpu().numpy(), got_val.cpu().numpy()
    want_idx = exp if idx_of is None else idx_of(exp)
    assert got_idx.dtype == np.int64 and got_idx.shape == exp.shape
    bad = np.flatnonzero((got_idx != want_idx).any(1))
    assert bad.size == 0, f"rows {bad[:5].tolist()}: got {got_idx[bad[0]][:12].tolist()} want {want_idx[bad[0]][:12].tolist()}"
    assert np.array_equal(K.bits_of(got_val), K.bits_of(np.take_along_axis(x, exp, 1)))        # the stored bits, not just equal values


def _run(dev, case):
    x, N, k, exp = case
    idx, val = ops.topk_rows(torch.from_numpy(x).to(dev), k, N=N, with_values=True)
    _check(case, idx, val)


def _cases():
    out = [("signed_zero", K.signed_zero, ())]
    out += [(f"random_bits-{k}", K.random_bits, (k,)) for k in K.RANDOM_BITS_K]
    out += [(f"nan_signs-{k}", K.nan_signs, (k,)) for k in K.NAN_SIGNS_K]
    out += [(f"pivot-pass{p}-{'low' if low else 'high'}", K.pivot_buckets, (p, low)) for p, low in K.PIVOT_CASES]
    out += [("index_byte2", K.index_byte2, ())]
    out += [(f"small_n-{N}-{k}", K.small_n, (N, k)) for N, k in K.SMALL_N]
    out += [("many_rows", K.many_rows, ())]
    return out


CASES = _cases()
ADDRESSED = [c for c in CASES if c[0].split("-")[0] in ("random_bits", "signed_zero", "nan_signs")]


@pytest.mark.parametrize("build,args", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_topk_case(dev, build, args):
    _run(dev, build(*args))


@pytest.mark.parametrize("build", [K.index_byte3, K.index_byte2_low], ids=["index_byte3", "index_byte2_low"])
def test_topk_large_row(dev, build):
    """One 67 MB row, read nine times by one workgroup: 0.19 s per launch on the MI355X (printed with -s)."""
    case = build()
    xd = torch.from_numpy(case[0]).to(dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    idx, val = ops.topk_rows(xd, case[2], N=case[1], with_values=True)
    torch.cuda.synchronize()
    print(f"\n{build.__name__}: N = {case[1]}, k = {case[2]}: {1e3 * (time.perf_counter() - t0):.1f} ms")
    _check(case, idx, val)


def _padded(case, pad=9):
    """ld = N + pad; the pad columns hold +inf and NaNs of both signs, which must never be selected."""
    x, N, k, exp = case
    fill = K.f32_of(np.array([0x7F800000, K.NAN_POS, K.NAN_NEG], dtype=np.uint32))
    wide = np.empty((x.shape[0], N + pad), np.float32)
    wide[:, :N] = x[:, :N]
    wide[:, N:] = fill[np.arange(pad) % 3]
    return wide, N, k, exp


@pytest.mark.parametrize("form", ["padded", "idx_map", "strided", "all"])
@pytest.mark.parametrize("build,args", [c[1:] for c in ADDRESSED], ids=[c[0] for c in ADDRESSED])
def test_topk_addressing_forms(dev, build, args, form):
    """The three forms the retrieval uses: a padded leading dimension, an index map, and outputs that are a column block of a wider
    candidate table whose other columns must keep their sentinel."""
    case = build(*args)
    if form in ("padded", "all"):
        case = _padded(case)
    x, N, k, exp = case
    R, ld = x.shape
    kw, idx_of = {}, None
    if form in ("idx_map", "all"):
        imap = (np.arange(R * ld, dtype=np.int64).reshape(R, ld) * 7 + 3) % 100003 + (np.int64(1) << 33)    # not monotone, past 32 bits
        kw["idx_map"] = torch.from_numpy(imap).to(dev)
        idx_of = lambda e: np.take_along_axis(imap, e, 1)                 # noqa: E731
    if form in ("strided", "all"):
        lead, trail = 5, 6
        wide_i = torch.full((R, lead + k + trail), IDX_FILL, dtype=torch.int64, device=dev)
        wide_v = torch.from_numpy(np.full((R, lead + k + trail), VAL_FILL_BITS, np.uint32).view(np.float32)).to(dev)
        kw["out_idx"], kw["out_val"] = wide_i[:, lead:lead + k], wide_v[:, lead:lead + k]
    idx, val = ops.topk_rows(torch.from_numpy(x).to(dev), k, N=N, with_values=True, **kw)
    _check(case, idx, val, idx_of)
    if form in ("strided", "all"):
        wi, wv = wide_i.cpu().numpy(), K.bits_of(wide_v.cpu().numpy())
        assert (wi[:, :lead] == IDX_FILL).all() and (wi[:, lead + k:] == IDX_FILL).all()
        assert (wv[:, :lead] == VAL_FILL_BITS).all() and (wv[:, lead + k:] == VAL_FILL_BITS).all()
        assert np.array_equal(wi[:, lead:lead + k], idx.cpu().numpy())


def test_topk_idx_add(dev):
    x, N, k, exp = K.nan_signs(K.NAN_SIGNS_K[-1])
    idx = ops.topk_rows(torch.from_numpy(x).to(dev), k, idx_add=(1 << 40) + 5)
    assert np.array_equal(idx.cpu().numpy(), exp + (1 << 40) + 5)


def test_merge_topk_equals_reference_over_the_union(dev):
    """Two chunk lists, each sorted by the contract: -0.0 in one where the other holds +0.0 at the k-th place, and a sign-bit NaN."""
    cand_idx, cand_val, k, exp = K.merge_case()
    idx, val = retrieval.merge_topk(torch.from_numpy(cand_idx).to(dev), torch.from_numpy(cand_val).to(dev), k)
    want = np.stack([K.reference(r, k) for r in cand_val])
    assert np.array_equal(want, exp)
    assert np.array_equal(idx.cpu().numpy(), np.take_along_axis(cand_idx, want, 1))
    assert np.array_equal(K.bits_of(val.cpu().numpy()), K.bits_of(np.take_along_axis(cand_val, want, 1)))
