"""The host decode of the instance predict's one result buffer (zutis_amd/instances.py: carve, read_fused, read_chain, assemble) on
buffers built with numpy the way the kernels fill them: no GPU."""
import numpy as np
import pytest

from zutis_amd import instances, rle

B, Q, H, W = 2, 6, 9, 7
IDS = np.array([33, 2, 40, 3], np.int64)      # wraps in CPython's set table: iteration order [40, 33, 2, 3], not ascending


def _content(counts, seed=0):
    """Random 9x7 masks, categories and scores, and per image the kernel's kept list: `counts[b]` queries, categories ascending."""
    rng = np.random.default_rng(seed)
    masks = (rng.random((B, Q, H, W)) > 0.5).astype(np.uint8)
    masks[0, 1] = 0                                                   # an empty mask: the one-run string
    masks[1, 2, 0, 0] = 1                                             # pixel 0 set: the leading empty run
    cats = IDS[rng.integers(0, 4, (B, Q))]
    cats[:, :4] = IDS                                                 # every id in every image
    scores = rng.random((B, Q))
    kept = []
    for b in range(B):
        qs = rng.permutation(Q)[:counts[b]]
        kept.append([int(q) for q in qs[np.argsort(cats[b, qs], kind="stable")]])
    return masks, cats, scores, kept


def _pk(cats, scores, kept):
    pk = np.full((B, 4 * Q + 2), np.nan)                              # entries past the count are never written by the kernel
    for b in range(B):
        n = len(kept[b])
        pk[b, :n], pk[b, Q:Q + n], pk[b, 2 * Q:2 * Q + n] = kept[b], scores[b, kept[b]], cats[b, kept[b]]
        pk[b, 3 * Q:4 * Q], pk[b, 4 * Q], pk[b, 4 * Q + 1] = cats[b], n, 0
    return pk


def _box_area(m):
    ys, xs = np.nonzero(m)
    return ([float(xs.min()), float(ys.min()), float(xs.max()), float(ys.max())] if len(ys) else [0.0] * 4), int(m.sum())


def _transitions(m):
    flat = m.reshape(-1, order="F")
    return (np.flatnonzero(flat[1:] != flat[:-1]) + 1).astype(np.int32), int(flat[0])


def _fused_buffer(masks, cats, scores, kept, unwritten=()):
    sections = instances.fused_layout(B, Q, 600)
    buf = np.full((instances.layout_bytes(sections),), 0xEE, np.uint8)
    v = instances.carve(buf, sections)
    v["pk"][:] = _pk(cats, scores, kept)
    slots = [(b, j, q) for b in range(B) for j, q in enumerate(kept[b])]
    at = 0
    for b, j, q in slots[::-1]:                                       # the cursor hands out offsets in the order workgroups arrive
        s = rle.encode(masks[b, q])["counts"]
        box, area = _box_area(masks[b, q])
        ln = -1 if (b, j) in unwritten else len(s)
        v["info"][b * Q + j] = [at, ln, *map(int, box), area, len(_transitions(masks[b, q])[0])]
        if ln >= 0:
            v["chars"][at:at + ln] = np.frombuffer(s, np.uint8)
            at += ln
    return buf, sections


def _chain_buffer(masks, cats, scores, kept, max_runs=8192, unwritten=()):
    """-> buffer, sections, lens, the whole packed list.  The head is too short for a real string kernel to matter: strings are placed
    by the documented rule, 5 * (start of the mask's list) + 16 * (kept masks before it), across the batch."""
    slots = [(b, j, q) for b in range(B) for j, q in enumerate(kept[b])]
    trans = {(b, j): _transitions(masks[b, q]) for b, j, q in slots}
    lens = [[min(len(trans[b, j][0]), max_runs) for j in range(len(kept[b]))] for b in range(B)]
    sections = instances.chain_layout(B, Q, sum(map(sum, lens)))
    buf = np.full((instances.layout_bytes(sections),), 0xEE, np.uint8)
    v = instances.carve(buf, sections)
    v["pk"][:] = _pk(cats, scores, kept)
    at, packed = 0, []
    for rank, (b, j, q) in enumerate(slots):
        pos, first = trans[b, j]
        s = rle.encode(masks[b, q])["counts"]
        box, area = _box_area(masks[b, q])
        v["nr"][b * Q + j] = [len(pos), first]
        v["ba"][b * Q + j] = [*map(int, box), area]
        over = len(pos) > max_runs or (b, j) in unwritten
        v["slen"][b * Q + j] = -1 if over else len(s)
        if not over:
            assert len(s) <= 5 * lens[b][j] + 16
            c0 = 5 * at + 16 * rank
            v["chars"][c0:c0 + len(s)] = np.frombuffer(s, np.uint8)
        packed.append(pos[:max_runs])
        at += lens[b][j]
    return buf, sections, lens, np.concatenate(packed) if packed else np.zeros((0,), np.int32)


def _expected(masks, cats, scores, kept, none=()):
    """The reference's emission order, restated: categories in the iteration order of set(category ids of the image)."""
    out = [], [], [], [], [], []
    for b in range(B):
        for c in set(cats[b]):
            for j, q in enumerate(kept[b]):
                if cats[b, q] != c:
                    continue
                box, area = _box_area(masks[b, q])
                if (b, j) in none:
                    out[5].append((len(out[0]), b * Q + q))
                out[0].append((b, int(c), q, float(scores[b, q])))
                out[1].append(None if (b, j) in none else rle.encode(masks[b, q]))
                out[2].append(box); out[3].append(area); out[4].append(j)
    return out


def _decode(buf, sections, reader, *args):
    v = instances.carve(buf, sections)
    counts = v["pk"][:, 4 * Q].astype(np.int64).tolist()
    return instances.assemble(v["pk"], reader(v, counts, *args), Q)


def test_set_order_of_the_category_ids_is_not_ascending():
    order = [int(c) for c in set(IDS)]
    assert order != sorted(order)
    rank = instances.reference_category_rank(IDS)
    assert sorted(rank, key=rank.get) == order


def test_carve_places_the_views_at_the_hand_computed_offsets():
    """B = 2, Q = 6: pk is 2 * 26 doubles = 416 bytes; fused: info 12 * 8 ints = 384 -> cursor at 800, strings at 808; chain: nr 96 ->
    ba at 512, 240 -> slen at 752, 48 -> strings at 800, 5 * head + 16 * 12 of them."""
    for sections, want, total in ((instances.fused_layout(B, Q, 64), {"pk": 0, "info": 416, "cursor": 800, "chars": 808}, 872),
                                  (instances.chain_layout(B, Q, 10), {"pk": 0, "nr": 416, "ba": 512, "slen": 752, "chars": 800}, 1042)):
        assert instances.layout_bytes(sections) == total
        buf = np.zeros((total,), np.uint8)
        v = instances.carve(buf, sections)
        base = buf.__array_interface__["data"][0]
        assert {k: a.__array_interface__["data"][0] - base for k, a in v.items()} == want
        assert all(np.shares_memory(a, buf) for a in v.values())
        assert {k: (a.dtype, a.shape) for k, a in v.items()} == {name: (np.dtype(dt), shape) for name, dt, shape in sections}
    assert v["chars"].shape == (5 * 10 + 16 * B * Q,) and v["pk"].shape == (B, 4 * Q + 2)


@pytest.mark.parametrize("counts", [(4, 5), (0, 4), (6, 0), (0, 0)])
def test_both_layouts_decode_to_the_reference_order(counts):
    """The same logical content through the fused layout, the chain layout (the string walk crosses the image boundary) and the
    chain's second-list form: identical kept / rles / boxes / areas / slots, equal to the reference's order restated; no redo."""
    content = _content(counts, seed=sum(counts))
    size = [H, W]
    want = _expected(*content)
    fb, fs = _fused_buffer(*content)
    cb, cs, lens, packed = _chain_buffer(*content)
    got_f = _decode(fb, fs, instances.read_fused, size)
    got_c = _decode(cb, cs, instances.read_chain, lens, size, 8192)
    got_2 = _decode(cb, cs, instances.read_chain, lens, size, 8192, packed)
    assert got_f == want and got_c == want and got_2 == want
    assert len(got_f[0]) == sum(counts) and got_f[5] == []
    assert all(type(a) is int for a in got_f[3] + got_c[3]) and all(type(x) is float for bx in got_f[2] + got_c[2] for x in bx)


def test_unwritten_strings_come_back_as_redo_entries_at_their_output_position():
    """Length -1 (fused info / chain slen): the string is None and (position in the output lists, flat mask index) is in redo —
    here the first slot of image 0 (not first in the output: the set order moves it) and the last of image 1."""
    content = _content((4, 5), seed=3)
    none = {(0, 0), (1, 4)}
    want = _expected(*content, none=none)
    assert len(want[5]) == 2 and want[5][0][0] != 0
    fb, fs = _fused_buffer(*content, unwritten=none)
    cb, cs, lens, _ = _chain_buffer(*content, unwritten=none)
    assert _decode(fb, fs, instances.read_fused, [H, W]) == want
    assert _decode(cb, cs, instances.read_chain, lens, [H, W], 8192) == want


def test_second_list_with_masks_over_max_runs():
    """rles_from_transitions(packed_max_runs=): every mask's list is cut at max_runs, the masks over it come back None -> redo; the
    device-written strings of the same buffer (slen -1 for those masks) decode to the same."""
    content = _content((4, 5), seed=5)
    masks, _, _, kept = content
    nt = {(b, j): len(_transitions(masks[b, q])[0]) for b in range(B) for j, q in enumerate(kept[b])}
    max_runs = sorted(nt.values())[len(nt) // 2]
    none = {k for k, t in nt.items() if t > max_runs}
    assert 0 < len(none) < len(nt)
    want = _expected(*content, none=none)
    cb, cs, lens, packed = _chain_buffer(*content, max_runs=max_runs)
    assert max(map(max, lens)) == max_runs and packed.size == sum(map(sum, lens))
    assert _decode(cb, cs, instances.read_chain, lens, [H, W], max_runs, packed) == want
    assert _decode(cb, cs, instances.read_chain, lens, [H, W], max_runs) == want
