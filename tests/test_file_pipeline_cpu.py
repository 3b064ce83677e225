"""CPU: the two shared pieces of the file pipeline (zutis_amd/preprocess.py) on their own — the prefetching generator every loader
iterates through and the writer ring of the drivers that write files.  Unpinned host tensors, no device; nothing here sleeps: the
threads are ordered with events (whose time limits only run out when the code under test is wrong)."""
import threading

import pytest

from zutis_amd import preprocess as P

LIMIT = 10.0        # seconds an event is waited for before a test gives up


def _decode_threads():
    return [t for t in threading.enumerate() if t.name.startswith("zutis-decode")]


# ------------------------------------------------------------------------------------------------------------------ prefetch
def test_prefetch_starts_one_item_ahead_and_never_two():
    log = []

    def start(pool, slot, item):
        log.append(("start", item, slot))
        return item, [pool.submit(lambda: None)]

    for batch in P.prefetch(iter(range(4)), start, 2):
        log.append(("yield", batch))
    assert log == [("start", 0, 0), ("start", 1, 1), ("yield", 0), ("start", 2, 0), ("yield", 1), ("start", 3, 1), ("yield", 2), ("yield", 3)]
    assert not _decode_threads()


def test_prefetch_raises_a_workers_exception_at_the_step_that_needs_its_batch():
    def boom():
        raise ValueError("item 1 does not decode")

    def start(pool, slot, item):
        return item, [pool.submit(boom if item == 1 else (lambda: None))]

    batches = P.prefetch(range(3), start, 2)
    assert next(batches) == 0                   # item 1 is already started (and has failed): batch 0 does not need it
    with pytest.raises(ValueError, match="item 1 does not decode"):
        next(batches)
    assert not _decode_threads()


def test_closing_prefetch_early_cancels_what_is_pending_and_joins_its_threads():
    release, made = threading.Event(), {}

    def start(pool, slot, item):
        if item == 0:
            return item, [pool.submit(lambda: None)]
        futures = [pool.submit(release.wait, LIMIT)] + [pool.submit(lambda: None) for _ in range(2)]      # one thread: the last two queue up
        futures[-1].add_done_callback(lambda f: release.set())                                            # ... until they are cancelled
        made[item] = futures
        return item, futures

    batches = P.prefetch(range(3), start, 1)
    assert next(batches) == 0
    batches.close()
    assert release.is_set() and all(f.cancelled() for f in made[1][1:]) and 2 not in made
    assert not _decode_threads()


def test_prefetch_of_nothing_yields_nothing_and_makes_no_pool(monkeypatch):
    def no_pool(*a, **k):
        raise AssertionError("a pool for no items")

    def start(pool, slot, item):
        raise AssertionError("nothing to start")

    monkeypatch.setattr(P, "ThreadPoolExecutor", no_pool)
    assert list(P.prefetch([], start, 4)) == [] and list(P.prefetch(iter(()), start, 4)) == []


# ------------------------------------------------------------------------------------------------------------------ writer ring
def _release_once(started: threading.Event, gate: threading.Event, log: list):
    """A thread that opens `gate` once `started` is set."""
    def run():
        if started.wait(LIMIT):
            log.append("released")
            gate.set()
    t = threading.Thread(target=run)
    t.start()
    return t


def test_take_waits_for_the_writers_of_its_slot():
    started, gate, log = threading.Event(), threading.Event(), []

    def writer():
        started.set()
        gate.wait(LIMIT)
        log.append("written")

    with P.WriterRing(False, 2, "zutis-write") as ring:
        ring.submit(0, writer)
        host, dev = ring.take(1, 64)                                    # the other slot: nothing to wait for
        assert log == [] and host.numel() == 64 and dev is None
        t = _release_once(started, gate, log)
        host, dev = ring.take(0, 100)
        log.append("taken")
        t.join()
    assert log == ["released", "written", "taken"] and host.numel() == 100 and not host.is_pinned()
    assert not [t for t in threading.enumerate() if t.name.startswith("zutis-write")]


def test_drain_waits_for_every_writer_and_raises_the_first_failure():
    started, gate, log = threading.Event(), threading.Event(), []

    def fails(e):
        raise e

    def slow():
        started.set()
        gate.wait(LIMIT)
        log.append("slow writer done")

    with P.WriterRing(False, 3, "zutis-rle") as ring:
        ring.submit(0, fails, ValueError("first"))
        ring.submit(0, slow)
        ring.submit(0, fails, OSError("second"))
        t = _release_once(started, gate, log)
        with pytest.raises(ValueError, match="first"):
            ring.drain(0)
        assert log == ["released", "slow writer done"]                  # drain came back only after the slow one
        t.join()
        ring.drain()                                                    # the slot is empty again: nothing is raised twice


def test_buffers_regrow_only_past_their_capacity_and_by_a_quarter():
    buf = P.DoubleBuffer(False)
    a = buf.take(0, 100)
    assert a.numel() == 100 and buf.buffers[0].numel() == 125 and buf.buffers[1].numel() == 0
    ptr = buf.buffers[0].data_ptr()
    assert buf.take(0, 7).data_ptr() == ptr and buf.take(0, 125).data_ptr() == ptr and buf.buffers[0].numel() == 125
    assert buf.take(0, 126).numel() == 126 and buf.buffers[0].numel() == 126 + 126 // 4
    assert buf.take(1, 3).numel() == 3 and buf.buffers[1].numel() == 3
    with P.WriterRing(False, 0, "zutis-write") as ring:                 # the ring's host side is that class
        ring.take(0, 1000)
        assert isinstance(ring.host, P.DoubleBuffer) and ring.host.buffers[0].numel() == 1250 and ring.pool is None


def test_thread_split_by_share():
    half = lambda n: P.thread_split(n, 0.5)                             # noqa: E731  — the values test_predict_files_cpu.py pins
    assert half(16) == (8, 8) and half(64) == (8, 8)
    assert half(2) == (1, 1) and half(3) == (2, 1) and half(5) == (3, 2)
    assert half(1) == (1, 1)
    for n in range(2, 40):
        d, w = half(n)
        assert d >= 1 and w >= 1 and d + w == min(n, 16)
    for n in range(1, 41):                                              # pseudo-labels: a quarter, at least one
        total = max(2, min(n, 16))
        assert P.thread_split(n, 0.25) == (total - max(1, total // 4), max(1, total // 4))
