"""-m gpu: the launch sequence of every engine — entry points, scalar arguments, buffer aliases (tests/_launch_trace.py) — equals
tests/golden/launch_traces.json, written by tools/launch_trace.py at the commit named inside it.  An engine refactor that means to
change no launch passes unchanged; one that means to change some regenerates the file and says which.  Nothing is launched."""
import json
import os

import pytest

import _launch_trace as LT

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_traces.json")))


def test_golden_file_covers_the_cases():
    assert sorted(GOLDEN["cases"]) == sorted(LT.CASES) and len(GOLDEN["commit"]) == 40
    assert all(c["calls"] == len(c["digests"]) > 0 for c in GOLDEN["cases"].values())


@pytest.mark.parametrize("name", sorted(LT.CASES))
def test_launch_trace_equals_golden(dev, name):
    lines = LT.run_case(name)
    got, want = LT.digests(lines), GOLDEN["cases"][name]["digests"]
    i = next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), None if len(got) == len(want) else min(len(got), len(want)))
    if i is not None:                       # a differing call, or the first call one side has and the other lacks
        print(f"{name}: first differing call {i} ({len(got)} calls here, {len(want)} golden): {lines[i] if i < len(lines) else '(no such call here)'}\n"
              f"  golden ({GOLDEN['commit'][:12]}): {want[i] if i < len(want) else '(no such call there)'}   "
              f"(python tools/launch_trace.py --show {name} on a worktree of that commit gives its full line)")
    assert len(got) == GOLDEN["cases"][name]["calls"] and got == want
