"""Developer tool: the engines' launch traces (tests/_launch_trace.py) — the check that an engine refactor changed no launch.

    python tools/launch_trace.py --write FILE [--commit HASH]   # at the PARENT commit (a scratch worktree): the golden file
    python tools/launch_trace.py --check FILE                   # at the head: every case call for call against FILE
    python tools/launch_trace.py --show CASE                    # the full canonical lines of one case (either side of a mismatch)

FILE (tests/golden/launch_traces.json) keeps the commit it was written at and, per case, the call count and per call
`entry:first 12 hex digits of sha256(canonical line)`.  Nothing is launched; needs a GPU for the allocations only."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import _launch_trace as LT  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--write", metavar="FILE")
    g.add_argument("--check", metavar="FILE")
    g.add_argument("--show", metavar="CASE", choices=sorted(LT.CASES))
    ap.add_argument("--commit", help="hash recorded by --write (default: git rev-parse HEAD)")
    a = ap.parse_args()
    if a.show:
        for i, ln in enumerate(LT.run_case(a.show)):
            print(f"{i:4d} {ln}")
        return 0
    if a.write:
        commit = a.commit or subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, check=True, capture_output=True, text=True).stdout.strip()
        cases = {}
        for name in LT.CASES:
            d = LT.digests(LT.run_case(name))
            cases[name] = {"calls": len(d), "digests": d}
            print(f"{name}: {len(d)} calls")
        with open(a.write, "w") as f:       # one line per case: diffs stay readable
            f.write('{"commit": %s,\n "cases": {\n' % json.dumps(commit))
            f.write(",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in cases.items()))
            f.write("\n }}\n")
        return 0
    gold = json.load(open(a.check))
    bad = 0
    for name in LT.CASES:
        lines = LT.run_case(name)
        got, want = LT.digests(lines), gold["cases"][name]["digests"]
        k = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), None if len(got) == len(want) else min(len(got), len(want)))
        if k is None:
            print(f"{name}: {len(got)} calls, identical")
        else:
            bad += 1
            print(f"{name}: DIFFERS from {gold['commit'][:7]} at call {k} ({len(got)} calls, {len(want)} there): "
                  f"{lines[k] if k < len(lines) else '(no such call here)'}  [there: {want[k] if k < len(want) else '(none)'}]")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
