"""Developer tool: the GEMM dispatcher's plans (csrc/gemm_dispatch.h, asked through zh_dev_gemm_plan) over the case list of
tests/_gemm_plan_case.py — the check that a change to the dispatcher changed no choice.

    python tools/gemm_plan_table.py --write FILE     # the library's plans as a golden file (before a change; or from a record, below)
    python tools/gemm_plan_table.py --check FILE     # every group's case count and digest against FILE
    python tools/gemm_plan_table.py --show GROUP     # the canonical lines of one group, e.g. "x3 tile=0 tile_small=0"

FILE (tests/golden/gemm_plans.json) keeps, per group (mode x forced tile code x tile_small), the case count and the sha256 of the
canonical lines `M N K batch ... -> family code tile_m x tile_n path` (a peeled call: `-> peel M' ; first call ; second call`).
The committed file was written from a record of what the dispatchers launched BEFORE they were rewritten onto the plan functions
(write_golden() with the lines of that record), not from the library it checks.  Nothing is launched; no GPU needed."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import _gemm_plan_case as PC  # noqa: E402


def write_golden(path, lines_of_group):
    """lines_of_group(group) -> canonical lines.  One line per group: diffs stay readable."""
    with open(path, "w") as f:
        rows = []
        for g in PC.groups():
            lines = lines_of_group(g)
            rows.append("  %s: %s" % (json.dumps(PC.group_name(g)), json.dumps({"cases": len(lines), "sha256": PC.digest(lines)})))
        f.write('{"groups": {\n' + ",\n".join(rows) + "\n }}\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--write", metavar="FILE")
    g.add_argument("--check", metavar="FILE")
    g.add_argument("--show", metavar="GROUP")
    a = ap.parse_args()
    from zutis_amd import _lib
    L = _lib.load(raw=True)
    names = {PC.group_name(g): g for g in PC.groups()}
    if a.show:
        if a.show not in names:
            ap.error(f"no group {a.show!r}; groups look like {next(iter(names))!r}")
        print("\n".join(PC.group_lines(L, names[a.show])))
        return 0
    if a.write:
        write_golden(a.write, lambda grp: PC.group_lines(L, grp))
        return 0
    gold = json.load(open(a.check))["groups"]
    bad = sorted(set(gold) ^ set(names))
    total = 0
    for name, grp in names.items():
        lines = PC.group_lines(L, grp)
        total += len(lines)
        want = gold.get(name, {})
        if (len(lines), PC.digest(lines)) != (want.get("cases"), want.get("sha256")):
            bad.append(name)
            print(f"{name}: DIFFERS ({len(lines)} cases, {want.get('cases')} there); --show {name!r} on either side gives the lines")
    print(f"{len(names)} groups, {total} cases: " + ("identical" if not bad else f"{len(bad)} groups differ"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
