"""oracle/_ref/graph_cases without a GPU: the reference side of every per-node parity case
(tests/test_gpu_graph_nodes.py) and the proof that the driver's comparator bites.

--ref-only runs the reference's ggml_graph_compute alone and prints an FNV-1a hash of every
checked tensor's logical elements; tests/golden/graph_cases.json holds those hashes as recorded
from the reference (`python tests/test_graph_cases_cpu.py` rewrites it), so a case whose inputs
or graph drift shows here.  --against-threads U pushes a second reference run, at U threads,
through the same comparator that the device run goes through: the cases whose sums are grouped
by the thread count must then report mismatches, every other case none.
"""
import json
import os
import re

import pytest

from test_gpu_graph_nodes import CASES, REFUSALS, THREAD_GROUPED, check_lines, run_case

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_cases.json")
HASH = re.compile(r"^HASH (\S+) (\S+) elems=(\d+) fnv1a=([0-9a-f]{16})$")


def hashes(out):
    got = {}
    for ln in out.splitlines():
        if ln.startswith("HASH"):
            m = HASH.match(ln)
            assert m, ln
            got[m.group(2)] = f"{m.group(3)}:{m.group(4)}"
    return got


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_covers_the_case_list():
    assert sorted(golden()) == sorted(CASES)


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("name", CASES)
def test_reference_hashes(name, threads):
    r = run_case(name, threads, "--ref-only")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = hashes(r.stdout)
    assert got and got == golden()[name][str(threads)]
    if name in REFUSALS:  # the refused graph is not shown to the reference, which asserts on some
        assert "SKIP" in r.stdout and list(got) == ["after"]


@pytest.mark.parametrize("name", THREAD_GROUPED)
def test_comparator_bites_on_thread_grouping(name):
    """1 thread against 4: a real last-bits difference, found by the comparator the device
    run is judged by, and reported through the exit status."""
    r = run_case(name, 1, "--against-threads", "4", "--ref-only")
    checks = check_lines(r.stdout)
    assert checks and all(m > 0 for _, m in checks.values()), r.stdout
    assert r.returncode == 1
    assert golden()[name]["1"] != golden()[name]["4"]


@pytest.mark.parametrize("name", [c for c in CASES if c not in THREAD_GROUPED])
def test_comparator_passes_thread_independent_cases(name):
    r = run_case(name, 1, "--against-threads", "4", "--ref-only")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    checks = check_lines(r.stdout)
    assert checks and all(m == 0 and n > 0 for n, m in checks.values()), r.stdout


if __name__ == "__main__":  # record the golden hashes from the reference's run
    import subprocess
    import sys

    from test_gpu_graph_nodes import CASES_BIN

    rec = {}
    for case in CASES:
        rec[case] = {}
        for t in (1, 4):
            p = subprocess.run([CASES_BIN, case, "--threads", str(t), "--ref-only"], capture_output=True, text=True)
            if p.returncode != 0:
                sys.exit(f"{case} at {t} threads: exit status {p.returncode}\n{p.stdout}{p.stderr}")
            rec[case][str(t)] = hashes(p.stdout)
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
