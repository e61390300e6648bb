"""The route ledger of join_probe's host code (join.hip).  Every launch group of a probe runs under a profile name, so
ops.profile_stats() after one probe is a complete trace of the route it took: which flavour, whether the sample was asked, whether a
speculation missed, which lazily built structure of the join table was made; ht.info() holds the two counters the probe keeps.  Each
case of tests/join_route_cases.py must give the oracle's rows — in probe order where the flavour promises it, as a multiset otherwise —
AND exactly what tests/golden/join_routes.json holds for it: {name: [calls, bytes]}, [probe_rows, output_rows], or the error's text
(integers computed on the host: no tolerance).  The golden file is a recording of `python -m tests.join_route_cases` on an MI355X with
the library built at 3e40503, the commit before join_probe became a plan, a core and one function per flavour; a change that is meant
to move a route records it again and says so.  (The test_zzz_ prefix: the module is collected after every test that was there before it.)"""
import json
import os
import time

import pytest

from tests import join_route_cases as JC
from tests.util import assert_tables_equal

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "join_routes.json")


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_case_is_in_the_golden_file_and_the_oracle_accepts_it():
    names = [c.name for c in JC.CASES]
    assert len(set(names)) == len(names) and set(names) == set(golden())
    t0 = time.perf_counter()
    tables = [(c.build(), c.probe()) for c in JC.CASES]
    assert time.perf_counter() - t0 < 10, "the case list must build in a few seconds"
    for c, (b, p) in zip(JC.CASES, tables):
        assert all(l in b.column_names and r in p.column_names for l, r in c.on), c.name
        if "error" in golden()[c.name]:
            continue
        exp = JC.expected(c)
        if c.join_type in ("Inner", "Right", "RightSemi", "RightAnti", "RightMark"):   # no tail of build rows: the probe's own output
            rows = exp.column("rows")[0].as_py() if exp.column_names == ["rows"] else exp.num_rows
            assert rows * c.probes == golden()[c.name]["info"][1], c.name


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in JC.CASES])
def test_join_route_ledger(name):
    case = JC.BY_NAME[name]
    want = golden()[name]
    got, ledger, counters = JC.run(case)
    if "error" in want:
        assert got is None and ledger == want, (name, ledger)
        return
    assert got is not None, (name, ledger)
    assert_tables_equal(got, JC.expected(case), ordered=case.ordered)
    assert ledger == want["profile"], (name, ledger)
    assert counters == want["info"], (name, counters)
