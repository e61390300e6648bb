"""The route ledger of sort.hip's host half.  Every launch group of a sort runs under a profile name, so ops.profile_stats() after one
ops.sort is a complete trace of the route it took: which narrowing, which full sort, how many passes, whether the keys were packed
twice.  Each case of tests/sort_route_cases.py must give the oracle's stable order position by position AND exactly the
{name: [calls, bytes]} that tests/golden/sort_routes.json holds for it (integers computed on the host: no tolerance).  The golden file
is a recording of `python -m tests.sort_route_cases` on an MI355X; a change that is meant to move a route records it again and says so."""
import json
import os
import time

import pytest

from tests import sort_route_cases as SC
from tests.util import assert_tables_equal

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sort_routes.json")


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_case_is_in_the_golden_file_and_the_oracle_accepts_it():
    from oracle import oracle
    names = [c.name for c in SC.CASES]
    assert len(set(names)) == len(names) and set(names) == set(golden())
    t0 = time.perf_counter()
    tables = [c.table() for c in SC.CASES]
    assert time.perf_counter() - t0 < 10, "the case list must build in a few seconds"
    for c, t in zip(SC.CASES, tables):
        exp = oracle.sort(t, c.keys, c.fetch)
        assert exp.num_rows == (t.num_rows if c.fetch is None else min(c.fetch, t.num_rows)) and exp.schema == t.schema, c.name


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in SC.CASES])
def test_sort_route_ledger(name):
    from oracle import oracle
    case = SC.BY_NAME[name]
    got, ledger = SC.run(case)
    assert_tables_equal(got, oracle.sort(case.table(), case.keys, case.fetch), ordered=True)
    assert ledger == golden()[name], (name, ledger)
