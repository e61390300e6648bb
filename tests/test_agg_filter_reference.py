"""tests/agg_filter_ref.py — the reference of aggregates with FILTER (WHERE ...) — held to the oracle through the CASE spelling, on the
tables the GPU tests use: `func(x) FILTER (WHERE p)` is `func(CASE WHEN p THEN x END)`, `COUNT(*) FILTER (WHERE p)` is `COUNT(CASE
WHEN p THEN 1 END)`.  Then four wrong implementations, each of which must differ from the reference on those tables, and the header's
side of the feature: ABI 16 and `has_filter` / `filter` behind `return_field` in dfgpu_agg_spec."""
import os
import re
import statistics
from decimal import Decimal

import pyarrow as pa
import pytest

from tests import agg_filter_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARROW = {"k": pa.int64(), "row": pa.int64(), "i32": pa.int32(), "i64": pa.int64(), "f64": pa.float64(), "dec": pa.decimal128(15, 2), "b": pa.bool_(), "u": pa.int64(),
         "p": pa.bool_(), "pf": pa.bool_(), "pt": pa.bool_(), "np_": pa.bool_()}
ORACLE_FUNCS = ("sum", "min", "max", "count", "avg")          # what oracle.aggregate implements


def to_arrow(table, names=None):
    return pa.table({c: pa.array(table[c], ARROW[c]) for c in (names or table)})


def _oracle_rows(table, keys, aggs, predicate=None):
    from oracle import oracle
    t = to_arrow(table)
    if predicate is not None:
        t = oracle.filter(t, ("col", predicate), t.column_names)
    case_aggs = []
    for func, arg, name, flt in aggs:
        x = ("lit", 1, pa.int64()) if arg is None else ("col", arg)
        if flt is None:
            case_aggs.append((func, None if arg is None else x, name))
        else:
            case_aggs.append((func, ("case", ("col", flt), x, None), name))
    return oracle.aggregate(t, [(("col", k), k) for k in keys], case_aggs, "Single").to_pylist()


@pytest.mark.parametrize("n", R.ROW_COUNTS)
@pytest.mark.parametrize("keys", [["k"], []])
@pytest.mark.parametrize("predicate", [None, "np_"])
def test_reference_agrees_with_the_oracle_through_the_case_spelling(n, keys, predicate):
    table = R.make_table(n)
    aggs = [a for a in R.main_aggs() if a[0] in ORACLE_FUNCS]
    want = _oracle_rows(table, keys, aggs, predicate)
    got = R.aggregate(table, keys, aggs, predicate)
    assert len(got) == len(want) and (keys or len(got) == 1)
    for g, w in zip(got, want):                     # both in first-seen order
        assert g == w, {c: (g[c], w[c]) for c in g if g[c] != w[c]}


def test_the_tables_hold_the_rows_the_tests_need():
    table = R.make_table(4097)
    rows = {r["k"]: r for r in R.aggregate(table, ["k"], R.main_aggs())}
    n = len(table["k"])
    # groups straddle the 64-row words; runs of 1, 63, 64 and 65 rows
    lengths = {}
    for k in table["k"]:
        lengths[k] = lengths.get(k, 0) + 1
    assert set(R.RUNS) <= set(lengths.values())
    # a group with no surviving row for one aggregate while another aggregate of the node sees all of its rows
    dead = [k for k, r in rows.items() if r["cnt"] == 0]
    assert any(lengths[k] == 64 for k in dead) and any(lengths[k] == 1 for k in dead)
    for k in dead:
        assert rows[k]["plain_cnt"] == lengths[k] and rows[k]["sum_i64"] is None and rows[k]["count_i64"] == 0 and rows[k]["bor"] is None
    assert any(rows[k]["plain_sum"] is not None for k in dead)
    # argument NULL where the filter is TRUE, and the reverse
    assert any(table["p"][i] is True and table["i64"][i] is None for i in range(n))
    assert any(table["p"][i] is not True and table["i64"][i] is not None for i in range(n))
    assert {True, False, None} == set(table["p"]) and set(table["pf"]) == {False} and set(table["pt"]) == {True}
    # the all-FALSE filter gives "nothing seen" everywhere, the all-TRUE one nothing but the plain aggregate
    assert all(r["none_sum"] is None and r["none_cnt"] == 0 and r["all_cnt"] == r["plain_cnt"] for r in rows.values())
    # without GROUP BY, everything filtered out, and over no rows at all: one row of "nothing seen"
    for t in (table, R.make_table(0)):
        (whole,) = R.aggregate(t, [], [("sum", "i64", "s", "pf"), ("count", None, "c", "pf"), ("count", "i64", "cx", "pf"), ("avg", "dec", "a", "pf")])
        assert whole == {"s": None, "c": 0, "cx": 0, "a": None}


def test_known_answers():
    t = {"k": [1, 1, 1, 2, 2, 3], "x": [10, None, 30, 5, 6, 7], "d": [Decimal("1.00"), Decimal("2.00"), Decimal("0.01"), None, Decimal("5.55"), Decimal("1.11")],
         "p": [True, True, False, None, False, True]}
    aggs = [("sum", "x", "s", "p"), ("count", None, "c", "p"), ("count", "x", "cx", "p"), ("avg", "d", "a", "p"), ("max", "x", "m", None)]
    assert R.aggregate(t, ["k"], aggs) == [{"k": 1, "s": 10, "c": 2, "cx": 1, "a": Decimal("1.500000"), "m": 30},
                                           {"k": 2, "s": None, "c": 0, "cx": 0, "a": None, "m": 6},
                                           {"k": 3, "s": 7, "c": 1, "cx": 1, "a": Decimal("1.110000"), "m": 7}]
    assert R.reduce("avg", [Decimal("0.01"), Decimal("0.01"), Decimal("0.02")]) == Decimal("0.013333")          # truncating, not rounding
    assert R.reduce("avg", [Decimal("-0.01"), Decimal("-0.01"), Decimal("-0.03")]) == Decimal("-0.016666")


def test_variance_reference_agrees_with_the_statistics_module():
    t = R.variance_table()
    aggs = [("var_samp", "x", "vs", "p"), ("var_pop", "x", "vp", "p"), ("stddev_samp", "x", "ss", "p"), ("stddev_pop", "x", "sp", "p"), ("count", "x", "n", "p")]
    rows = {r["k"]: r for r in R.aggregate(t, ["k"], aggs)}
    assert {r["n"] for r in rows.values()} == {0, 1, 2, 4}
    for k, r in rows.items():
        xs = [x for kk, x, p in zip(t["k"], t["x"], t["p"]) if kk == k and p is True and x is not None]
        assert r["vs"] == (statistics.variance(xs) if len(xs) > 1 else None) and r["vp"] == (statistics.pvariance(xs) if xs else None), k
        assert r["ss"] == (statistics.stdev(xs) if len(xs) > 1 else None) and r["sp"] == (statistics.pstdev(xs) if xs else None), k
    assert rows[3]["vs"] is None and rows[3]["vp"] == 0.0 and rows[4]["vp"] is None and rows[2]["vs"] == 20.0 / 3.0


# ---------------------------------------------------------------------- wrong implementations
def _wrong(table, keys, aggs, mistake):
    """R.aggregate with one of the mistakes an implementation of FILTER can make"""
    n = len(table["k"])
    first_filter = next(a[3] for a in aggs if a[3] is not None)
    groups = {}
    for i in range(n):
        if mistake == "filter_drops_the_group" and table[first_filter][i] is not True:
            continue                                            # the filter applied as a node predicate: rows it drops make no group
        groups.setdefault(tuple(table[k][i] for k in keys), []).append(i)
    out = []
    for kt, rows in groups.items():
        row = dict(zip(keys, kt))
        leaked = None
        for func, arg, name, flt in aggs:
            if mistake == "filter_leaks_to_the_next_aggregate" and flt is None:
                flt = leaked                                    # the aggregate next to a filtered one takes its mask
            leaked = flt
            if mistake == "count_star_ignores_the_filter" and arg is None:
                flt = None
            passes = (lambda v: v is not False) if mistake == "null_filter_taken_as_true" else (lambda v: v is True)
            kept = [i for i in rows if flt is None or passes(table[flt][i])]
            values = [1] * len(kept) if arg is None else [table[arg][i] for i in kept if table[arg][i] is not None]
            row[name] = R.reduce(func, values)
        out.append(row)
    return out


@pytest.mark.parametrize("n", [65, 4097])
@pytest.mark.parametrize("mistake, shows_in", [("filter_drops_the_group", None), ("null_filter_taken_as_true", "sum_i64"), ("count_star_ignores_the_filter", "cnt"),
                                               ("filter_leaks_to_the_next_aggregate", "plain_cnt")])
def test_wrong_implementations_differ_from_the_reference(mistake, shows_in, n):
    table, aggs = R.make_table(n), R.main_aggs()
    ref = R.aggregate(table, ["k"], aggs)
    assert _wrong(table, ["k"], aggs, None) == ref              # the restatement itself is right
    bad = _wrong(table, ["k"], aggs, mistake)
    if shows_in is None:
        assert len(bad) < len(ref)                              # whole groups are missing
        return
    assert len(bad) == len(ref) and any(b[shows_in] != r[shows_in] for b, r in zip(bad, ref)), mistake


# ---------------------------------------------------------------------- the header
def test_the_header_carries_the_filter_behind_return_field():
    from datafusion_amd import _lib
    header = open(os.path.join(ROOT, "include", "dfgpu.h")).read()
    assert int(re.search(r"#define DFGPU_ABI_VERSION (\d+)", header).group(1)) >= 16
    body = re.search(r"typedef struct dfgpu_agg_spec \{(.*?)\} dfgpu_agg_spec;", header, re.S).group(1)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == ["func", "has_arg", "arg", "name", "return_field", "has_filter", "filter"], fields
    assert re.search(r"int32_t\s+has_filter;", body) and re.search(r"dfgpu_expr\s+filter;", body)
    assert [f[0] for f in _lib.AggSpec._fields_] == fields      # the ctypes mirror, name by name
    assert _lib.AggSpec().has_filter == 0                       # a zeroed struct has no filter
