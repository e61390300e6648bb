"""tests/window_ref.py held to known answers and to the oracle, and shown to tell wrong window evaluators apart (no GPU needed).

The hand-worked cases are the specification's.  On the 200-row table of tests/window_cases.py every aggregate window value is checked
against oracle.aggregate: the `partition` frame against the aggregate grouped by the partition keys, broadcast back to the rows, and each
row's `rows_to_current` / `range_to_current` value against the aggregate over exactly that frame's rows (one grouped call: group g holds
the rows of row g's frame).  Float64 SUM / AVG are rationals in the restatement; the oracle's doubles are held to them by the bound of
tests/float_sum_ref.py with m additions (m - 1 of the values, one for an accumulator that starts at 0.0).  The last tests run mistaken
evaluators over the same table and require each to differ from the restatement there — the table is what the GPU tests' inputs imitate."""
import functools
import math
import struct
from fractions import Fraction

import pyarrow as pa
import pytest

from tests import float_sum_ref as R
from tests import window_cases as WC
from tests import window_ref as W


def _bits(x):
    return None if x is None else struct.pack("<d", x)


HAND = {"p": ["a", "a", "a", "a", "b", "b"], "o": [1, 1, 2, 3, 5, 5], "v": [10, 20, 30, 40, 1, 2]}


def test_hand_worked_case():
    got = W.window(HAND, {"v": "int64"}, ["p"], ["o"],
                   [("row_number", None, "rn", None), ("rank", None, "rk", None), ("dense_rank", None, "dr", None), ("sum", "v", "s_range", "range_to_current"),
                    ("sum", "v", "s_default", None), ("sum", "v", "s_rows", "rows_to_current"), ("sum", "v", "s_part", "partition")])
    assert got["rn"] == [1, 2, 3, 4, 1, 2]
    assert got["rk"] == [1, 1, 3, 4, 1, 1]
    assert got["dr"] == [1, 1, 2, 3, 1, 1]
    assert got["s_range"] == got["s_default"] == [30, 30, 60, 100, 3, 3]
    assert got["s_rows"] == [10, 30, 60, 100, 1, 3]
    assert got["s_part"] == [100, 100, 100, 100, 3, 3]


def test_hand_worked_case_with_nulls():
    cols = dict(HAND, v=[None, None, 30, 40, 1, 2])
    got = W.window(cols, {"v": "int64"}, ["p"], ["o"], [("sum", "v", "s", "range_to_current"), ("count", "v", "c", "range_to_current"), ("count", None, "n", "range_to_current")])
    assert got["s"] == [None, None, 30, 70, 3, 3]
    assert got["c"] == [0, 0, 1, 2, 2, 2]
    assert got["n"] == [2, 2, 3, 4, 2, 2]


def test_no_keys_and_wrapping():
    cols = {"v": [2**63 - 1, 1, None], "d": [2**127 - 1, 1, 5]}
    types = {"v": "int64", "d": ("decimal", 38, 0)}
    got = W.window(cols, types, [], [], [("sum", "v", "s", None), ("sum", "v", "r", "rows_to_current"), ("sum", "d", "ds", "rows_to_current"), ("rank", None, "rk", None),
                                         ("row_number", None, "rn", None), ("avg", "d", "da", "rows_to_current")])
    assert got["s"] == [-2**63] * 3                       # no order keys: every row is a peer of every other, and Int64 sums wrap
    assert got["r"] == [2**63 - 1, -2**63, -2**63]
    assert got["ds"] == [2**127 - 1, -2**127, -2**127 + 5]  # Decimal128 sums wrap at 128 bits
    assert got["rk"] == [1, 1, 1] and got["rn"] == [1, 2, 3]
    assert got["da"][0] == (2**127 - 1) * 10**4 and got["da"][1] == -((2**127 * 10**4) // 2)   # truncating toward zero at scale + 4


# ------------------------------------------------------------------------------------------------------------------ against the oracle
@functools.lru_cache(maxsize=None)
def _table():
    cols, types = WC.reference_table()
    return cols, types, WC.to_arrow(cols, types), WC.frames(cols, WC.PARTITION_LENGTHS, ["o"])


def _specs(frame):
    return [(f, a, f"{f}_{a}", frame) for a in WC.ARGS for f in WC.FUNCS_OF[a]] + [("count", None, "count_star", frame)]


def _oracle_aggs(specs):
    return [(f, None if a is None else ("col", a), n) for f, a, n, _ in specs]


def _hold(label, func, tag, want, got):
    """one window value of the restatement against the oracle's aggregate over the same rows"""
    if isinstance(want, W.FloatSum):
        assert got is not None, label
        sum_bound = R.gamma(want.m) * want.S
        if func == "sum":
            assert R.within(got, want.exact, sum_bound), (label, got, want)
        else:
            avg = want.exact / want.m
            assert R.within(got, avg, sum_bound / want.m + R.U * abs(avg) + Fraction(1, 2**1075)), (label, got, want)
    elif tag == "float64" and func in ("min", "max"):
        assert _bits(got) == _bits(want), (label, got, want)
    else:
        assert got == want and type(got) is type(want), (label, got, want)


def test_table_is_what_the_mistakes_need():
    cols, types, _, fr = _table()
    n = len(cols["o"])
    assert n == 200 and sum(WC.PARTITION_LENGTHS) == n
    heads = [a for a, _, _, _ in fr if True]
    assert {64, 128} <= set(heads)                                             # partition heads on 64-row word edges
    assert any(e > i for _, i, e, _ in fr)                                     # peer groups of more than one row
    assert any(v is None for v in cols["p1"]) and any(v is None for v in cols["p2"]) and any(v is None for v in cols["o"])
    assert all(any(v is None for v in cols[a]) for a in WC.ARGS)
    assert any(isinstance(v, float) and math.isnan(v) for v in cols["fe"]) and _bits(-0.0) in map(_bits, cols["fe"]) and _bits(0.0) in map(_bits, cols["fe"])


def test_partition_frame_equals_the_grouped_aggregate_broadcast_to_rows():
    from oracle import oracle
    cols, types, table, fr = _table()
    specs = _specs("partition")
    want = W.window(cols, types, ["p1", "p2"], ["o"], specs)
    agg = oracle.aggregate(table, [(("col", "p1"), "p1"), (("col", "p2"), "p2")], _oracle_aggs(specs))
    assert list(zip(agg.column("p1").to_pylist(), agg.column("p2").to_pylist())) == list(WC.PARTITION_KEYS)     # groups in first-seen order
    part_of = [p for p, length in enumerate(WC.PARTITION_LENGTHS) for _ in range(length)]
    for f, a, name, _ in specs:
        tag = WC.result_tag(f, None if a is None else types[a])
        per_group = WC.from_array(agg.column(name), tag)
        for i, p in enumerate(part_of):
            _hold((name, i), f, tag, want[name][i], per_group[p])


@pytest.mark.parametrize("frame", ["rows_to_current", "range_to_current"])
def test_running_frames_equal_the_aggregate_over_exactly_the_frames_rows(frame):
    from oracle import oracle
    cols, types, table, fr = _table()
    specs = _specs(frame)
    want = W.window(cols, types, ["p1", "p2"], ["o"], specs)
    take, gid = [], []
    for g, (start, rows_end, range_end, _) in enumerate(fr):
        end = rows_end if frame == "rows_to_current" else range_end
        take += range(start, end + 1)
        gid += [g] * (end + 1 - start)
    expanded = table.take(pa.array(take, type=pa.int64())).append_column("gid", pa.array(gid, type=pa.int64()))
    agg = oracle.aggregate(expanded, [(("col", "gid"), "gid")], _oracle_aggs(specs))
    assert agg.column("gid").to_pylist() == list(range(len(fr)))
    for f, a, name, _ in specs:
        tag = WC.result_tag(f, None if a is None else types[a])
        got = WC.from_array(agg.column(name), tag)
        for i in range(len(fr)):
            _hold((name, frame, i), f, tag, want[name][i], got[i])


# ------------------------------------------------------------------------------------------------------------------- wrong evaluators
def _ref(specs, cols=None, partition_by=("p1", "p2"), order_by=("o",)):
    c, types, _, _ = _table()
    return W.window(c if cols is None else cols, types, list(partition_by), list(order_by), specs)


SUM = [("sum", "i64", "s", "range_to_current")]


def test_range_frame_computed_as_rows_differs():
    assert _ref(SUM)["s"] != _ref([("sum", "i64", "s", "rows_to_current")])["s"]


def test_rank_computed_as_dense_rank_differs():
    got = _ref([("rank", None, "r", None), ("dense_rank", None, "d", None)])
    assert got["r"] != got["d"]


def test_missing_the_boundary_where_only_the_second_partition_key_changes_differs():
    specs = SUM + [("row_number", None, "rn", None)]
    right, wrong = _ref(specs), _ref(specs, partition_by=("p1",))
    assert right["s"] != wrong["s"] and right["rn"] != wrong["rn"]


def test_null_keys_treated_as_unequal_differs():
    cols, _, _, _ = _table()
    apart = dict(cols)
    for k in ("p1", "p2", "o"):     # every NULL key becomes a value no other row holds: NULL != NULL
        apart[k] = [v if v is not None else 10**6 + i for i, v in enumerate(cols[k])]
    specs = SUM + [("row_number", None, "rn", None), ("rank", None, "rk", None)]
    right, wrong = _ref(specs), _ref(specs, cols=apart)
    assert right["s"] != wrong["s"] and right["rn"] != wrong["rn"] and right["rk"] != wrong["rk"]
    only_order = dict(cols, o=apart["o"])
    assert _ref(specs)["rk"] != _ref(specs, cols=only_order)["rk"]


def test_null_argument_read_as_the_value_in_its_buffer_differs():
    cols, _, _, _ = _table()
    filled = dict(cols, i64=[77 if v is None else v for v in cols["i64"]])
    for frame in W.FRAMES:
        specs = [("sum", "i64", "s", frame), ("min", "i64", "lo", frame), ("count", "i64", "c", frame)]
        right, wrong = _ref(specs), _ref(specs, cols=filled)
        assert right["s"] != wrong["s"] and right["c"] != wrong["c"]


def test_a_carry_that_survives_a_partition_boundary_on_a_word_edge_differs():
    cols, _, _, fr = _table()
    merged = {k: list(v) for k, v in cols.items()}
    for i in range(len(fr)):                       # the heads at rows 64 and 128 go unnoticed: those partitions take their predecessor's keys
        start = fr[i][0]
        if start % 64 == 0 and start > 0:
            merged["p1"][i], merged["p2"][i] = merged["p1"][start - 1], merged["p2"][start - 1]
    specs = [("sum", "i64", "s", "rows_to_current"), ("max", "i32", "hi", "rows_to_current"), ("row_number", None, "rn", None)]
    right, wrong = _ref(specs), _ref(specs, cols=merged)
    for name in ("s", "hi", "rn"):
        assert right[name][64:129] != wrong[name][64:129], name
        assert right[name][:64] == wrong[name][:64]


def test_sum_over_no_value_giving_zero_differs():
    right = _ref([("sum", "i64", "s", f) for f in W.FRAMES][:1] + [("sum", "i64", "rows", "rows_to_current"), ("sum", "i64", "part", "partition")])
    for name, col in right.items():
        assert None in col and [0 if v is None else v for v in col] != col, name


def test_count_of_a_column_counting_nulls_differs():
    for frame in W.FRAMES:
        got = _ref([("count", "i64", "c", frame), ("count", None, "n", frame)])
        assert got["c"] != got["n"]
