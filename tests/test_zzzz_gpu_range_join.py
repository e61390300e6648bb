"""dfgpu_range_join (the range join on the device) against tests/range_join_ref.py, position by position — the output order is part of
the contract — with Float64 compared by bits.  The cases are tests/range_join_cases.py's; tests/test_range_join_reference.py holds the
reference to hand-worked answers and to the pair-space reference, checks that every case has the rows it is named for, and shows that
the usual wrong range joins differ from the reference on these tables.  Every case asserts which of the operator's kernels ran.  A
test takes one case through all ten join types: the case's tables are uploaded once and its matching pairs are computed once per
process (tests.range_join_cases.pairs).

The file sorts behind every other test file on purpose: the suite is also run in slices of its collection order, and tests added in
the middle of that order move every later test into another slice."""
import numpy as np
import pyarrow as pa
import pytest

from tests import nlj_cases as NC
from tests import nlj_ref as N
from tests import range_join_cases as RC
from tests import range_join_ref as R

pytestmark = pytest.mark.gpu

CASES = RC.all_cases()
BAND = [c for c in CASES if c.name.startswith("band_")]
RIGHT_FLAG_TYPES = ("Right", "Full") + N.RIGHT_ONE_SIDED


def _profiled(call):
    """-> (the output as an Arrow table, the names of the profiled launches)"""
    from datafusion_amd import ops
    ops.profile_enable(True)
    ops.profile_reset()
    try:
        out = call()
        stats = ops.profile_stats()
    finally:
        ops.profile_enable(False)
    got = out.to_arrow()
    out.free()
    return got, set(stats)


def run_rj(dl, dr, x, lower, upper, join_type, left_cols=None, right_cols=None):
    """-> (the output as an Arrow table, the set of rangejoin_* profile names that ran)"""
    from datafusion_amd import ops
    got, names = _profiled(lambda: ops.range_join(dl, dr, x, lower, upper, join_type, left_cols, right_cols))
    assert not {k for k in names if k.startswith("nlj_")}
    return got, {k for k in names if k.startswith("rangejoin_")}


def run_nlj(dl, dr, flt, join_type):
    from datafusion_amd import ops
    got, names = _profiled(lambda: ops.nested_loop_join(dl, dr, join_type, flt))
    assert not {k for k in names if k.startswith("rangejoin_")}
    return got


class uploaded:
    """`with uploaded(left, right) as (dl, dr)`: the two tables on the device for the block"""

    def __init__(self, *tables):
        self.tables = tables

    def __enter__(self):
        from datafusion_amd.table import DeviceTable
        self.dev = [DeviceTable.from_arrow(t) for t in self.tables]
        return self.dev

    def __exit__(self, *a):
        for t in self.dev:
            t.free()


def expected_kernels(join_type, nl, nr, n_points, n_pairs):
    """what the operator launches: nothing for an empty side or a right side without a non-NULL x; the coverage only for the types that
    need right-side flags; the expansion only for the pair types, and only when a pair was counted"""
    if not (nl and nr and n_points):
        return set()
    out = {"rangejoin_keys", "rangejoin_bounds"}
    if join_type in RIGHT_FLAG_TYPES:
        out.add("rangejoin_cover")
    if join_type in N.PAIR_TYPES and n_pairs:
        out.add("rangejoin_expand")
    return out


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_every_join_type_against_the_reference(case):
    pairs = list(RC.pairs(case.name))
    n_points = case.right.num_rows - case.right.column(case.x).null_count
    with uploaded(case.left, case.right) as (dl, dr):
        for join_type in N.ALL_TYPES:
            want = R.range_join(case.left, case.right, case.x, case.lower, case.upper, join_type, pairs=pairs)
            got, kernels = run_rj(dl, dr, case.x, case.lower, case.upper, join_type)
            assert R.difference(got, want) is None, (join_type, R.difference(got, want))
            exp = expected_kernels(join_type, case.left.num_rows, case.right.num_rows, n_points, len(pairs))
            assert kernels == exp, (join_type, kernels, exp)


@pytest.mark.parametrize("case", BAND, ids=[c.name for c in BAND])
def test_the_band_cases_equal_the_nested_loop_join_in_the_same_process(case):
    with uploaded(case.left, case.right) as (dl, dr):
        for join_type in N.ALL_TYPES:
            got, _ = run_rj(dl, dr, case.x, case.lower, case.upper, join_type)
            nlj = run_nlj(dl, dr, case.filter, join_type)
            assert got.column_names == nlj.column_names and got.schema.types == nlj.schema.types
            assert [f.nullable for f in got.schema] == [f.nullable for f in nlj.schema], join_type
            if join_type in N.PAIR_TYPES:
                assert N.multiset(got) == N.multiset(nlj), join_type
            else:
                assert N.difference(got, nlj) is None, (join_type, N.difference(got, nlj))


def test_projections_subsets_reordered_and_empty():
    c = RC.by_name("band_65x63")
    pairs = list(RC.pairs(c.name))
    with uploaded(c.left, c.right) as (dl, dr):
        for join_type in N.ALL_TYPES:
            for lc, rc in ((["tag", "lo"], ["w"]), ([], ["x", "w"]), (["hi"], []), ([], []), ([2, 0, 1], [1, 0])):
                want = R.range_join(c.left, c.right, c.x, c.lower, c.upper, join_type, lc, rc, pairs=pairs)
                got, _ = run_rj(dl, dr, c.x, c.lower, c.upper, join_type, lc, rc)
                if want.num_columns == 0:     # (an Arrow table without columns cannot say how many rows the reference has: the row ids can)
                    li, ri, _ = N.index_rows(c.left.num_rows, c.right.num_rows, pairs, join_type)
                    assert got.num_columns == 0 and got.num_rows == len(li if li is not None else ri)
                    continue
                assert R.difference(got, want) is None, (join_type, lc, rc, R.difference(got, want))


def test_sliced_inputs_and_columns_at_an_offset():
    from datafusion_amd import ops
    left, right = NC.band_tables(300, 280)
    lower, upper = ("lo", True), ("hi", False)
    with uploaded(left, right) as (dl, dr):
        sl, sr = dl.slice(37, 257), dr.slice(19, 255)
        al, ar = left.slice(37, 257), right.slice(19, 255)
        pairs = R.matching_pairs(al, ar, "x", lower, upper)
        assert pairs
        for join_type in N.ALL_TYPES:
            got, _ = run_rj(sl, sr, "x", lower, upper, join_type)
            assert R.difference(got, R.range_join(al, ar, "x", lower, upper, join_type, pairs=pairs)) is None, join_type
        # partitions of a table without NULLs are views into one buffer per column: every part but the first starts at an offset
        lparts, rparts = ops.partition(dl, ["lo"], 3), ops.partition(dr, ["x"], 2)
        pl, pr = lparts[1], rparts[1]
        al, ar = pl.to_arrow(), pr.to_arrow()
        assert al.num_rows and ar.num_rows
        pairs = R.matching_pairs(al, ar, "x", lower, upper)
        for join_type in N.ALL_TYPES:
            got, _ = run_rj(pl, pr, "x", lower, upper, join_type)
            assert R.difference(got, R.range_join(al, ar, "x", lower, upper, join_type, pairs=pairs)) is None, join_type
        for t in [sl, sr] + lparts + rparts:
            t.free()


def test_refusals_by_their_messages_and_the_plan_time_reasons_are_the_same_text():
    import ctypes as C
    from decimal import Decimal

    from datafusion_amd import _lib, ops, physical_plan as P
    from datafusion_amd.table import DeviceTable
    n = 5
    left = pa.table({"lo": pa.array(range(n), type=pa.int64()), "hi": pa.array(range(1, n + 1), type=pa.int64()),
                     "dec": pa.array([Decimal(i) for i in range(n)], type=pa.decimal128(10, 0)), "s": pa.array([f"s{i}" for i in range(n)], type=pa.string()),
                     "d": pa.array([f"d{i % 2}" for i in range(n)], type=pa.string()).dictionary_encode(), "lo32": pa.array(range(n), type=pa.int32())})
    right = pa.table({"x": pa.array(range(n), type=pa.int64()), "dec": pa.array([Decimal(i) for i in range(n)], type=pa.decimal128(10, 0)),
                      "s": pa.array([f"s{i}" for i in range(n)], type=pa.string()), "d": pa.array([f"d{i % 2}" for i in range(n)], type=pa.string()).dictionary_encode()})
    with uploaded(left, right) as (dl, dr):
        refused = [
            ("dec", ("dec", True), None, P.RANGE_JOIN_KEY_TYPE),             # Decimal128 keys
            ("d", ("d", True), None, P.RANGE_JOIN_DICT_KEY),                 # dictionary-encoded keys
            ("x", ("lo", True), ("d", False), P.RANGE_JOIN_DICT_KEY),
            ("s", ("s", True), None, P.RANGE_JOIN_KEY_TYPE),                 # Utf8 keys
            ("x", ("lo32", True), None, P.RANGE_JOIN_MIXED_KEYS),            # mixed types
            ("x", ("lo", True), ("lo32", True), P.RANGE_JOIN_MIXED_KEYS),
            ("x", None, None, P.RANGE_JOIN_NO_BOUND),                        # no bound
        ]
        for x, lower, upper, msg in refused:
            for jt in ("Inner", "LeftSemi", "RightMark"):
                with pytest.raises(_lib.DfgpuError) as err:
                    ops.range_join(dl, dr, x, lower, upper, jt)
                assert str(err.value) == msg, (x, lower, upper)
                node = P.GpuRangeJoinExec(P.MemoryExec(dl, "l"), P.MemoryExec(dr, "r"), x, lower, upper, jt)
                assert P.unsupported_reason(node) == msg
            if msg != P.RANGE_JOIN_NO_BOUND:
                assert msg.endswith("is not supported on the GPU path")
        # column indices out of range
        for x, lower, upper, words in ((4, ("lo", True), None, "range join key column out of range"), (-1, ("lo", True), None, "range join key column out of range"),
                                       ("x", (6, True), None, "range join bound column out of range"), ("x", ("lo", True), (9, False), "range join bound column out of range")):
            with pytest.raises(_lib.DfgpuError, match=words):
                ops.range_join(dl, dr, x, lower, upper, "Inner")
        lib, out = _lib.load(), C.c_void_p()
        ints = lambda *v: (C.c_int * len(v))(*v)
        assert lib.dfgpu_range_join(dl.handle, dr.handle, 0, 0, 0, 1, 1, 0, ints(0, 6), 2, ints(0), 1, C.byref(out)) != 0
        assert "left output column out of range" in lib.dfgpu_last_error().decode()
        assert lib.dfgpu_range_join(dl.handle, dr.handle, 2, 0, 0, 1, 1, 0, ints(0), 1, ints(-1), 1, C.byref(out)) != 0
        assert "right output column out of range" in lib.dfgpu_last_error().decode()
        assert lib.dfgpu_range_join(dl.handle, dr.handle, 10, 0, 0, 1, 1, 0, ints(0), 1, ints(0), 1, C.byref(out)) != 0
        assert "bad join type" in lib.dfgpu_last_error().decode()
        assert lib.dfgpu_range_join(dl.handle, None, 0, 0, 0, 1, 1, 0, ints(0), 1, ints(0), 1, C.byref(out)) != 0
        assert lib.dfgpu_range_join(dl.handle, dr.handle, 0, 0, 0, 1, 1, 0, None, 1, ints(0), 1, C.byref(out)) != 0
        assert "null argument" in lib.dfgpu_last_error().decode()


def test_an_output_the_pool_cannot_admit_is_resources_exhausted():
    from datafusion_amd import _lib, ops
    from datafusion_amd.table import DeviceTable
    c = RC.by_name("nulls_lower_only_b_all_null")
    pairs = RC.pairs(c.name)
    assert len(pairs) > 2000
    dl, dr = DeviceTable.from_arrow(c.left), DeviceTable.from_arrow(c.right)
    run_rj(dl, dr, c.x, c.lower, c.upper, "RightSemi")            # (the key column's statistics are cached on the table from here on)
    ops.sync()
    before = ops.mem_stats()["in_use"]
    ops.mem_set_limit(before + 4096)            # the row ids of 2000 pairs alone are 32 000 bytes
    try:
        for jt in ("Inner", "Full"):
            with pytest.raises(_lib.DfgpuError, match="Resources exhausted"):
                run_rj(dl, dr, c.x, c.lower, c.upper, jt)
            ops.sync()
            assert ops.mem_stats()["in_use"] == before
        got, kernels = run_rj(dl, dr, c.x, c.lower, c.upper, "RightSemi")      # the one-sided types write no pair
        assert got.num_rows == len({r for _, r in pairs}) and "rangejoin_expand" not in kernels
    finally:
        ops.mem_set_limit(0)
    got, _ = run_rj(dl, dr, c.x, c.lower, c.upper, "Inner")
    assert got.num_rows == len(pairs)
    for t in (dl, dr):
        t.free()


def test_the_entry_point_from_ctypes_with_null_column_arrays():
    """the Mark types with no output column at all: NULL arrays and zero counts"""
    import ctypes as C

    from datafusion_amd import _lib, ops
    from datafusion_amd.table import DeviceTable
    c = RC.by_name("ties_le_lt")
    pairs = RC.pairs(c.name)
    with uploaded(c.left, c.right) as (dl, dr):
        lib = _lib.load()
        for jt, n, hit in (("LeftMark", c.left.num_rows, {l for l, _ in pairs}), ("RightMark", c.right.num_rows, {r for _, r in pairs})):
            out = C.c_void_p()
            rc = lib.dfgpu_range_join(dl.handle, dr.handle, ops.JOIN_TYPES[jt], 0, 0, 1, 1, 0, None, 0, None, 0, C.byref(out))
            assert rc == 0, lib.dfgpu_last_error().decode()
            t = DeviceTable(out)
            got = t.to_arrow()
            t.free()
            assert got.column_names == ["mark"] and got.column("mark").to_pylist() == [i in hit for i in range(n)]


# ------------------------------------------------------------------------------------------------------------------------- plans
def _collect(plan):
    """-> (rows as an Arrow table, the nlj_* and rangejoin_* profile names that ran)"""
    from datafusion_amd import physical_plan as P
    got, names = _profiled(lambda: P.collect(plan))
    return got, {k for k in names if k.startswith(("nlj_", "rangejoin_"))}


def test_band_joins_through_the_rule():
    from datafusion_amd import physical_plan as P
    from datafusion_amd.expr import col
    c = RC.by_name("band_257x255")
    with uploaded(c.left, c.right) as (dl, dr):
        leaves = lambda: (P.MemoryExec(dl, "l"), P.MemoryExec(dr, "r"))
        # RightSemi at the root: taken, and the rows are the nested-loop plan's, position by position
        semi = lambda: P.NestedLoopJoinExec(*leaves(), c.filter, "RightSemi", ([], ["w", "x"]))
        plain, asked = P.GpuOffloadRule().optimize(semi()), P.GpuOffloadRule(range_joins=True).optimize(semi())
        assert type(plain) is P.NestedLoopJoinExec and type(asked) is P.GpuRangeJoinExec
        assert P.displayable(asked).split("\n")[0] == "GpuRangeJoinExec: join_type=RightSemi, lo@0 <= x@0 AND x@0 < hi@1, projection=([], ['w', 'x'])"
        (want, kw), (got, kg) = _collect(plain), _collect(asked)
        assert want.num_rows and N.difference(got, want) is None
        assert kw == {"nlj_flags"} and kg == {"rangejoin_keys", "rangejoin_bounds", "rangejoin_cover"}
        # Inner under an aggregate: nobody observes the pair order, the join is taken
        agg = lambda: P.AggregateExec("Single", [], [("count", None, "c"), ("sum", col("tag"), "s"), ("sum", col("x"), "sx")],
                                      P.NestedLoopJoinExec(*leaves(), c.filter, "Inner"))
        plain, asked = P.GpuOffloadRule().optimize(agg()), P.GpuOffloadRule(range_joins=True).optimize(agg())
        assert type(plain.children()[0]) is P.NestedLoopJoinExec and type(asked.children()[0]) is P.GpuRangeJoinExec
        (want, kw), (got, kg) = _collect(plain), _collect(asked)
        assert want.column("c").to_pylist() == [len(RC.pairs(c.name))] and N.difference(got, want) is None
        assert kw == {"nlj_count", "nlj_emit"} and kg == {"rangejoin_keys", "rangejoin_bounds", "rangejoin_expand"}
        # Inner at the root: the order is observed, the nested-loop join stays and runs its own kernels — as with the default argument
        root = lambda: P.NestedLoopJoinExec(*leaves(), c.filter, "Inner")
        for rule in (P.GpuOffloadRule(range_joins=True), P.GpuOffloadRule()):
            plan = rule.optimize(root())
            assert type(plan) is P.NestedLoopJoinExec and not rule.declined
            got, k = _collect(plan)
            assert k == {"nlj_count", "nlj_emit"}
            assert N.difference(got, N.nested_loop_join(c.left, c.right, "Inner", passing=N.passing_pairs(c.left, c.right, c.ref_filter))) is None


def test_q11_shape_through_the_rule():
    """grouped sums joined with a one-row aggregate by `value > total * 0.0001` (TPC-H Q11's HAVING).  The Decimal128 filter with its
    product is no range condition and stays a nested-loop join under range_joins=True; the same shape over Int64 sums with the bare
    comparison `value > threshold` is taken.  Both give the nested-loop plan's rows."""
    from decimal import Decimal

    from datafusion_amd import physical_plan as P
    from datafusion_amd.expr import col, lit
    from datafusion_amd.table import DeviceTable
    rng = np.random.default_rng(3)
    k = rng.integers(0, 60, size=4000)
    cents = rng.integers(1, 100000, size=4000)
    cents[k % 7 == 0] = 1                          # the groups the HAVING drops
    t = DeviceTable.from_arrow(pa.table({"k": pa.array(k, type=pa.int64()), "v": pa.array([Decimal(int(x)).scaleb(-2) for x in cents], type=pa.decimal128(15, 2)),
                                         "c": pa.array(cents, type=pa.int64())}))
    th = DeviceTable.from_arrow(pa.table({"threshold": pa.array([int(cents.sum()) // 10000], type=pa.int64())}))
    try:
        frac = lit(Decimal("0.0001"), pa.decimal128(5, 4))
        grouped = lambda v: P.AggregateExec("Single", [(col("k"), "k")], [("sum", col(v), "value")], P.MemoryExec(t, "t"))
        total = lambda: P.AggregateExec("Single", [], [("sum", col("v"), "total")], P.MemoryExec(t, "t"))
        q11 = lambda jt: P.NestedLoopJoinExec(total(), grouped("v"), (col("f1") > col("f0") * frac, [(0, "Left"), (1, "Right")]), jt, ([], ["k", "value"]))
        q11_int = lambda jt: P.NestedLoopJoinExec(P.MemoryExec(th, "th"), grouped("c"), (col("f1") > col("f0"), [(0, "Left"), (1, "Right")]), jt, ([], ["k", "value"]))
        for shape, taken in ((q11, False), (q11_int, True)):
            for jt in ("Inner", "RightSemi"):
                plain, asked = P.GpuOffloadRule().optimize(shape(jt)), P.GpuOffloadRule(range_joins=True).optimize(shape(jt))
                assert type(plain) is P.NestedLoopJoinExec
                assert type(asked) is (P.GpuRangeJoinExec if taken and jt == "RightSemi" else P.NestedLoopJoinExec)    # (Inner at the root: order is observed)
                (want, kw), (got, kg) = _collect(plain), _collect(asked)
                assert 0 < want.num_rows < 60 and got.column_names == ["k", "value"] and N.difference(got, want) is None
                assert all(n.startswith("nlj_") for n in kw) and kw
                assert all(n.startswith("rangejoin_" if type(asked) is P.GpuRangeJoinExec else "nlj_") for n in kg) and kg
            # below an aggregate the Inner join of the Int64 shape is taken too
            cnt = lambda: P.AggregateExec("Single", [], [("count", None, "n"), ("sum", col("value"), "s")], shape("Inner"))
            plain, asked = P.GpuOffloadRule().optimize(cnt()), P.GpuOffloadRule(range_joins=True).optimize(cnt())
            assert type(asked.children()[0]) is (P.GpuRangeJoinExec if taken else P.NestedLoopJoinExec)
            assert N.difference(_collect(asked)[0], _collect(plain)[0]) is None
    finally:
        t.free()
        th.free()
