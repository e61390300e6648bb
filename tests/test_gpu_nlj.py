"""dfgpu_nested_loop_join (NestedLoopJoinExec / CrossJoinExec on the device) against tests/nlj_ref.py, position by position — the output
order is part of the contract — with Float64 compared by bits.  The cases are tests/nlj_cases.py's; tests/test_nlj_reference.py holds
the reference to hand-worked answers and the oracle, checks that every case has the matched and unmatched rows it is named for, and
shows that the usual wrong joins differ from the reference on these tables.  Every case asserts which of the operator's kernels ran.
A test takes one case through all ten join types: the case's tables are uploaded once and its passing pairs are computed once per
process (tests.nlj_cases.passing)."""
from decimal import Decimal

import numpy as np
import pyarrow as pa
import pytest

from tests import nlj_cases as NC
from tests import nlj_ref as R

pytestmark = pytest.mark.gpu

CASES = NC.all_cases()
_passing = NC.passing


def run_nlj(left, right, join_type, flt, options=None, left_cols=None, right_cols=None):
    """-> (the output as an Arrow table, the set of nlj_* profile names that ran); Arrow inputs are uploaded and freed here"""
    from datafusion_amd import ops
    from datafusion_amd.table import DeviceTable
    dl, dr = (t if isinstance(t, DeviceTable) else DeviceTable.from_arrow(t) for t in (left, right))
    if options:
        ops.set_options(**options)
    ops.profile_enable(True)
    ops.profile_reset()
    try:
        out = ops.nested_loop_join(dl, dr, join_type, flt, left_cols, right_cols)
        stats = ops.profile_stats()
    finally:
        ops.profile_enable(False)
        if options:
            ops.set_options(**{k: None for k in options})
    got = out.to_arrow()
    out.free()
    for t, src in ((dl, left), (dr, right)):
        if t is not src:
            t.free()
    return got, {k for k in stats if k.startswith("nlj_")}


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


def expected_kernels(path, join_type, nl, nr):
    """what the operator launches: nothing for an empty right side (row programs) or an empty pair space (materialising path)"""
    if path == "cartesian":
        return {"nlj_cartesian"} if nl and nr else set()
    if not nr:
        return set()
    return {"nlj_count", "nlj_emit"} if join_type in R.PAIR_TYPES else {"nlj_flags"}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_every_join_type_against_the_reference(case):
    passing = list(_passing(case.name))
    with uploaded(case.left, case.right) as (dl, dr):
        for join_type in R.ALL_TYPES:
            want = R.nested_loop_join(case.left, case.right, join_type, passing=passing)
            got, kernels = run_nlj(dl, dr, join_type, case.filter, case.options)
            assert R.difference(got, want) is None, (join_type, R.difference(got, want))
            exp = expected_kernels(case.path, join_type, case.left.num_rows, case.right.num_rows)
            if "nlj_emit" in exp and not passing:
                exp = exp - {"nlj_emit"}          # nothing counted: nothing to emit
            assert kernels == exp, (join_type, kernels, exp)


@pytest.mark.parametrize("name", ["band_257x255", "band_wide_65x63", "nulls_65x257", "float_lt_65x257", "decimal_65x257"])
def test_the_two_evaluations_agree_bit_for_bit(name):
    """the same filter through the row program and, under nlj.rowprog=0, through the materialising path in pieces"""
    c = NC.by_name(name)
    with uploaded(c.left, c.right) as (dl, dr):
        for join_type in R.ALL_TYPES:
            a, ka = run_nlj(dl, dr, join_type, c.filter)
            b, kb = run_nlj(dl, dr, join_type, c.filter, {"nlj__rowprog": 0, "nlj__chunk_pairs": 1000})
            assert R.difference(a, b) is None, (join_type, R.difference(a, b))
            assert "nlj_cartesian" not in ka and kb == {"nlj_cartesian"}


def test_early_exit_changes_nothing():
    c = NC.by_name("band_515x63_ragged_chunks")
    with uploaded(c.left, c.right) as (dl, dr):
        for join_type in R.ALL_TYPES:
            a, _ = run_nlj(dl, dr, join_type, c.filter, c.options)
            b, _ = run_nlj(dl, dr, join_type, c.filter, dict(c.options, nlj__early_exit=0))
            assert R.difference(a, b) is None, join_type


@pytest.mark.parametrize("name", ["band_257x255", "nulls_65x257", "decimal_65x257"])
def test_the_constant_key_hash_join_is_the_same_join(name):
    """a second device path: ops.hash_join on an added constant key column with the same JoinFilter, as multisets"""
    from datafusion_amd import ops
    c = NC.by_name(name)
    key = lambda t: t.append_column("__k", pa.array([1] * t.num_rows, type=pa.int32()))
    with uploaded(key(c.left), key(c.right)) as (dl, dr):
        lc, rc = list(range(c.left.num_columns)), list(range(c.right.num_columns))
        for join_type in R.ALL_TYPES:
            out = ops.hash_join(dl, dr, [("__k", "__k")], join_type, join_filter=c.filter, build_cols=lc, probe_cols=rc)
            hj = out.to_arrow()
            out.free()
            got, _ = run_nlj(dl, dr, join_type, c.filter, left_cols=lc, right_cols=rc)
            assert got.column_names == hj.column_names and R.multiset(got) == R.multiset(hj), join_type


def test_projections_subsets_reordered_and_empty():
    c = NC.by_name("band_65x63")
    passing = list(_passing(c.name))
    with uploaded(c.left, c.right) as (dl, dr):
        for join_type in R.ALL_TYPES:
            for lc, rc in ((["tag", "lo"], ["w"]), ([], ["x", "w"]), (["hi"], []), ([], []), ([2, 0, 1], [1, 0])):
                want = R.nested_loop_join(c.left, c.right, join_type, left_cols=lc, right_cols=rc, passing=passing)
                got, _ = run_nlj(dl, dr, join_type, c.filter, left_cols=lc, right_cols=rc)
                if want.num_columns == 0:     # (an Arrow table without columns cannot say how many rows the reference has: the row ids can)
                    li, ri, _ = R.index_rows(c.left.num_rows, c.right.num_rows, passing, join_type)
                    assert got.num_columns == 0 and got.num_rows == len(li if li is not None else ri)
                    continue
                assert R.difference(got, want) is None, (join_type, lc, rc, R.difference(got, want))


def _band_ref():
    from tests.util import to_oracle_expr
    flt = NC.band_filter()
    return flt, (to_oracle_expr(flt[0]), flt[1])


def test_dictionary_and_utf8_payload_columns():
    left, right = NC.payload_tables(65, 63)
    flt, ref = _band_ref()
    passing = R.passing_pairs(left, right, ref)
    with uploaded(left, right) as (dl, dr):
        for join_type in R.ALL_TYPES:
            got, kernels = run_nlj(dl, dr, join_type, flt)
            want = R.nested_loop_join(left, right, join_type, passing=passing)
            assert R.difference(got, want) is None, (join_type, R.difference(got, want))
            assert "nlj_cartesian" not in kernels


def test_sliced_inputs_and_columns_at_an_offset():
    from datafusion_amd import ops
    flt, ref = _band_ref()
    left, right = NC.band_tables(300, 280)
    with uploaded(left, right) as (dl, dr):
        # a slice of each side
        sl, sr = dl.slice(37, 257), dr.slice(19, 255)
        al, ar = left.slice(37, 257), right.slice(19, 255)
        passing = R.passing_pairs(al, ar, ref)
        for join_type in R.ALL_TYPES:
            got, _ = run_nlj(sl, sr, join_type, flt)
            assert R.difference(got, R.nested_loop_join(al, ar, join_type, passing=passing)) is None, join_type
        # partitions of a table without NULLs are views into one buffer per column: every part but the first starts at an offset
        lparts, rparts = ops.partition(dl, ["lo"], 3), ops.partition(dr, ["x"], 2)
        assert any(p.column_view(0).data != lparts[0].column_view(0).data for p in lparts[1:])
        pl, pr = lparts[1], rparts[1]
        al, ar = pl.to_arrow(), pr.to_arrow()
        assert al.num_rows and ar.num_rows
        passing = R.passing_pairs(al, ar, ref)
        for join_type in R.ALL_TYPES:
            got, _ = run_nlj(pl, pr, join_type, flt)
            assert R.difference(got, R.nested_loop_join(al, ar, join_type, passing=passing)) is None, join_type
        for t in [sl, sr] + lparts + rparts:
            t.free()


def test_refusals_by_their_messages():
    import ctypes as C

    from datafusion_amd import _lib, ops
    from datafusion_amd.expr import col
    from datafusion_amd.table import DeviceTable
    left, right = NC.null_tables(5, 4)
    dl, dr = DeviceTable.from_arrow(left), DeviceTable.from_arrow(right)
    lr = [(0, "Left"), (0, "Right")]
    for jt in ("Inner", "LeftSemi", "RightMark"):
        with pytest.raises(_lib.DfgpuError, match="join filter expression must be Boolean"):
            ops.nested_loop_join(dl, dr, jt, (col("f0") + col("f1"), lr))
        with pytest.raises(_lib.DfgpuError, match="join filter column index out of range"):
            ops.nested_loop_join(dl, dr, jt, (col("f0") < col("f1"), [(0, "Left"), (2, "Right")]))
        with pytest.raises(_lib.DfgpuError, match="join filter column index out of range"):
            ops.nested_loop_join(dl, dr, jt, (col("f0") < col("f1"), [(-1, "Left"), (0, "Right")]))
    lib, out = _lib.load(), C.c_void_p()
    ints = lambda *v: (C.c_int * len(v))(*v)
    assert lib.dfgpu_nested_loop_join(dl.handle, dr.handle, 0, None, ints(0, 2), 2, ints(0), 1, C.byref(out)) != 0
    assert "left output column out of range" in lib.dfgpu_last_error().decode()
    assert lib.dfgpu_nested_loop_join(dl.handle, dr.handle, 2, None, ints(0), 1, ints(-1), 1, C.byref(out)) != 0
    assert "right output column out of range" in lib.dfgpu_last_error().decode()
    assert lib.dfgpu_nested_loop_join(dl.handle, dr.handle, 10, None, ints(0), 1, ints(0), 1, C.byref(out)) != 0
    assert "bad join type" in lib.dfgpu_last_error().decode()
    assert lib.dfgpu_nested_loop_join(dl.handle, None, 0, None, ints(0), 1, ints(0), 1, C.byref(out)) != 0
    for t in (dl, dr):
        t.free()


@pytest.mark.parametrize("options", [{}, {"nlj__rowprog": 0}], ids=["rowprog", "materialised"])
def test_an_output_the_pool_cannot_admit_is_resources_exhausted(options):
    from datafusion_amd import _lib, ops
    from datafusion_amd.table import DeviceTable
    c = NC.by_name("nulls_65x257")
    assert len(_passing(c.name)) > 2000
    dl, dr = DeviceTable.from_arrow(c.left), DeviceTable.from_arrow(c.right)
    ops.sync()
    before = ops.mem_stats()["in_use"]
    ops.mem_set_limit(before + 4096)            # the row ids of 2997 pairs alone are 47 952 bytes
    try:
        for jt in ("Inner", "Full"):
            with pytest.raises(_lib.DfgpuError, match="Resources exhausted"):
                run_nlj(dl, dr, jt, c.filter, options)
            ops.sync()
            assert ops.mem_stats()["in_use"] == before
        if not options:
            with pytest.raises(_lib.DfgpuError, match="Resources exhausted"):      # a cross join's size is known before anything runs
                run_nlj(dl, dr, "Inner", None)
            assert ops.mem_stats()["in_use"] == before
        got, _ = run_nlj(dl, dr, "RightSemi", c.filter, options)                     # the one-sided types write no pair
        assert got.num_rows == len({r for _, r in _passing(c.name)})
    finally:
        ops.mem_set_limit(0)
    got, _ = run_nlj(dl, dr, "Inner", c.filter, options)
    assert got.num_rows == len(_passing(c.name))
    for t in (dl, dr):
        t.free()


# ------------------------------------------------------------------------------------------------------------------------- plans
def test_q11_shape_through_the_rule():
    """grouped sums joined with a one-row aggregate by `value > total * 0.0001` (TPC-H Q11's HAVING): the NestedLoopJoinExec plan and
    the same plan built from ScalarSubqueryExec give the same rows"""
    from datafusion_amd import physical_plan as P
    from datafusion_amd.expr import ScalarSubqueryExpr, ScalarSubqueryResults, col, lit
    from datafusion_amd.table import DeviceTable
    rng = np.random.default_rng(3)
    k = rng.integers(0, 60, size=4000)
    v = [Decimal(int(x)).scaleb(-2) for x in rng.integers(1, 100000, size=4000)]
    for i in range(4000):
        if k[i] % 7 == 0:
            v[i] = Decimal("0.01")              # the groups the HAVING drops
    t = DeviceTable.from_arrow(pa.table({"k": pa.array(k, type=pa.int64()), "v": pa.array(v, type=pa.decimal128(15, 2))}))
    grouped = lambda: P.AggregateExec("Single", [(col("k"), "k")], [("sum", col("v"), "value")], P.MemoryExec(t, "t"))
    total = lambda: P.AggregateExec("Single", [], [("sum", col("v"), "total")], P.MemoryExec(t, "t"))
    frac = lit(Decimal("0.0001"), pa.decimal128(5, 4))
    nlj = P.NestedLoopJoinExec(total(), grouped(), (col("f1") > col("f0") * frac, [(0, "Left"), (1, "Right")]), "Inner", ([], ["k", "value"]))
    rule = P.GpuOffloadRule()
    plan = rule.optimize(nlj)
    assert type(plan) is P.NestedLoopJoinExec and not rule.declined
    out = P.collect(plan)
    got = out.to_arrow()
    out.free()
    res = ScalarSubqueryResults(1)
    sub = P.ScalarSubqueryExec(P.FilterExec(col("value") > ScalarSubqueryExpr(res, 0, pa.decimal128(25, 2)) * frac, grouped()), [(total(), 0)], res)
    out = P.collect(P.GpuOffloadRule().optimize(sub))
    want = out.to_arrow()
    out.free()
    t.free()
    assert got.column_names == ["k", "value"] and R.multiset(got) == R.multiset(want)
    sums = {}
    for key, val in zip(k.tolist(), v):
        sums[key] = sums.get(key, Decimal(0)) + val
    keep = sorted(key for key, s in sums.items() if s > sum(sums.values()) * Decimal("0.0001"))
    assert sorted(got.column("k").to_pylist()) == keep and 0 < len(keep) < len(sums)


def test_cross_join_under_a_filter_through_the_rule():
    from datafusion_amd import physical_plan as P
    from datafusion_amd.expr import col
    from datafusion_amd.table import DeviceTable
    left, right = NC.null_tables(65, 64)
    dl, dr = DeviceTable.from_arrow(left), DeviceTable.from_arrow(right)
    plan = P.FilterExec(col("a") < col("x"), P.CoalesceBatchesExec(P.CrossJoinExec(P.MemoryExec(dl, "l"), P.MemoryExec(dr, "r"))))
    rule = P.GpuOffloadRule()
    opt = rule.optimize(plan)
    assert type(opt.input) is P.CrossJoinExec and not rule.declined
    out = P.collect(opt)
    got = out.to_arrow()
    out.free()
    want = R.nested_loop_join(left, right, "Inner", (("bin", "<", ("col", "f0"), ("col", "f1")), [(0, "Left"), (0, "Right")]))
    assert R.difference(got, want) is None, R.difference(got, want)
    # a cross join the pool cannot hold stays the reference's operator, with the pool's reason
    from datafusion_amd import ops
    ops.mem_set_limit(ops.mem_stats()["in_use"] + 4096)
    try:
        tight = P.GpuOffloadRule()
        kept = tight.optimize(P.CrossJoinExec(P.MemoryExec(dl, "l"), P.MemoryExec(dr, "r")))
        assert getattr(kept, "kept_on_cpu", False) and len(tight.declined) == 1 and "Resources exhausted" in tight.declined[0][1]
        semi = P.GpuOffloadRule()
        assert not getattr(semi.optimize(P.NestedLoopJoinExec(P.MemoryExec(dl, "l"), P.MemoryExec(dr, "r"), None, "RightSemi")), "kept_on_cpu", False)
    finally:
        ops.mem_set_limit(0)
    for t in (dl, dr):
        t.free()
