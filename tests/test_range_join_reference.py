"""tests/range_join_ref.py held to hand-worked answers and to the pair-space reference (tests/nlj_ref.py with the equivalent JoinFilter),
the cases of tests/range_join_cases.py held to what they are named for, and the usual wrong range joins shown to differ from the
reference on those tables — so that a device operator that passes tests/test_zzzz_gpu_range_join.py cannot be one of them.  No GPU."""
import pyarrow as pa
import pytest

from tests import expr_ref
from tests import nlj_ref as N
from tests import range_join_cases as RC
from tests import range_join_ref as R

T = RC.T
SMALL = RC.small_cases()
ALL = RC.all_cases()

# ---- six rows by hand: intervals [1, 3], [3, 3], [NULL, 9] against the points 3, 1, NULL
L = pa.table({"lo": pa.array([1, 3, None], type=pa.int64()), "hi": pa.array([3, 3, 9], type=pa.int64())})
P = pa.table({"x": pa.array([3, 1, None], type=pa.int64())})
HAND = {
    "le_lt": [(0, 1)],                                        # [1, 3) holds 1; [3, 3) is empty; a NULL lower bound matches nothing
    "le_le": [(0, 1), (0, 0), (1, 0)],                        # [1, 3] holds 1 then 3 (ascending x, not ascending row); [3, 3] holds 3
    "lt_lt": [],                                              # (1, 3) holds neither
    "lt_le": [(0, 0)],                                        # (1, 3] holds 3; (3, 3] is empty
    "le_only": [(0, 1), (0, 0), (1, 0)],                      # 1 <= x: both points; 3 <= x: 3; NULL <= x: nothing
    "lt_only": [(0, 0)],
    "only_le": [(0, 1), (0, 0), (1, 1), (1, 0), (2, 1), (2, 0)],   # the NULL of the absent lower bound's column does not matter
    "only_lt": [(0, 1), (1, 1), (2, 1), (2, 0)],
}


def _bounds(cond):
    li, ui = RC.CONDITIONS[cond]
    return (None if li is None else ("lo", li)), (None if ui is None else ("hi", ui))


@pytest.mark.parametrize("cond", list(RC.CONDITIONS))
def test_six_rows_by_hand(cond):
    lower, upper = _bounds(cond)
    assert R.matching_pairs(L, P, "x", lower, upper) == HAND[cond]
    full = R.range_join(L, P, "x", lower, upper, "Full")
    rows = [tuple(c[i].as_py() for c in full.columns) for i in range(full.num_rows)]
    val = lambda t, c, i: None if i is None else t.column(c)[i].as_py()
    hit_l, hit_r = {l for l, _ in HAND[cond]}, {r for _, r in HAND[cond]}
    want = [(l, r) for l, r in HAND[cond]] + [(None, r) for r in range(3) if r not in hit_r] + [(l, None) for l in range(3) if l not in hit_l]
    assert rows == [(val(L, "lo", l), val(L, "hi", l), val(P, "x", r)) for l, r in want]
    mark = R.range_join(L, P, "x", lower, upper, "RightMark")
    assert mark.column("mark").to_pylist() == [r in hit_r for r in range(3)] and mark.column("x").to_pylist() == [3, 1, None]
    anti = R.range_join(L, P, "x", lower, upper, "LeftAnti")
    assert anti.column("hi").to_pylist() == [[3, 3, 9][l] for l in range(3) if l not in hit_l]


def test_no_bound_is_refused():
    with pytest.raises(AssertionError, match="needs a lower or an upper bound"):
        R.matching_pairs(L, P, "x")


@pytest.mark.parametrize("case", SMALL, ids=[c.name for c in SMALL])
def test_the_reference_is_the_nested_loop_join_with_the_equivalent_filter(case):
    assert case.left.num_rows * case.right.num_rows <= 328 * 257
    passing = N.passing_pairs(case.left, case.right, case.ref_filter)
    pairs = list(RC.pairs(case.name))
    for jt in N.ALL_TYPES:
        got = R.range_join(case.left, case.right, case.x, case.lower, case.upper, jt, pairs=pairs)
        want = N.nested_loop_join(case.left, case.right, jt, passing=passing)
        assert got.column_names == want.column_names
        if jt in N.PAIR_TYPES:
            assert N.multiset(got) == N.multiset(want), jt
        else:
            assert N.difference(got, want) is None, (jt, N.difference(got, want))


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_every_case_has_the_rows_it_is_named_for(case):
    nl, nr = case.left.num_rows, case.right.num_rows
    pairs = RC.pairs(case.name)
    lh, rh = {l for l, _ in pairs}, {r for _, r in pairs}
    if case.kind == "empty":
        assert nl == 0 or nr == 0
    elif case.kind == "all_match":
        assert len(pairs) == nl * nr > 0
    elif case.kind == "no_match":
        assert not pairs and nl and nr
    else:
        assert case.kind == "mixed"
        for hit, n in ((lh, nl), (rh, nr)):
            assert len(hit) >= 1
            assert n == 1 or len(hit) < n, "a side of two rows or more has an unmatched row"
    # the order contract on the pairs themselves: ascending left row, then ascending x, then ascending right row
    xs = R.key_values(case.right.column(case.x))
    assert list(pairs) == sorted(pairs, key=lambda p: (p[0], xs[p[1]], p[1]))


def test_the_skew_cases_sit_on_the_tile_edges_they_are_named_for():
    counts = lambda name: [sum(1 for l, _ in RC.pairs(name) if l == g) for g in range(RC.by_name(name).left.num_rows)]
    assert counts(f"skew_1x{2 * T + 3}_all_match") == [2 * T + 3]
    c = counts(f"skew_{T + 1}_rows_one_match_each")
    assert c == [1] * (T + 1) + [0]
    c = counts("skew_300_rows_without_a_match_between_heavy_rows")
    assert c == [1500] + [0] * 300 + [1500] and 1500 < T < 3000           # the second tile starts inside the last row's run
    c = counts(f"skew_{T + 5}_rows_without_a_match_in_one_tile")
    assert c == [10] + [0] * (T + 5) + [10, 0, 3] and sum(c) < T and len(c) > T   # one tile whose rows outnumber its slots
    c = counts("skew_one_row_over_three_tiles")
    assert c == [T // 2, 0, 1, 2 * T + 100, 0, 1]
    first, last = T // 2 + 1, T // 2 + 1 + 2 * T + 100 - 1                  # the big row's first and last output slot
    assert first // T == 0 and last // T == 2
    for total in (T - 1, T, T + 1):
        assert sum(counts(f"skew_total_{total}")) == total
    runs = {}
    for v in RC.by_name("ties_le_le").right.column("x").to_pylist():
        runs[v] = runs.get(v, 0) + 1
    assert [runs[v] for v in (10, 20, 30, 40, 50)] == [1, 63, 64, 65, 130]


def test_the_type_cases_hold_the_edges_they_are_named_for():
    import struct
    bits = lambda t, c: [None if v is None else struct.unpack("<Q", struct.pack("<d", v))[0] for v in t.column(c).to_pylist()]
    f = RC.by_name("type_float64_le_lt")
    for col, t in (("lo", f.left), ("x", f.right)):
        b = set(bits(t, col))
        assert {0x0, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000, 0xFFF8000000000000, 0x1, 0x8000000000000001} <= b
    i = RC.by_name("type_int64_le_lt")
    for col, t in (("lo", i.left), ("hi", i.left), ("x", i.right)):
        v = t.column(col).to_pylist()
        assert -2**63 in v and 2**63 - 1 in v
    u = RC.by_name("type_uint64_le_lt")
    assert 2**63 in u.right.column("x").to_pylist() and 2**64 - 1 in u.left.column("hi").to_pylist()
    for name, typ in RC.KEY_TYPES.items():
        c = RC.by_name(f"type_{name}_le_lt")
        assert c.left.schema.field("lo").type == c.left.schema.field("hi").type == c.right.schema.field("x").type == typ
        assert c.left.column("lo").null_count and c.left.column("hi").null_count and c.right.column("x").null_count


# ------------------------------------------------------------------------------------------------------------------- wrong joins
def _raw(col):
    """a key column as its stored integers (Float64: the bit pattern as an unsigned integer), None = NULL"""
    import numpy as np
    col = N._flat(col)
    if pa.types.is_float64(col.type):
        bits = np.frombuffer(col.buffers()[1], dtype=np.uint64)[col.offset:col.offset + len(col)]
        return [int(b) if ok else None for b, ok in zip(bits, col.is_valid().to_pylist())]
    return (col.cast(pa.int32()) if pa.types.is_date32(col.type) else col).to_pylist()


def wrong_join(case, what, join_type):
    """the range join with one mistake, over the pair space"""
    import struct
    typ = case.right.schema.field(case.x).type
    is_f = pa.types.is_float64(typ)
    if what == "ieee" and is_f:
        key = lambda v: struct.unpack("<d", struct.pack("<Q", v))[0]         # NaN compares false with everything, -0.0 == +0.0
    elif what == "unsigned" and not is_f:
        key = lambda v: v % 2**64
    elif is_f:
        key = expr_ref.total_key
    else:
        key = lambda v: v
    conv = lambda vals: [None if v is None else key(v) for v in vals]
    xs = conv(_raw(case.right.column(case.x)))
    a = None if case.lower is None else conv(_raw(case.left.column(case.lower[0])))
    b = None if case.upper is None else conv(_raw(case.left.column(case.upper[0])))
    li = case.lower[1] if case.lower else None
    ui = case.upper[1] if case.upper else None
    if what == "lt_as_le":
        li, ui = (True if li is not None else None), (True if ui is not None else None)
    if what == "le_as_lt":
        li, ui = (False if li is not None else None), (False if ui is not None else None)

    def holds(l, r, li=li, ui=ui):
        if xs[r] is None:
            return what == "null_x_matches"
        for bound, inc, lower in ((a, li, True), (b, ui, False)):
            if bound is None:
                continue
            if bound[l] is None:
                if what == "null_bound_unbounded":
                    continue
                return False
            lhs, rhs = (bound[l], xs[r]) if lower else (xs[r], bound[l])
            if not (lhs <= rhs if inc else lhs < rhs):
                return False
        return True

    nl, nr = case.left.num_rows, case.right.num_rows
    pairs = [(l, r) for l in range(nl) for r in range(nr) if holds(l, r)]
    order_key = lambda p: (p[0], (xs[p[1]] is None, xs[p[1]] if xs[p[1]] is not None and xs[p[1]] == xs[p[1]] else 0), p[1])
    if what == "ties_descending":
        order_key = lambda p: (p[0], xs[p[1]], -p[1])
    if what == "right_row_major":
        order_key = lambda p: (p[1], p[0])
    pairs.sort(key=order_key)
    lrows, rrows, marks = N.index_rows(nl, nr, pairs, join_type)
    if what == "no_unmatched_right_tail" and join_type in ("Right", "Full"):
        keep = [i for i in range(len(lrows)) if lrows[i] is not None or rrows[i] is None]
        lrows, rrows = [lrows[i] for i in keep], [rrows[i] for i in keep]
    if what == "touching_counts_as_hit" and join_type in N.RIGHT_ONE_SIDED + ("Right", "Full"):
        # the right-side flags taken from closed intervals whatever the condition says: an empty interval that touches a point hits it
        touched = {r for l in range(nl) for r in range(nr) if holds(l, r, True if li is not None else None, True if ui is not None else None)}
        closed = sorted(touched | {r for _, r in pairs})
        fake = [(0, r) for r in closed]
        if join_type in N.RIGHT_ONE_SIDED:
            lrows, rrows, marks = N.index_rows(nl, nr, fake, join_type)
        else:
            tail = [i for i in range(len(lrows)) if lrows[i] is None and rrows[i] in touched]
            lrows, rrows = [v for i, v in enumerate(lrows) if i not in tail], [v for i, v in enumerate(rrows) if i not in tail]
    return N.materialise(case.left, case.right, lrows, rrows, marks, join_type)


WRONG = [
    ("lt_as_le", ("Inner", "LeftSemi", "RightMark"), ("ties_lt_lt", "ties_le_lt", "band_lt_lt_64x64")),
    ("le_as_lt", ("Inner", "LeftAnti", "RightSemi"), ("ties_le_le",)),      # (the run at 500 is hit by [500, 500] alone)
    ("le_as_lt", ("Inner", "LeftAnti"), ("ties_lt_le",)),
    ("null_bound_unbounded", ("Inner", "Left", "LeftMark", "RightSemi"), ("nulls_le_lt", "nulls_a_all_null", "nulls_b_all_null")),
    ("null_x_matches", ("Inner", "Right", "RightAnti", "LeftSemi"), ("nulls_le_lt", "nulls_x_all_null")),
    ("ieee", ("Inner", "LeftSemi", "RightSemi"), ("type_float64_le_lt", "type_float64_lt_le")),
    ("ties_descending", ("Inner", "Full"), ("ties_le_le", "ties_le_lt")),
    ("right_row_major", ("Inner", "Left"), ("band_65x63", "ties_le_le")),
    ("unsigned", ("Inner", "LeftSemi"), ("type_int64_le_lt", "type_int32_le_lt", "type_date32_lt_le")),
    ("no_unmatched_right_tail", ("Right", "Full"), ("band_65x63", "nulls_le_lt")),
    ("touching_counts_as_hit", ("RightSemi", "RightAnti", "RightMark", "Right", "Full"), ("ties_le_lt", "ties_lt_lt", "ties_lt_le")),
]


@pytest.mark.parametrize("what, types, names", WRONG, ids=[f"{w[0]}-{w[2][0]}" for w in WRONG])
def test_wrong_joins_differ_from_the_reference_on_the_gpu_tests_tables(what, types, names):
    for name in names:
        c = RC.by_name(name)
        pairs = list(RC.pairs(name))
        for jt in types:
            want = R.range_join(c.left, c.right, c.x, c.lower, c.upper, jt, pairs=pairs)
            assert N.difference(wrong_join(c, what, jt), want) is not None, (what, name, jt)


def test_the_wrong_join_machinery_without_a_mistake_is_the_reference():
    """`wrong_join` with no mistake switched on gives the reference's tables: the differences above come from the mistakes alone"""
    for name in ("ties_le_lt", "nulls_le_lt", "type_float64_le_lt", "type_int64_lt_le", "band_65x63"):
        c = RC.by_name(name)
        for jt in N.ALL_TYPES:
            want = R.range_join(c.left, c.right, c.x, c.lower, c.upper, jt, pairs=list(RC.pairs(name)))
            assert N.difference(wrong_join(c, "nothing", jt), want) is None, (name, jt)
