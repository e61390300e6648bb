"""The range join's boundary without a GPU: ABI 20 (dfgpu_range_join in the header, the library and the ctypes binding), the plan node's
display and schemas, and what GpuOffloadRule does with and without range_joins=True."""
import os
import re
import subprocess
import sys

import pyarrow as pa
import pytest

from datafusion_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "dfgpu.h")).read()
ALL_TYPES = ["Inner", "Left", "Right", "Full", "LeftSemi", "RightSemi", "LeftAnti", "RightAnti", "LeftMark", "RightMark"]
PAIR_TYPES = ALL_TYPES[:4]


class StubTable:
    """a leaf table for planning only: a row count and a schema"""

    def __init__(self, n, schema=None):
        self.num_rows, self.schema = n, schema

    def index_of(self, c):
        return c if isinstance(c, int) else self.schema.get_field_index(c)


LS = pa.schema([pa.field("lo", pa.int64(), nullable=False), pa.field("hi", pa.int64(), nullable=False), pa.field("name", pa.string()),
                pa.field("lo32", pa.int32()), pa.field("price", pa.decimal128(15, 2)), pa.field("flag", pa.uint8())])
RS = pa.schema([pa.field("x", pa.int64(), nullable=False), pa.field("w", pa.float64(), nullable=False), pa.field("y", pa.int64()),
                pa.field("code", pa.dictionary(pa.int32(), pa.string())), pa.field("s", pa.string()), pa.field("ok", pa.bool_())])


def _leaves(P):
    return P.MemoryExec(StubTable(10, LS), "l"), P.MemoryExec(StubTable(100, RS), "r")


def _band():
    from datafusion_amd.expr import col
    return (col("f0") <= col("f2")).and_(col("f2") < col("f1")), [(0, "Left"), (1, "Left"), (0, "Right")]


def test_the_header_declares_and_the_library_exports_dfgpu_range_join_at_abi_20():
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    decl = re.search(r"int dfgpu_range_join\((.*?)\);", body, flags=re.S)
    assert decl is not None
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["dfgpu_table_t left", "dfgpu_table_t right", "int join_type", "int right_key_col", "int lower_col", "int lower_inclusive",
                    "int upper_col", "int upper_inclusive", "const int* left_out_cols", "int n_left_out", "const int* right_out_cols",
                    "int n_right_out", "dfgpu_table_t* out"]
    assert body.index("int dfgpu_range_join(") > body.index("int dfgpu_nested_loop_join(")
    lib = _lib.load()
    assert hasattr(lib, "dfgpu_range_join") and "dfgpu_range_join" in _lib.SYMBOLS
    assert len(lib.dfgpu_range_join.argtypes) == len(args)
    assert int(re.search(r"#define DFGPU_ABI_VERSION (\d+)", HEADER).group(1)) >= 20 and lib.dfgpu_abi_version() >= 20
    # the semantics and the order contract are part of the declaration's comment
    comment = HEADER[:HEADER.index("int dfgpu_range_join(")].rsplit("/*", 1)[1]
    comment = " ".join(comment.replace("\n *", "\n").split())       # (the comment's line breaks fall inside some of these phrases)
    for words in ("LEFT-row-major", "equal x by ascending right row", "unmatched right rows", "unmatched left rows", "Kleene AND", "-NaN < -inf",
                  "a range join needs a lower or an upper bound", "Resources exhausted", "2^31"):
        assert words in comment, words


def test_the_tile_constant_is_the_headers():
    from datafusion_amd import ops
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert int(re.search(r"#define DFGPU_RANGE_JOIN_TILE (\d+)", body).group(1)) == ops.RANGE_JOIN_TILE
    kernel = open(os.path.join(ROOT, "datafusion_amd", "csrc", "nlj.hip")).read()
    assert "RJ_TILE = DFGPU_RANGE_JOIN_TILE" in kernel            # the expand kernel's tile is the header's


def test_the_call_before_dfgpu_init_fails_with_the_init_message():
    """in a process of its own: this one may have initialised a device already"""
    code = ("import ctypes as C\nfrom datafusion_amd import _lib\nlib = _lib.load()\nout = C.c_void_p()\n"
            "rc = lib.dfgpu_range_join(None, None, 0, 0, 0, 1, -1, 0, None, 0, None, 0, C.byref(out))\nprint(rc, lib.dfgpu_last_error().decode())\n")
    got = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert got.returncode == 0, got.stderr
    assert got.stdout.startswith("1 ") and "dfgpu_init() has not been called" in got.stdout


def test_displayable_prints_the_condition_and_is_a_fixed_point_under_with_new_children():
    from datafusion_amd import physical_plan as P
    l, r = _leaves(P)
    n = P.GpuRangeJoinExec(l, r, "x", ("lo", True), ("hi", False), "Inner")
    lines = P.displayable(n).split("\n")
    assert lines[0] == "GpuRangeJoinExec: join_type=Inner, lo@0 <= x@0 AND x@0 < hi@1"
    assert lines[1].startswith("  MemoryExec: l") and lines[2].startswith("  MemoryExec: r")
    again = n.with_new_children(n.children())
    assert type(again) is P.GpuRangeJoinExec and again is not n and P.displayable(again) == P.displayable(n) and again.children() == [l, r]
    assert not isinstance(n, P.NestedLoopJoinExec)
    by_index = P.GpuRangeJoinExec(l, r, 2, None, (1, True), "RightSemi", ([], ["y"]))
    assert P.displayable(by_index).split("\n")[0] == "GpuRangeJoinExec: join_type=RightSemi, y@2 <= hi@1, projection=([], ['y'])"
    assert P.displayable(P.GpuRangeJoinExec(l, r, "x", ("lo", False), None, "Left")).split("\n")[0] == "GpuRangeJoinExec: join_type=Left, lo@0 < x@0"
    with pytest.raises(ValueError, match="unknown join type"):
        P.GpuRangeJoinExec(l, r, "x", ("lo", True), None, "Outer")


@pytest.mark.parametrize("join_type", ALL_TYPES)
def test_plan_schema_is_the_nested_loop_joins(join_type):
    from datafusion_amd import physical_plan as P
    l, r = _leaves(P)
    for proj in (None, (["hi"], ["w", "x"])):
        rj = P.plan_schema(P.GpuRangeJoinExec(l, r, "x", ("lo", True), ("hi", False), join_type, proj))
        nlj = P.plan_schema(P.NestedLoopJoinExec(l, r, _band(), join_type, proj))
        assert list(rj) == list(nlj) and [f.nullable for f in rj] == [f.nullable for f in nlj]


def test_unsupported_reason_names_what_the_library_refuses():
    from datafusion_amd import physical_plan as P
    l, r = _leaves(P)
    node = lambda x, lower, upper: P.GpuRangeJoinExec(l, r, x, lower, upper, "Inner")
    assert P.unsupported_reason(node("x", ("lo", True), ("hi", False))) is None
    assert P.unsupported_reason(node("x", None, ("hi", True))) is None
    assert P.unsupported_reason(node("x", None, None)) == "a range join needs a lower or an upper bound"
    for bad in (node("x", ("price", True), None), node("s", ("name", True), None), node("ok", ("lo", True), None), node("x", ("flag", True), None)):
        assert P.unsupported_reason(bad) == P.RANGE_JOIN_KEY_TYPE and P.RANGE_JOIN_KEY_TYPE.endswith("is not supported on the GPU path")
    assert P.unsupported_reason(node("code", ("lo", True), None)) == P.RANGE_JOIN_DICT_KEY
    assert P.unsupported_reason(node("x", ("lo32", True), None)) == P.RANGE_JOIN_MIXED_KEYS
    assert P.unsupported_reason(node("x", ("lo", True), ("lo32", True))) == P.RANGE_JOIN_MIXED_KEYS
    assert "out of range" in P.unsupported_reason(node(9, ("lo", True), None))
    for msg in (P.RANGE_JOIN_DICT_KEY, P.RANGE_JOIN_MIXED_KEYS):
        assert msg.endswith("is not supported on the GPU path")
    # the library's own words (the run-time refusals are held to them on the GPU)
    kernel = open(os.path.join(ROOT, "datafusion_amd", "csrc", "nlj.hip")).read()
    for msg in (P.RANGE_JOIN_NO_BOUND, P.RANGE_JOIN_DICT_KEY, P.RANGE_JOIN_KEY_TYPE, P.RANGE_JOIN_MIXED_KEYS):
        assert f'"{msg}"' in kernel


# ------------------------------------------------------------------------------------------------------------------------ the rule
def _forms():
    """(name, filter, x, lower, upper) of every accepted form over the stub leaves"""
    from datafusion_amd.expr import col
    f0, f1, f2 = col("f0"), col("f1"), col("f2")
    lr, llr = [(0, "Left"), (0, "Right")], [(0, "Left"), (1, "Left"), (0, "Right")]
    return [
        ("band", ((f0 <= f2).and_(f2 < f1), llr), 0, (0, True), (1, False)),
        ("band_operands_swapped", ((f2 >= f0).and_(f1 > f2), llr), 0, (0, True), (1, False)),
        ("band_upper_first", ((f2 <= f1).and_(f0 < f2), llr), 0, (0, False), (1, True)),
        ("lower_only", (f0 < f1, lr), 0, (0, False), None),
        ("lower_only_swapped", (f1 >= f0, lr), 0, (0, True), None),
        ("upper_only", (f1 <= f0, lr), 0, None, (0, True)),
        ("upper_only_swapped", (f0 > f1, lr), 0, None, (0, False)),
        ("same_left_column_twice", ((f0 <= f1).and_(f1 <= f0), lr), 0, (0, True), (0, True)),
        ("right_column_2", (f0 < f1, [(1, "Left"), (2, "Right")]), 2, (1, False), None),
        ("indexed_columns", (col("a", 0) < col("b", 1), lr), 0, (0, False), None),
    ]


def _declined():
    """(name, filter) of forms that stay a nested-loop join"""
    from datafusion_amd.expr import col, lit
    f0, f1, f2, f3 = col("f0"), col("f1"), col("f2"), col("f3")
    lr, llr = [(0, "Left"), (0, "Right")], [(0, "Left"), (1, "Left"), (0, "Right")]
    return [
        ("extra_conjunct", ((f0 <= f2).and_(f2 < f1).and_(f0 < f1), llr)),
        ("expression_operand", (f1 > f0 * lit(2), lr)),
        ("literal_operand", ((f0 <= f2).and_(f2 < lit(7)), llr)),
        ("two_lower_bounds", ((f0 <= f2).and_(f1 < f2), llr)),
        ("two_upper_bounds", ((f2 <= f0).and_(f2 < f1), llr)),
        ("both_columns_of_one_side", ((f0 <= f2).and_(f0 < f1), llr)),
        ("one_comparison_inside_one_side", (f0 < f1, [(0, "Left"), (1, "Left")])),
        ("not_equal", (f0.ne(f1), lr)),
        ("equal", (f0.eq(f1), lr)),
        ("or", ((f0 <= f2).or_(f2 < f1), llr)),
        ("two_right_columns", ((f0 <= f2).and_(f3 < f1), [(0, "Left"), (1, "Left"), (0, "Right"), (2, "Right")])),
        ("decimal_keys", (f0 < f1, [(4, "Left"), (0, "Right")])),
        ("utf8_keys", (f0 < f1, [(2, "Left"), (4, "Right")])),
        ("dictionary_key", (f0 < f1, [(2, "Left"), (3, "Right")])),
        ("uint8_key", (f0 < f1, [(5, "Left"), (0, "Right")])),
        ("mixed_key_types", (f0 < f1, [(3, "Left"), (0, "Right")])),
        ("no_filter", None),
    ]


@pytest.mark.parametrize("form", _forms(), ids=[f[0] for f in _forms()])
def test_the_rule_rewrites_every_accepted_form_when_asked(form):
    from datafusion_amd import physical_plan as P
    _, flt, x, lower, upper = form
    l, r = _leaves(P)
    for jt in ALL_TYPES:
        node = lambda: P.NestedLoopJoinExec(l, r, flt, jt, (["hi"], ["w"]))
        # the default: exactly as before
        plain, asked = P.GpuOffloadRule(), P.GpuOffloadRule(range_joins=True)
        out = plain.optimize(node())
        assert type(out) is P.NestedLoopJoinExec and P.displayable(out) == P.displayable(node()) and not plain.declined
        # asked, at the root: the one-sided types only (the root's order is observed and the pair order differs)
        out = asked.optimize(node())
        if jt in PAIR_TYPES:
            assert type(out) is P.NestedLoopJoinExec and P.displayable(out) == P.displayable(node())
        else:
            assert type(out) is P.GpuRangeJoinExec and (out.x, out.lower, out.upper, out.join_type, out.projection) == (x, lower, upper, jt, (["hi"], ["w"]))
            assert out.left is l and out.right is r
        # asked, below an aggregate: every type
        agg = asked.optimize(P.AggregateExec("Single", [], [("count", None, "c")], node()))
        out = agg.children()[0]
        assert type(out) is P.GpuRangeJoinExec and (out.x, out.lower, out.upper, out.join_type) == (x, lower, upper, jt)
        assert not asked.declined


@pytest.mark.parametrize("form", _declined(), ids=[f[0] for f in _declined()])
def test_every_other_form_stays_a_nested_loop_join(form):
    from datafusion_amd import physical_plan as P
    _, flt = form
    l, r = _leaves(P)
    for jt in ("Inner", "RightSemi", "LeftMark"):
        node = lambda: P.AggregateExec("Single", [], [("count", None, "c")], P.NestedLoopJoinExec(l, r, flt, jt))
        asked, plain = P.GpuOffloadRule(range_joins=True).optimize(node()), P.GpuOffloadRule().optimize(node())
        assert type(asked.children()[0]) is P.NestedLoopJoinExec
        assert P.displayable(asked) == P.displayable(plain)


def test_several_ranks_and_untyped_children_stay_a_nested_loop_join():
    from datafusion_amd import physical_plan as P
    l, r = _leaves(P)
    rule = P.GpuOffloadRule(world_size=2, range_joins=True)
    out = rule.optimize(P.NestedLoopJoinExec(l, r, _band(), "RightSemi"))
    assert type(out) is P.NestedLoopJoinExec and getattr(out, "kept_on_cpu", False) and "2 ranks" in rule.declined[0][1]
    # leaves without a schema: the key types cannot be checked at plan time
    bare = P.NestedLoopJoinExec(P.MemoryExec(StubTable(10), "l"), P.MemoryExec(StubTable(100), "r"), _band(), "RightSemi")
    assert type(P.GpuOffloadRule(range_joins=True).optimize(bare)) is P.NestedLoopJoinExec
    # a cross join is no range join
    assert type(P.GpuOffloadRule(range_joins=True).optimize(P.CrossJoinExec(l, r))) is P.CrossJoinExec


def test_the_default_leaves_the_q11_shape_and_a_band_join_exactly_as_they_were():
    """the same node types and the same displayable text with the default argument as without the argument"""
    from decimal import Decimal

    from datafusion_amd import physical_plan as P
    from datafusion_amd.expr import col, lit
    sch = pa.schema([pa.field("k", pa.int64()), pa.field("v", pa.decimal128(15, 2))])
    t = lambda: P.MemoryExec(StubTable(4000, sch), "t")
    grouped = lambda: P.AggregateExec("Single", [(col("k"), "k")], [("sum", col("v"), "value")], t())
    total = lambda: P.AggregateExec("Single", [], [("sum", col("v"), "total")], t())
    frac = lit(Decimal("0.0001"), pa.decimal128(5, 4))
    q11 = lambda: P.NestedLoopJoinExec(total(), grouped(), (col("f1") > col("f0") * frac, [(0, "Left"), (1, "Right")]), "Inner", ([], ["k", "value"]))
    l, r = _leaves(P)
    band = lambda: P.AggregateExec("Single", [], [("count", None, "c")], P.CoalesceBatchesExec(P.NestedLoopJoinExec(l, r, _band(), "Inner")))
    types = lambda n: [type(n).__name__] + [x for c in n.children() for x in types(c)]
    for plan in (q11, band):
        a, b = P.GpuOffloadRule().optimize(plan()), P.GpuOffloadRule(range_joins=False).optimize(plan())
        c = P.GpuOffloadRule(1, True).optimize(plan())
        assert types(a) == types(b) == types(c) and P.displayable(a) == P.displayable(b) == P.displayable(c)
        assert "GpuRangeJoinExec" not in types(a) and "NestedLoopJoinExec" in types(a)
    # and asked: the Q11 filter multiplies (an expression, over Decimal128) and stays; the band join below the aggregate is taken
    assert "GpuRangeJoinExec" not in types(P.GpuOffloadRule(range_joins=True).optimize(q11()))
    assert types(P.GpuOffloadRule(range_joins=True).optimize(band())) == ["AggregateExec", "GpuRangeJoinExec", "MemoryExec", "MemoryExec"]
