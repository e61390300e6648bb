"""The nested-loop join's boundary without a GPU: ABI 19 (dfgpu_nested_loop_join in the header, the library and the ctypes binding), the
two plan nodes' display and schemas, and what GpuOffloadRule does with them."""
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


class StubTable:
    """a leaf table for planning only: a row count and a schema"""

    def __init__(self, n, schema=None):
        self.num_rows, self.schema = n, schema

    def index_of(self, c):
        return c if isinstance(c, int) else self.schema.get_field_index(c)


LS = pa.schema([pa.field("lo", pa.int64(), nullable=False), pa.field("hi", pa.int64(), nullable=False), pa.field("name", pa.string())])
RS = pa.schema([pa.field("x", pa.int64(), nullable=False), pa.field("w", pa.float64(), nullable=False)])


def _leaves(P):
    return P.MemoryExec(StubTable(10, LS), "l"), P.MemoryExec(StubTable(100, RS), "r")


def _band():
    from datafusion_amd.expr import col
    return (col("f0") <= col("f2")).and_(col("f2") < col("f1")), [(0, "Left"), (1, "Left"), (0, "Right")]


def test_the_header_declares_and_the_library_exports_dfgpu_nested_loop_join_at_abi_19():
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    decl = re.search(r"int dfgpu_nested_loop_join\((.*?)\);", body, flags=re.S)
    assert decl is not None
    args = [a.strip() for a in decl.group(1).split(",")]
    assert args == ["dfgpu_table_t left", "dfgpu_table_t right", "int join_type", "const dfgpu_join_filter* filter", "const int* left_out_cols",
                    "int n_left_out", "const int* right_out_cols", "int n_right_out", "dfgpu_table_t* out"]
    lib = _lib.load()
    assert hasattr(lib, "dfgpu_nested_loop_join") and "dfgpu_nested_loop_join" in _lib.SYMBOLS
    assert int(re.search(r"#define DFGPU_ABI_VERSION (\d+)", HEADER).group(1)) >= 19 and lib.dfgpu_abi_version() >= 19
    # the order contract is part of the declaration's comment
    comment = HEADER[:HEADER.index("int dfgpu_nested_loop_join(")].rsplit("/*", 1)[1]
    assert "right-row-major" in comment and "unmatched right rows" in comment and "unmatched left rows" in comment


def test_the_call_before_dfgpu_init_fails_with_the_init_message():
    """in a process of its own: this one may have initialised a device already"""
    code = ("import ctypes as C\nfrom datafusion_amd import _lib\nlib = _lib.load()\nout = C.c_void_p()\none = (C.c_int * 1)(0)\n"
            "rc = lib.dfgpu_nested_loop_join(None, None, 0, None, one, 0, one, 0, C.byref(out))\nprint(rc, lib.dfgpu_last_error().decode())\n")
    got = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert got.returncode == 0, got.stderr
    assert got.stdout.startswith("1 ") and "dfgpu_init() has not been called" in got.stdout


def test_displayable_prints_both_nodes_and_is_a_fixed_point_under_with_new_children():
    from datafusion_amd import physical_plan as P
    l, r = _leaves(P)
    from datafusion_amd.expr import col
    n = P.NestedLoopJoinExec(l, r, (col("f0") < col("f1"), [(0, "Left"), (0, "Right")]), "Left")
    lines = P.displayable(n).split("\n")
    assert lines[0] == "NestedLoopJoinExec: join_type=Left, filter=(f0@None < f1@None)"
    assert lines[1].startswith("  MemoryExec: l") and lines[2].startswith("  MemoryExec: r")
    again = n.with_new_children(n.children())
    assert type(again) is P.NestedLoopJoinExec and P.displayable(again) == P.displayable(n)
    p = P.NestedLoopJoinExec(l, r, None, "RightSemi", (["lo"], ["x"]))
    assert P.displayable(p).split("\n")[0] == "NestedLoopJoinExec: join_type=RightSemi, projection=(['lo'], ['x'])"
    assert P.displayable(p.with_new_children([l, r])) == P.displayable(p)
    c = P.CrossJoinExec(l, r)
    assert P.displayable(c).split("\n")[0] == "CrossJoinExec" and c.children() == [l, r] and c.filter is None and c.join_type == "Inner"
    again = c.with_new_children([l, r])
    assert type(again) is P.CrossJoinExec and P.displayable(again) == P.displayable(c)
    with pytest.raises(ValueError, match="unknown join type"):
        P.NestedLoopJoinExec(l, r, None, "Outer")


@pytest.mark.parametrize("join_type", ALL_TYPES)
def test_plan_schema_of_every_join_type(join_type):
    from datafusion_amd import physical_plan as P
    l, r = _leaves(P)
    sch = P.plan_schema(P.NestedLoopJoinExec(l, r, _band(), join_type))
    mark = [pa.field("mark", pa.bool_(), nullable=False)]
    nullable = lambda s: [f.with_nullable(True) for f in s]
    want = {"Inner": list(LS) + list(RS), "Left": list(LS) + nullable(RS), "Right": nullable(LS) + list(RS), "Full": nullable(LS) + nullable(RS),
            "LeftSemi": list(LS), "LeftAnti": list(LS), "RightSemi": list(RS), "RightAnti": list(RS), "LeftMark": list(LS) + mark,
            "RightMark": list(RS) + mark}[join_type]
    assert list(sch) == want and [f.nullable for f in sch] == [f.nullable for f in want]
    proj = P.plan_schema(P.NestedLoopJoinExec(l, r, _band(), join_type, (["hi"], ["w", "x"])))
    names = {"LeftSemi": ["hi"], "LeftAnti": ["hi"], "LeftMark": ["hi", "mark"], "RightSemi": ["w", "x"], "RightAnti": ["w", "x"],
             "RightMark": ["w", "x", "mark"]}.get(join_type, ["hi", "w", "x"])
    assert proj.names == names


def test_plan_schema_of_a_cross_join():
    from datafusion_amd import physical_plan as P
    l, r = _leaves(P)
    assert list(P.plan_schema(P.CrossJoinExec(l, r))) == list(LS) + list(RS)


def test_the_rule_keeps_a_typed_plan_on_the_gpu_and_hands_order_to_the_right_side_only():
    from datafusion_amd import ops, physical_plan as P
    free = ops.PROBE_MODES["order_not_needed"]
    l, r = _leaves(P)
    hj = lambda: P.HashJoinExec(P.MemoryExec(StubTable(10), "b"), P.MemoryExec(StubTable(100), "p"), [("k", "k2")], "Inner")
    rule = P.GpuOffloadRule()
    out = rule.optimize(P.NestedLoopJoinExec(l, r, _band(), "Full"))
    assert type(out) is P.NestedLoopJoinExec and not getattr(out, "kept_on_cpu", False) and not rule.declined
    out = rule.optimize(P.CoalesceBatchesExec(P.CrossJoinExec(l, P.CoalesceBatchesExec(r))))
    assert type(out) is P.CrossJoinExec and out.right is r and not rule.declined
    # the order of the join's output is the right side's: a hash join on the left side may probe in any order, one on the right may not
    both = P.GpuOffloadRule().optimize(P.NestedLoopJoinExec(hj(), hj(), None, "Inner"))
    assert both.left.probe_mode == free and both.right.probe_mode != free
    # below an aggregate nobody needs any order
    agg = P.GpuOffloadRule().optimize(P.AggregateExec("Single", [], [("count", None, "c")], P.NestedLoopJoinExec(hj(), hj(), None, "Inner")))
    assert agg.children()[0].left.probe_mode == free and agg.children()[0].right.probe_mode == free


def test_several_ranks_keep_the_node_on_the_cpu_and_say_why():
    from datafusion_amd import physical_plan as P
    l, r = _leaves(P)
    for node in (P.NestedLoopJoinExec(l, r, _band(), "Left"), P.CrossJoinExec(l, r)):
        rule = P.GpuOffloadRule(world_size=2)
        out = rule.optimize(node)
        assert type(out) is type(node) and getattr(out, "kept_on_cpu", False)
        assert len(rule.declined) == 1 and rule.declined[0][0] is out and "2 ranks" in rule.declined[0][1] and node.name() in rule.declined[0][1]


def test_hash_join_rewriting_is_left_as_it_is():
    from datafusion_amd import physical_plan as P
    from datafusion_amd.expr import col, lit
    probe = P.FilterExec(col("v") > lit(3), P.MemoryExec(StubTable(100), "p"))
    plan = P.NestedLoopJoinExec(P.MemoryExec(StubTable(5), "l"), P.HashJoinExec(P.MemoryExec(StubTable(10), "b"), probe, [("k", "k2")], "Inner"), None, "Inner")
    out = P.GpuOffloadRule().optimize(plan)
    assert type(out) is P.NestedLoopJoinExec and type(out.right) is P.GpuHashJoinExec
    alone = P.GpuOffloadRule().optimize(P.HashJoinExec(P.MemoryExec(StubTable(10), "b"), probe, [("k", "k2")], "Inner"))
    assert P.displayable(alone) == P.displayable(out.right)
