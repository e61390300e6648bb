"""The window operator's boundary without a GPU: ABI 17 (dfgpu_window, dfgpu_window_spec and its ctypes mirror, the enums and the tile
constant the Python layer restates), the plan node's display, and what GpuOffloadRule tells the nodes below a WindowAggExec about order."""
import ctypes as C
import os
import re
import subprocess

from datafusion_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "dfgpu.h")).read()


class StubTable:
    def __init__(self, n):
        self.num_rows = n


def test_the_library_exports_dfgpu_window_at_abi_17():
    lib = _lib.load()
    assert hasattr(lib, "dfgpu_window") and "dfgpu_window" in _lib.SYMBOLS
    assert int(re.search(r"#define DFGPU_ABI_VERSION (\d+)", HEADER).group(1)) >= 17 and lib.dfgpu_abi_version() >= 17


def test_window_spec_layout_matches_the_header(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dfgpu.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(dfgpu_window_spec), '
                   'offsetof(dfgpu_window_spec, func), offsetof(dfgpu_window_spec, has_arg), offsetof(dfgpu_window_spec, arg), '
                   'offsetof(dfgpu_window_spec, frame), offsetof(dfgpu_window_spec, name));return 0;}')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    S = _lib.WindowSpec
    assert got == [C.sizeof(S), S.func.offset, S.has_arg.offset, S.arg.offset, S.frame.offset, S.name.offset], got


def test_python_constants_restate_the_header():
    from datafusion_amd import ops
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    funcs = dict(re.findall(r"DFGPU_WINDOW_(ROW_NUMBER|RANK|DENSE_RANK|SUM|COUNT|MIN|MAX|AVG) = (\d+)", body))
    assert {k.lower(): int(v) for k, v in funcs.items()} == ops.WINDOW_FUNCS
    frames = dict(re.findall(r"DFGPU_WINDOW_(RANGE_TO_CURRENT|ROWS_TO_CURRENT|PARTITION) = (\d+)", body))
    assert {k.lower(): int(v) for k, v in frames.items()} == ops.WINDOW_FRAMES
    assert int(re.search(r"#define DFGPU_WINDOW_TILE (\d+)", body).group(1)) == ops.WINDOW_TILE
    kernel = open(os.path.join(ROOT, "datafusion_amd", "csrc", "window.hip")).read()
    assert "static_assert(WIN_TILE == DFGPU_WINDOW_TILE" in kernel     # the kernels' tile is the header's, checked when the library is compiled


def test_window_expressions_are_normalised_and_checked():
    import pytest

    from datafusion_amd import ops
    from datafusion_amd.expr import col
    v = col("v")
    assert ops.normalize_window_exprs([("sum", v, "s", None), ("rank", v, "r", "partition"), ("count", None, "c")]) == [
        ("sum", v, "s", "range_to_current"), ("rank", None, "r", "partition"), ("count", None, "c", "range_to_current")]
    with pytest.raises(ValueError, match="not supported on the GPU path"):
        ops.normalize_window_exprs([("lag", v, "l", None)])
    with pytest.raises(ValueError, match="not supported on the GPU path"):
        ops.normalize_window_exprs([("sum", v, "s", "groups_2_preceding")])


def test_displayable_prints_the_node():
    from datafusion_amd import physical_plan as P
    from datafusion_amd.expr import col
    w = P.WindowAggExec([("rank", None, "rk", None), ("sum", col("v"), "running", None), ("avg", col("v"), "whole", "partition")], ["g"],
                        [("d", True, True), "e"], P.SortExec([("g", False, False), ("d", True, True), ("e", False, False)], P.MemoryExec(StubTable(10), "t")))
    lines = P.displayable(w).split("\n")
    assert lines[0] == ("WindowAggExec: wdw=[rank() AS rk, sum(v@None) range_to_current AS running, avg(v@None) partition AS whole], "
                        "partition_by=[g], order_by=[d DESC NULLS FIRST, e ASC NULLS LAST]")
    assert lines[1].startswith("  SortExec: ") and lines[2].startswith("    MemoryExec")
    again = w.with_new_children([w.input])
    assert isinstance(again, P.WindowAggExec) and P.displayable(again) == P.displayable(w)


def _join(P):
    return P.HashJoinExec(P.MemoryExec(StubTable(10), "b"), P.MemoryExec(StubTable(100), "p"), [("k", "k2")], "Inner")


def test_the_rule_demands_order_of_the_windows_child_and_not_of_the_sorts_child():
    """A join's probe mode shows what the rule told it: below an aggregate the probe order is not needed — unless a window sits
    between them, whose partitions and peer groups ARE its input's order; a SortExec below the window makes the order itself, so the
    join below THAT is free again."""
    from datafusion_amd import ops, physical_plan as P
    free = ops.PROBE_MODES["order_not_needed"]
    wexpr = [("row_number", None, "rn", None)]

    def agg(child):
        return P.AggregateExec("Single", [], [("count", None, "c")], child)
    plain = P.GpuOffloadRule().optimize(agg(_join(P)))
    assert plain.children()[0].probe_mode == free
    direct = P.GpuOffloadRule().optimize(agg(P.WindowAggExec(wexpr, ["k"], ["k2"], _join(P))))
    win = direct.children()[0]
    assert isinstance(win, P.WindowAggExec) and not getattr(win, "kept_on_cpu", False)
    assert isinstance(win.input, P.HashJoinExec) and win.input.probe_mode != free
    through_filter = P.GpuOffloadRule().optimize(agg(P.WindowAggExec(wexpr, ["k"], ["k2"], P.CoalesceBatchesExec(_join(P)))))
    assert through_filter.children()[0].input.probe_mode != free
    sorted_below = P.GpuOffloadRule().optimize(agg(P.WindowAggExec(wexpr, ["k"], ["k2"], P.SortExec([("k", False, False), ("k2", False, False)], _join(P)))))
    sort = sorted_below.children()[0].input
    assert isinstance(sort, P.SortExec) and sort.input.probe_mode == free
    # the window hands its parent's need on: what is ABOVE it is decided as before (a join whose probe side is the window)
    above = P.GpuOffloadRule().optimize(agg(P.HashJoinExec(P.MemoryExec(StubTable(5), "b2"), P.WindowAggExec(wexpr, ["k"], ["k2"], _join(P)), [("k", "k")], "Inner")))
    assert above.children()[0].probe_mode == free and above.children()[0].right.input.probe_mode != free


def test_several_ranks_keep_the_window_on_the_cpu_and_say_why():
    from datafusion_amd import physical_plan as P
    plan = P.WindowAggExec([("rank", None, "rk", None)], ["k"], ["k2"], P.SortExec([("k", False, False), ("k2", False, False)], P.MemoryExec(StubTable(10), "t")))
    rule = P.GpuOffloadRule(world_size=2)
    out = rule.optimize(plan)
    assert isinstance(out, P.WindowAggExec) and getattr(out, "kept_on_cpu", False)
    assert len(rule.declined) == 1 and rule.declined[0][0] is out and "2 ranks" in rule.declined[0][1]
    one = P.GpuOffloadRule()
    assert not getattr(one.optimize(plan), "kept_on_cpu", False) and not one.declined
