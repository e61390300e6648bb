"""ABI 18 without a GPU: the six window functions beside the eight of ABI 17 — the header's enumerators against the Python tables,
dfgpu_window_spec.n and its ctypes mirror, how a window expression carries ntile's and nth_value's integer, the parameter errors, and
the plan node's display."""
import ctypes as C
import os
import re
import subprocess

import pytest

from datafusion_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "dfgpu.h")).read()


class StubTable:
    def __init__(self, n):
        self.num_rows = n


def test_the_header_and_the_library_are_at_abi_18():
    lib = _lib.load()
    assert int(re.search(r"#define DFGPU_ABI_VERSION (\d+)", HEADER).group(1)) >= 18 and lib.dfgpu_abi_version() >= 18


def test_python_tables_restate_the_new_enumerators():
    from datafusion_amd import ops
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    enum = re.search(r"typedef enum dfgpu_window_func \{(.*?)\} dfgpu_window_func;", body, flags=re.S).group(1)
    all_funcs = {k.lower(): int(v) for k, v in re.findall(r"DFGPU_WINDOW_(\w+) = (\d+)", enum)}
    assert sorted(all_funcs.values()) == list(range(14))
    assert {k: v for k, v in all_funcs.items() if v >= 8} == dict(ops.WINDOW_DIST_FUNCS, **ops.WINDOW_VALUE_FUNCS)
    assert ops.WINDOW_DIST_FUNCS == {"percent_rank": 8, "cume_dist": 9, "ntile": 10}
    assert ops.WINDOW_VALUE_FUNCS == {"first_value": 11, "last_value": 12, "nth_value": 13}
    assert {k: v for k, v in all_funcs.items() if v < 8} == ops.WINDOW_FUNCS              # the old table is as it was
    assert ops.WINDOW_RANKING == frozenset(("row_number", "rank", "dense_rank"))
    assert [ops.window_func_code(f) for f in ("rank", "avg", ("ntile", 3), "cume_dist", ("nth_value", -1), "first_value")] == [1, 7, 10, 9, 13, 11]


def test_window_spec_n_is_the_last_field_and_matches_the_header(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dfgpu.h"\nint main(void){printf("%zu %zu %zu %zu\\n", sizeof(dfgpu_window_spec), '
                   'offsetof(dfgpu_window_spec, n), offsetof(dfgpu_window_spec, name), sizeof(((dfgpu_window_spec*)0)->n));return 0;}')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off_n, off_name, width = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    S = _lib.WindowSpec
    assert (size, off_n, off_name, width) == (C.sizeof(S), S.n.offset, S.name.offset, 8)
    assert S._fields_[-1][0] == "n" and off_n > off_name and off_n + 8 == size
    assert S().n == 0                                                                      # a zeroed struct is an ABI 17 spec


def test_new_window_expressions_are_normalised_and_checked():
    from datafusion_amd import ops
    from datafusion_amd.expr import col
    v = col("v")
    got = ops.normalize_window_exprs([(("ntile", 4), None, "q", None), ("percent_rank", v, "pr", "partition"), ("cume_dist", None, "cd"),
                                      (("nth_value", -2), v, "x", "partition"), ("first_value", v, "f", None), ("last_value", v, "l", "rows_to_current"),
                                      (["ntile", 2**40], v, "big", None), ("sum", v, "s", None), ("rank", v, "r", "partition")])
    assert got == [(("ntile", 4), None, "q", "range_to_current"), ("percent_rank", None, "pr", "partition"), ("cume_dist", None, "cd", "range_to_current"),
                   (("nth_value", -2), v, "x", "partition"), ("first_value", v, "f", "range_to_current"), ("last_value", v, "l", "rows_to_current"),
                   (("ntile", 2**40), None, "big", "range_to_current"), ("sum", v, "s", "range_to_current"), ("rank", None, "r", "partition")]
    assert ops.normalize_window_exprs(got) == got                                          # normal forms are fixed points
    for bad, message in [((("ntile", 0), None, "q", None), "NTILE needs a positive number of buckets"),
                         ((("ntile", -1), None, "q", None), "NTILE needs a positive number of buckets"),
                         ((("nth_value", 0), v, "x", None), "NTH_VALUE needs a non-zero n"),
                         (("first_value", None, "f", None), "FIRST_VALUE needs an argument"),
                         (("last_value", None, "l", None), "LAST_VALUE needs an argument"),
                         ((("nth_value", 1), None, "x", None), "NTH_VALUE needs an argument")]:
        with pytest.raises(ValueError) as err:
            ops.normalize_window_exprs([bad])
        assert str(err.value) == message
    for bad in [("ntile", None, "q", None), (("ntile", 2.0), None, "q", None), (("ntile", True), None, "q", None), (("ntile", None), None, "q", None),
                ("nth_value", v, "x", None), (("nth_value", "2"), v, "x", None), (("ntile", 2**63), None, "q", None), (("ntile", 1, 2), None, "q", None),
                (("rank", 3), None, "r", None), (("sum", 1), v, "s", None), (("first_value", 1), v, "f", None), (("percent_rank", 2), None, "p", None),
                (("rank", None), None, "r", None)]:
        with pytest.raises(ValueError):
            ops.normalize_window_exprs([bad])


def test_what_abi_17_refused_is_still_refused():
    from datafusion_amd import ops
    from datafusion_amd.expr import col
    v = col("v")
    with pytest.raises(ValueError, match="window function 'lag' is not supported on the GPU path"):
        ops.normalize_window_exprs([("lag", v, "l", None)])
    with pytest.raises(ValueError, match="window function 'lead' is not supported on the GPU path"):
        ops.normalize_window_exprs([(("lead", 1), v, "l", None)])
    for func in ("sum", "first_value", ("nth_value", 1)):
        with pytest.raises(ValueError, match="window frame 'groups_2_preceding' is not supported on the GPU path"):
            ops.normalize_window_exprs([(func, v, "s", "groups_2_preceding")])


def test_displayable_prints_the_new_functions():
    from datafusion_amd import physical_plan as P
    from datafusion_amd.expr import col
    w = P.WindowAggExec([(("ntile", 4), None, "q", None), ("percent_rank", None, "pr", None), (("nth_value", -2), col("v"), "x", "partition"),
                         ("first_value", col("v"), "f", None), ("cume_dist", col("v"), "cd", "rows_to_current"), ("rank", None, "rk", None),
                         ("sum", col("v"), "running", None)], ["g"], ["d"], P.SortExec([("g", False, False), ("d", False, False)], P.MemoryExec(StubTable(10), "t")))
    lines = P.displayable(w).split("\n")
    assert lines[0] == ("WindowAggExec: wdw=[ntile(4) AS q, percent_rank() AS pr, nth_value(v@None, -2) partition AS x, "
                        "first_value(v@None) range_to_current AS f, cume_dist() AS cd, rank() AS rk, sum(v@None) range_to_current AS running], "
                        "partition_by=[g], order_by=[d ASC NULLS LAST]")
    for piece in ("ntile(4) AS q", "percent_rank() AS pr"):
        assert piece in lines[0]
    assert "nth_value(v, -2) partition AS x" in lines[0].replace("@None", "")
    again = w.with_new_children([w.input])
    assert isinstance(again, P.WindowAggExec) and P.displayable(again) == P.displayable(w)
    opt = P.GpuOffloadRule().optimize(w)                                                   # nothing in the new forms trips the rule
    assert isinstance(opt, P.WindowAggExec) and not getattr(opt, "kept_on_cpu", False)
