"""COUNT(DISTINCT) / SUM(DISTINCT) at the boundary, without a GPU: ABI 21 (the two function ids in the header, the Python table and the
generated Rust bindings; dfgpu_agg_spec unchanged), the plan layer's result types and refusals, and what GpuOffloadRule does with the
Final(Partial) pair of a multi-partition plan that carries a DISTINCT aggregate."""
import os
import re
import subprocess
import sys

import pyarrow as pa

from datafusion_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "dfgpu.h")).read()


class StubTable:
    """a leaf table for planning only: a row count and a schema"""

    def __init__(self, n, schema=None):
        self.num_rows, self.schema = n, schema

    def index_of(self, c):
        return c if isinstance(c, int) else self.schema.get_field_index(c)


SCHEMA = pa.schema([pa.field("r", pa.int32()), pa.field("a", pa.int64()), pa.field("w", pa.float64()), pa.field("u", pa.int64()), pa.field("p", pa.bool_())])


def test_the_header_carries_the_two_functions_at_abi_21():
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    enum = re.search(r"typedef enum dfgpu_agg_func \{(.*?)\} dfgpu_agg_func;", body, re.S).group(1)
    ids = {n: int(v) for n, v in re.findall(r"DFGPU_AGG_(\w+)\s*=\s*(\d+)", enum)}
    assert ids["COUNT_DISTINCT"] == 14 and ids["SUM_DISTINCT"] == 15 and len(set(ids.values())) == len(ids) == 16
    assert int(re.search(r"#define DFGPU_ABI_VERSION (\d+)", HEADER).group(1)) >= 21 and _lib.load().dfgpu_abi_version() >= 21
    assert ops.AGG_FUNCS["count_distinct"] == 14 and ops.AGG_FUNCS["sum_distinct"] == 15
    assert ops.DISTINCT_FUNCS == {"count_distinct", "sum_distinct"}
    # every older id is where it was
    assert {k: ops.AGG_FUNCS[k] for k in ("sum", "min", "max", "count", "avg", "var", "stddev_pop", "bit_and", "bool_or")} == \
        {"sum": 0, "min": 1, "max": 2, "count": 3, "avg": 4, "var": 5, "stddev_pop": 8, "bit_and": 9, "bool_or": 13}
    # the semantics are part of the header
    comment = HEADER[:HEADER.index("typedef enum dfgpu_agg_func")].rsplit("COUNT_DISTINCT / SUM_DISTINCT (ABI 21)", 1)[1]
    for words in ("never NULL", "bit patterns", "SUM(DISTINCT) over Float64 is not", "over Boolean is not supported on the GPU path", "List column", "made unique"):
        assert words in comment, words
    assert "agg.distinct_slots" in HEADER


def test_the_spec_struct_is_unchanged():
    body = re.search(r"typedef struct dfgpu_agg_spec \{(.*?)\} dfgpu_agg_spec;", HEADER, re.S).group(1)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == ["func", "has_arg", "arg", "name", "return_field", "has_filter", "filter"]
    assert [f[0] for f in _lib.AggSpec._fields_] == fields


def test_the_rust_bindings_follow_the_header():
    got = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_shim_sys.py"), "--check"], capture_output=True, text=True, timeout=120)
    assert got.returncode == 0, got.stdout + got.stderr
    rs = open(os.path.join(ROOT, "shim", "src", "sys.rs")).read()
    assert re.search(r"DFGPU_AGG_COUNT_DISTINCT\s*:\s*\w+\s*=\s*14", rs) and re.search(r"DFGPU_AGG_SUM_DISTINCT\s*:\s*\w+\s*=\s*15", rs)
    assert re.search(r"DFGPU_ABI_VERSION\s*:\s*i32\s*=\s*(\d+)", rs).group(1) == re.search(r"#define DFGPU_ABI_VERSION (\d+)", HEADER).group(1)


def test_result_types():
    from datafusion_amd import physical_plan as P
    for t in (pa.int32(), pa.float64(), pa.string(), pa.decimal128(15, 2), pa.date32()):
        assert P._agg_type("count_distinct", t) == pa.int64()
    assert P._agg_type("sum_distinct", pa.int32()) == pa.int64() and P._agg_type("sum_distinct", pa.uint8()) == pa.int64()
    assert P._agg_type("sum_distinct", pa.uint32()) == pa.uint64() and P._agg_type("sum_distinct", pa.uint64()) == pa.uint64()
    assert P._agg_type("sum_distinct", pa.decimal128(15, 2)) == pa.decimal128(25, 2) == P._agg_type("sum", pa.decimal128(15, 2))


def _staged(P, aggs, final="FinalPartitioned", world=1, below_filter=True):
    """FinalPartitioned(CoalesceBatches(Repartition(Partial(Projection(Filter(scan)))))): what a multi-partition plan carries"""
    from datafusion_amd.expr import col, lit
    leaf = P.MemoryExec(StubTable(1000, SCHEMA), "t")
    inp = leaf
    if below_filter:
        inp = P.ProjectionExec([(col("r"), "r"), (col("a") + col("u"), "au"), (col("w"), "w"), (col("u"), "u"), (col("p"), "p")], P.FilterExec(col("a") > lit(3), leaf))
    partial = P.AggregateExec("Partial", [(col("r"), "r")], aggs, inp)
    final_aggs = [(a[0], col(a[2]), "out_" + a[2]) for a in aggs]
    plan = P.AggregateExec(final, [(col("r"), "r_out")], final_aggs, P.CoalesceBatchesExec(P.RepartitionExec(partial, ["r"], 4)))
    return plan, partial, leaf, P.GpuOffloadRule(world_size=world)


def _mixed_aggs():
    from datafusion_amd.expr import col
    return [("sum", col("au"), "s"), ("avg", col("w"), "m"), ("count_distinct", col("u"), "d", col("p")), ("sum_distinct", col("u"), "sd")]


def test_one_rank_collapses_final_over_partial_into_one_single_node():
    from datafusion_amd import physical_plan as P
    plan, partial, leaf, rule = _staged(P, _mixed_aggs())
    out = rule.optimize(plan)
    # the ProjectionExec(FilterExec) below goes into the node as for any Single aggregate; its update falls back inside the library
    assert type(out) is P.GpuFusedAggregateExec and out.mode == "Single" and out.input is leaf and not rule.declined
    assert [n for _, n in out.group_by] == ["r_out"] and repr(out.group_by[0][0]) == repr(partial.group_by[0][0])
    got = ops.normalize_aggs(out.aggr_expr)
    assert [(f, n) for f, _, n, _ in got] == [("sum", "out_s"), ("avg", "out_m"), ("count_distinct", "out_d"), ("sum_distinct", "out_sd")]
    assert repr(got[0][1]) == "(a@None + u@None)" and repr(got[2][1]) == "u@None"                 # the projection's expressions, inlined
    assert repr(got[2][3]) == "p@None" and got[3][3] is None and repr(out.predicate) == "(a@None > 3:int64)"
    assert not getattr(out, "kept_on_cpu", False)
    # without a FilterExec below: a plain Single AggregateExec over the Partial's input, Final (not partitioned) alike
    plan, partial, leaf, rule = _staged(P, _mixed_aggs()[2:], final="Final", below_filter=False)
    out = rule.optimize(plan)
    assert type(out) is P.AggregateExec and out.mode == "Single" and out.input is leaf and not rule.declined
    assert P.displayable(out).split("\n")[0] == "AggregateExec: mode=Single, gby=[r_out], aggr=[out_d FILTER (WHERE p@None), out_sd]"


def test_two_ranks_keep_both_nodes_and_say_why():
    from datafusion_amd import physical_plan as P
    plan, partial, leaf, rule = _staged(P, _mixed_aggs(), world=2)
    out = rule.optimize(plan)
    assert type(out) is P.AggregateExec and out.mode == "FinalPartitioned" and getattr(out, "kept_on_cpu", False)
    below = P._partial_below(out.input)
    assert type(below) is P.AggregateExec and below.mode == "Partial" and getattr(below, "kept_on_cpu", False)
    assert type(below.input) is P.ProjectionExec                                                   # not fused either
    reasons = {node.mode: why for node, why in rule.declined}
    assert reasons == {"Partial": "COUNT(DISTINCT) (aggregate d) is not supported in mode Partial on the GPU path: its partial state is a List column",
                       "FinalPartitioned": "COUNT(DISTINCT) (aggregate out_d) is not supported in mode FinalPartitioned on the GPU path: its partial state is a List column"}


def test_a_partial_that_no_final_consumes_stays_on_the_cpu():
    from datafusion_amd import physical_plan as P
    from datafusion_amd.expr import col
    leaf = P.MemoryExec(StubTable(1000, SCHEMA), "t")
    rule = P.GpuOffloadRule()
    out = rule.optimize(P.CoalesceBatchesExec(P.AggregateExec("Partial", [(col("r"), "r")], [("sum_distinct", col("u"), "sd")], leaf)))
    assert type(out) is P.AggregateExec and out.mode == "Partial" and getattr(out, "kept_on_cpu", False)
    assert rule.declined == [(out, "SUM(DISTINCT) (aggregate sd) is not supported in mode Partial on the GPU path: its partial state is a List column")]
    # the same words for every staged mode, and none for the single-stage ones
    for mode in ("Partial", "Final", "FinalPartitioned", "PartialReduce"):
        why = P.unsupported_reason(P.AggregateExec(mode, [], [("count_distinct", col("u"), "c")], leaf))
        assert why == f"COUNT(DISTINCT) (aggregate c) is not supported in mode {mode} on the GPU path: its partial state is a List column"
    for mode in ("Single", "SinglePartitioned"):
        assert P.unsupported_reason(P.AggregateExec(mode, [], [("count_distinct", col("u"), "c")], leaf)) is None
    assert P.unsupported_reason(P.AggregateExec("Single", [], [("count_distinct", None, "c")], leaf)) == "COUNT(DISTINCT) (aggregate c) needs an argument"


def test_a_plan_without_distinct_is_rewritten_as_before():
    from datafusion_amd import physical_plan as P
    plan, partial, leaf, rule = _staged(P, _mixed_aggs()[:2])
    out = rule.optimize(plan)
    assert type(out) is P.AggregateExec and out.mode == "FinalPartitioned" and not rule.declined and not getattr(out, "kept_on_cpu", False)
    assert type(out.input) is P.GpuFusedAggregateExec and out.input.mode == "Partial" and out.input.input is leaf
    assert P.displayable(out).split("\n") == [
        "AggregateExec: mode=FinalPartitioned, gby=[r_out], aggr=[out_s, out_m]",
        "  GpuFusedAggregateExec: mode=Partial, predicate=(a@None > 3:int64), gby=[r], aggr=[s, m]",
        "    " + P.displayable(leaf)]
    for world in (1, 2):
        plan, _, leaf, rule = _staged(P, _mixed_aggs()[:2], world=world, below_filter=False)
        out = rule.optimize(plan)
        assert out.mode == "FinalPartitioned" and not rule.declined and P._partial_below(out.input).mode == "Partial"


def test_a_node_with_meaning_between_final_and_partial_keeps_the_pair_on_the_cpu():
    """the collapse drops what lies between the two nodes, so only exchange and bookkeeping nodes may lie there"""
    from datafusion_amd import physical_plan as P
    from datafusion_amd.expr import col
    leaf = P.MemoryExec(StubTable(1000, SCHEMA), "t")
    aggs = [("count_distinct", col("u"), "d")]
    for between in (lambda x: P.SortExec([("r", False, False)], x, fetch=10), lambda x: P.FilterExec(col("r") > col("r"), x)):
        partial = P.AggregateExec("Partial", [(col("r"), "r")], aggs, leaf)
        plan = P.AggregateExec("FinalPartitioned", [(col("r"), "r")], [("count_distinct", col("d"), "d")], P.RepartitionExec(between(partial), ["r"], 4))
        rule = P.GpuOffloadRule()
        out = rule.optimize(plan)
        assert type(out) is P.AggregateExec and out.mode == "FinalPartitioned" and getattr(out, "kept_on_cpu", False)
        assert type(out.input) in (P.SortExec, P.FilterExec)                               # still there
        below = P._partial_below(out.input)
        assert below.mode == "Partial" and getattr(below, "kept_on_cpu", False)
        assert sorted(n.mode for n, _ in rule.declined) == ["FinalPartitioned", "Partial"] and all("List column" in why for _, why in rule.declined)


def test_refusals_spell_types_as_the_library_does():
    from datafusion_amd import physical_plan as P
    assert [P._device_type_name(t) for t in (pa.int32(), pa.uint8(), pa.date32(), pa.float64(), pa.bool_(), pa.decimal128(15, 2))] == \
        ["Int32", "UInt8", "Date32", "Float64", "Boolean", "Decimal128(15,2)"]
    src = open(os.path.join(ROOT, "datafusion_amd", "csrc", "runtime.hip")).read()
    body = src[src.index("std::string type_name(const dfgpu_field& f) {"):]
    body = body[:body.index("\n}\n")]
    for name in ("Int32", "Int64", "Float64", "UInt8", "UInt32", "UInt64", "Date32", "Boolean"):
        assert f'return "{name}";' in body, name
    assert '"Decimal128(" + std::to_string(f.precision) + "," + std::to_string(f.scale) + ")"' in body
