"""MEDIAN at the boundary, without a GPU: ABI 22 (the function id in a second enum of the header, the Python table and the generated Rust
bindings; dfgpu_agg_spec and dfgpu_agg_func unchanged), the plan layer's result types and refusals, and what GpuOffloadRule does with
the Final(Partial) pair of a multi-partition plan that carries a MEDIAN."""
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


SCHEMA = pa.schema([pa.field("r", pa.int32()), pa.field("a", pa.int64()), pa.field("w", pa.float64()), pa.field("u", pa.int64()), pa.field("p", pa.bool_()),
                    pa.field("d", pa.date32()), pa.field("s", pa.string()), pa.field("ds", pa.dictionary(pa.int32(), pa.string())), pa.field("m", pa.decimal128(15, 2)),
                    pa.field("b", pa.uint8())])
TAKEN = (pa.int32(), pa.int64(), pa.uint8(), pa.uint32(), pa.uint64(), pa.float64(), pa.decimal128(15, 2), pa.decimal128(38, 4))


def test_the_header_carries_median_outside_dfgpu_agg_func_at_abi_22():
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    first = re.search(r"typedef enum dfgpu_agg_func \{(.*?)\} dfgpu_agg_func;", body, re.S).group(1)
    assert "MEDIAN" not in first and len(re.findall(r"DFGPU_AGG_(\w+)\s*=\s*(\d+)", first)) == 16
    second = re.search(r"typedef enum dfgpu_agg_func_ordered \{(.*?)\} dfgpu_agg_func_ordered;", body, re.S).group(1)
    assert re.findall(r"DFGPU_AGG_(\w+)\s*=\s*(\d+)", second) == [("MEDIAN", "16")]
    assert body.index("} dfgpu_agg_func;") < body.index("typedef enum dfgpu_agg_func_ordered")
    assert int(re.search(r"#define DFGPU_ABI_VERSION (\d+)", HEADER).group(1)) >= 22 and _lib.load().dfgpu_abi_version() >= 22
    assert ops.AGG_FUNCS["median"] == 16 and ops.HOLISTIC_FUNCS == {"median"}
    assert ops.DISTINCT_FUNCS == {"count_distinct", "sum_distinct"}
    assert {k: ops.AGG_FUNCS[k] for k in ("sum", "min", "max", "count", "avg", "var", "stddev_pop", "bit_and", "bool_or", "count_distinct", "sum_distinct")} == \
        {"sum": 0, "min": 1, "max": 2, "count": 3, "avg": 4, "var": 5, "stddev_pop": 8, "bit_and": 9, "bool_or": 13, "count_distinct": 14, "sum_distinct": 15}
    # the contract is part of the header
    comment = HEADER[HEADER.index("} dfgpu_agg_func;"):HEADER.index("typedef enum dfgpu_agg_func_ordered")]
    for words in ("continue dfgpu_agg_func's", "same field", "add_wrapping", "div_wrapping", "gives -1", "gives 72", "truncating toward zero", "totalOrder", "gives +inf",
                  "MEDIAN over Date32 is not supported on the GPU path", "its partial state is a List", "needs an argument", "12 bytes per row", "20 for Decimal128",
                  "double-buffered", "2^31 - 2", "agg.median_rows", "MEDIAN(DISTINCT)", "approx_median", "grouping sets"):
        assert words in comment, words
    assert HEADER.count("agg.median_rows") >= 2                                   # the contract and the list of options


def test_the_spec_struct_is_unchanged():
    body = re.search(r"typedef struct dfgpu_agg_spec \{(.*?)\} dfgpu_agg_spec;", HEADER, re.S).group(1)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == ["func", "has_arg", "arg", "name", "return_field", "has_filter", "filter"]
    assert [f[0] for f in _lib.AggSpec._fields_] == fields
    assert re.search(r"int32_t\s+func;", body)


def test_the_rust_bindings_follow_the_header():
    got = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_shim_sys.py"), "--check"], capture_output=True, text=True, timeout=120)
    assert got.returncode == 0, got.stdout + got.stderr
    rs = open(os.path.join(ROOT, "shim", "src", "sys.rs")).read()
    assert re.search(r"DFGPU_AGG_MEDIAN\s*:\s*\w+\s*=\s*16", rs)
    assert re.search(r"DFGPU_ABI_VERSION\s*:\s*i32\s*=\s*(\d+)", rs).group(1) == re.search(r"#define DFGPU_ABI_VERSION (\d+)", HEADER).group(1)


def test_result_types():
    from datafusion_amd import physical_plan as P
    for t in TAKEN:
        assert P._agg_type("median", t) == t


def test_every_refusal_of_the_plan_layer_in_the_librarys_words():
    from datafusion_amd import physical_plan as P
    from datafusion_amd.expr import col
    leaf = P.MemoryExec(StubTable(1000, SCHEMA), "t")
    for mode in ("Partial", "Final", "FinalPartitioned", "PartialReduce"):
        why = P.unsupported_reason(P.AggregateExec(mode, [], [("median", col("w"), "c")], leaf))
        assert why == f"MEDIAN (aggregate c) is not supported in mode {mode} on the GPU path: its partial state is a List column"
    assert P.unsupported_reason(P.AggregateExec("Single", [], [("median", None, "c")], leaf)) == "MEDIAN (aggregate c) needs an argument"
    for mode in ("Single", "SinglePartitioned"):
        assert P.unsupported_reason(P.AggregateExec(mode, [(col("r"), "r")], [("median", col("w"), "c", col("p"))], leaf)) is None, mode
    # the library says the same: the words are in its source (tests/test_zzzzzzz_gpu_agg_median.py asks the library itself)
    src = open(os.path.join(ROOT, "datafusion_amd", "csrc", "aggregate.hip")).read()
    for words in ('"MEDIAN over Boolean is not supported on the GPU path"', '"MEDIAN over Utf8 is not supported on the GPU path"',
                  '"MEDIAN over " + type_name(v.field) + " is not supported on the GPU path"', '" needs an argument"',
                  '" on the GPU path: its partial state is a List column"', '"MEDIAN keeps the rows of every group"'):
        assert words in src, words


def test_the_type_refusals_of_the_plan_layer(monkeypatch):
    """typing an argument goes through the library and a device; here the two calls are stood in for by the stub table's schema, so that
    what unsupported_reason DOES with an argument's type is asked without either"""
    from datafusion_amd import physical_plan as P
    from datafusion_amd.expr import col
    class Typed:                                                                 # what stands in for the empty device table
        def __init__(self, table):
            self.schema = table.schema

        def free(self):
            pass
    monkeypatch.setattr(P.DeviceTable, "from_arrow", staticmethod(Typed))
    monkeypatch.setattr(P.ops, "expr_type", lambda empty, e: empty.schema.field(e.name).type)
    leaf = P.MemoryExec(StubTable(1000, SCHEMA), "t")
    for c, name in (("d", "Date32"), ("p", "Boolean"), ("s", "Utf8"), ("ds", "Utf8")):
        for mode in ("Single", "SinglePartitioned"):
            why = P.unsupported_reason(P.AggregateExec(mode, [(col("r"), "r")], [("sum", col("a"), "x"), ("median", col(c), "c")], leaf))
            assert why == f"MEDIAN over {name} is not supported on the GPU path", (c, why)
    for c in ("r", "a", "w", "u", "m", "b"):
        assert P.unsupported_reason(P.AggregateExec("Single", [(col("r"), "r")], [("median", col(c), "c", col("p"))], leaf)) is None, c
    # a filter that is not Boolean is still said first, and the rule keeps a staged pair over a refused type as it was
    assert "not Boolean" in P.unsupported_reason(P.AggregateExec("Single", [], [("median", col("w"), "c", col("a"))], leaf))
    partial = P.AggregateExec("Partial", [(col("r"), "r")], [("median", col("d"), "m")], leaf)
    rule = P.GpuOffloadRule()
    out = rule.optimize(P.AggregateExec("FinalPartitioned", [(col("r"), "r")], [("median", col("m"), "m")], P.RepartitionExec(partial, ["r"], 4)))
    below = P._partial_below(out.input)
    assert out.mode == "FinalPartitioned" and getattr(out, "kept_on_cpu", False) and below.mode == "Partial" and getattr(below, "kept_on_cpu", False)
    assert rule.declined[0] == (out, "MEDIAN over Date32 is not supported on the GPU path")
    # the DISTINCT aggregates see a dictionary-encoded argument through the same helper
    assert P.unsupported_reason(P.AggregateExec("Single", [], [("sum_distinct", col("ds"), "c")], leaf)) == "SUM(DISTINCT) over Utf8 is not supported on the GPU path"
    assert P.unsupported_reason(P.AggregateExec("Single", [], [("count_distinct", col("ds"), "c")], leaf)) is None


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


def _q6_aggs():
    from datafusion_amd.expr import col
    return [("median", col("w"), "med"), ("stddev", col("w"), "sd"), ("median", col("au"), "mf", col("p"))]


def test_one_rank_collapses_final_over_partial_into_one_single_node():
    from datafusion_amd import physical_plan as P
    plan, partial, leaf, rule = _staged(P, _q6_aggs())
    out = rule.optimize(plan)
    assert type(out) is P.GpuFusedAggregateExec and out.mode == "Single" and out.input is leaf and not rule.declined
    got = ops.normalize_aggs(out.aggr_expr)
    assert [(f, n) for f, _, n, _ in got] == [("median", "out_med"), ("stddev", "out_sd"), ("median", "out_mf")]
    assert repr(got[0][1]) == "w@None" and repr(got[2][1]) == "(a@None + u@None)" and repr(got[2][3]) == "p@None" and got[0][3] is None
    assert repr(out.predicate) == "(a@None > 3:int64)" and not getattr(out, "kept_on_cpu", False)
    plan, partial, leaf, rule = _staged(P, _q6_aggs()[:2], final="Final", below_filter=False)
    out = rule.optimize(plan)
    assert type(out) is P.AggregateExec and out.mode == "Single" and out.input is leaf and not rule.declined
    assert P.displayable(out).split("\n")[0] == "AggregateExec: mode=Single, gby=[r_out], aggr=[out_med, out_sd]"


def test_two_ranks_keep_both_nodes_and_say_why():
    from datafusion_amd import physical_plan as P
    plan, partial, leaf, rule = _staged(P, _q6_aggs(), world=2)
    out = rule.optimize(plan)
    assert type(out) is P.AggregateExec and out.mode == "FinalPartitioned" and getattr(out, "kept_on_cpu", False)
    below = P._partial_below(out.input)
    assert type(below) is P.AggregateExec and below.mode == "Partial" and getattr(below, "kept_on_cpu", False)
    assert {node.mode: why for node, why in rule.declined} == {
        "Partial": "MEDIAN (aggregate med) is not supported in mode Partial on the GPU path: its partial state is a List column",
        "FinalPartitioned": "MEDIAN (aggregate out_med) is not supported in mode FinalPartitioned on the GPU path: its partial state is a List column"}


def test_the_collapse_declines_where_it_must():
    from datafusion_amd import physical_plan as P
    from datafusion_amd.expr import col
    leaf = P.MemoryExec(StubTable(1000, SCHEMA), "t")
    rule = P.GpuOffloadRule()
    # a Partial that no Final consumes
    out = rule.optimize(P.CoalesceBatchesExec(P.AggregateExec("Partial", [(col("r"), "r")], [("median", col("w"), "m")], leaf)))
    assert type(out) is P.AggregateExec and out.mode == "Partial" and getattr(out, "kept_on_cpu", False)
    assert rule.declined == [(out, "MEDIAN (aggregate m) is not supported in mode Partial on the GPU path: its partial state is a List column")]
    # a node with meaning between the two
    for between in (lambda x: P.SortExec([("r", False, False)], x, fetch=10), lambda x: P.FilterExec(col("r") > col("r"), x)):
        partial = P.AggregateExec("Partial", [(col("r"), "r")], [("median", col("w"), "m")], leaf)
        plan = P.AggregateExec("FinalPartitioned", [(col("r"), "r")], [("median", col("m"), "m")], P.RepartitionExec(between(partial), ["r"], 4))
        rule = P.GpuOffloadRule()
        out = rule.optimize(plan)
        assert type(out) is P.AggregateExec and out.mode == "FinalPartitioned" and getattr(out, "kept_on_cpu", False)
        assert type(out.input) in (P.SortExec, P.FilterExec)
        below = P._partial_below(out.input)
        assert below.mode == "Partial" and getattr(below, "kept_on_cpu", False)
        assert sorted(n.mode for n, _ in rule.declined) == ["FinalPartitioned", "Partial"] and all("List column" in why for _, why in rule.declined)
    # and a plan without a MEDIAN is rewritten as before
    plan, _, leaf, rule = _staged(P, _q6_aggs()[1:2])
    out = rule.optimize(plan)
    assert out.mode == "FinalPartitioned" and not rule.declined and type(out.input) is P.GpuFusedAggregateExec and out.input.mode == "Partial"
