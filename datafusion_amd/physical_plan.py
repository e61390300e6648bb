"""Host-side mirror of the reference's operator / plugin surface for the hot path.

The reference plugs new operators in through two traits: `ExecutionPlan`
(physical-plan/src/execution_plan.rs:102 — `name` :110, `children` :268, `with_new_children` :435,
`execute(partition, ctx)` :696-700) and `PhysicalOptimizerRule`
(session/src/physical_optimizer.rs:52-84 — `optimize`, `name`, `schema_check`).  Rust cannot be compiled in
this image (INTEGRATION.md shows the shim a maintainer adds), so this module is the same surface in Python
over the same C ABI: plan nodes carry the reference's names and constructor arguments, `GpuOffloadRule.optimize`
rewrites a reference-shaped physical plan bottom-up exactly as the Rust rule would, and `execute()` runs the
node on device tables.  Parity tests build the plans pinned in the reference's own plan files
(sqllogictest/test_files/tpch/plans/q1.slt.part:50-58, q3.slt.part:61-76) node for node.

What the rule substitutes (everything else is left as it is — on the CPU in the Rust shim, here the plain
per-operator GPU node):
  AggregateExec(ProjectionExec?(FilterExec?(x)))    -> GpuFusedAggregateExec   one pass, dfgpu_agg_update_filtered
  HashJoinExec(build, FilterExec(probe))             -> GpuHashJoinExec         predicate applied inside the probe kernel
  CoalesceBatchesExec / CoalescePartitionsExec       -> removed                 (whole partitions per launch)
  RepartitionExec(Hash) on one GPU                   -> removed                 (one partition per GPU)
  SortPreservingMergeExec on one GPU                 -> removed                 (one sorted partition is the merge)
WindowAggExec stays the node it is (dfgpu_window); the rule demands order of its child, so the SortExec below keeps its meaning.
NestedLoopJoinExec / CrossJoinExec stay the nodes they are (dfgpu_nested_loop_join); only their right child inherits the parent's need of order.
With GpuOffloadRule(range_joins=True) a NestedLoopJoinExec over a range condition becomes a GpuRangeJoinExec (dfgpu_range_join).
"""
from __future__ import annotations

from . import _lib, ops
from .expr import BinaryExpr, CaseExpr, CastExpr, Column, DatePartExpr, InListExpr, IsNotNullExpr, IsNullExpr, LikeExpr, Literal, NotExpr, PhysicalExpr, SubstrExpr
from .table import DeviceTable


# --------------------------------------------------------------------------- expression helpers
def substitute(e: PhysicalExpr, mapping: dict) -> PhysicalExpr:
    """replace Column references by the expressions a ProjectionExec computed them from (projection.rs:713-746
    `update_expr`: how the reference pushes expressions through projections)"""
    if isinstance(e, Column):
        return mapping.get(e.name, e)
    if isinstance(e, Literal):
        return e
    if isinstance(e, CastExpr):
        return CastExpr(substitute(e.expr, mapping), e.cast_type)
    if isinstance(e, BinaryExpr):
        return BinaryExpr(substitute(e.left, mapping), e.op, substitute(e.right, mapping))
    if isinstance(e, IsNullExpr):
        return IsNullExpr(substitute(e.arg, mapping))
    if isinstance(e, IsNotNullExpr):
        return IsNotNullExpr(substitute(e.arg, mapping))
    if isinstance(e, NotExpr):
        return NotExpr(substitute(e.arg, mapping))
    if isinstance(e, (CaseExpr, InListExpr, DatePartExpr, SubstrExpr)):
        return e.map_children(lambda x: substitute(x, mapping))
    if isinstance(e, LikeExpr):
        return LikeExpr(substitute(e.expr, mapping), e.pattern, e.negated, e.case_insensitive)
    raise TypeError(f"unsupported expression node {type(e).__name__}")


def columns_of(e: PhysicalExpr, out=None) -> set:
    out = set() if out is None else out
    if isinstance(e, Column):
        out.add(e.name)
    for c in e.children():
        columns_of(c, out)
    return out


# --------------------------------------------------------------------------------- plan nodes
class ExecutionPlan:
    """execution_plan.rs:102.  `execute` returns the node's whole output partition as a device table
    (the pull-stream contract lives at the Rust boundary only)."""

    def name(self) -> str:
        return type(self).__name__

    def children(self) -> list:
        return []

    def with_new_children(self, children: list) -> "ExecutionPlan":
        raise NotImplementedError

    def execute(self, partition: int = 0) -> DeviceTable:
        raise NotImplementedError

    def detail(self) -> str:
        return ""

    def _run_child(self, child: "ExecutionPlan"):
        """(table, owned): leaf tables belong to the caller and are never freed by a plan"""
        t = child.execute()
        return t, not isinstance(child, MemoryExec)

    def _pass_through(self, child: "ExecutionPlan") -> DeviceTable:
        """output = the child's output; a leaf's table is handed on as a zero-copy view the parent may free"""
        t, owned = self._run_child(child)
        return t if owned else t.select(list(range(t.num_columns)))


class MemoryExec(ExecutionPlan):
    """DataSourceExec over an in-memory table (datasource/src/memory.rs:58) — here: a device-resident table.
    `projection` = the scan's column projection (DataSourceExec: projection=[...]); a zero-copy view."""

    def __init__(self, table: DeviceTable, name: str = "", projection=None):
        self.table, self.label, self.projection = table, name, projection
        self._view = None

    def project(self, columns) -> "MemoryExec":
        return MemoryExec(self.table, self.label, list(columns))

    def with_new_children(self, children):
        return self

    def execute(self, partition=0):
        if self.projection is None:
            return self.table
        if self._view is None:
            self._view = self.table.select(self.projection)     # owned by this node, like the table by the caller
        return self._view

    def detail(self):
        return f"{self.label} rows={self.table.num_rows}" + (f", projection={self.projection}" if self.projection else "")


class ParquetExec(ExecutionPlan):
    """DataSourceExec over a ParquetSource (datasource/src/source.rs:366, datasource-parquet) with the scan's column
    projection — here the GPU scan: every projected column chunk is decoded on the device (parquet.ParquetFile.read,
    dfgpu_parquet_decode_chunk).  The decoded table is owned by the node's consumer."""

    def __init__(self, path: str, projection=None, name: str = ""):
        self.path, self.projection, self.label = path, projection, name
        self.dynamic_bounds = {}   # column -> (lo, hi): published by a HashJoinExec above once its build side is known
        self.dynamic_in_lists = {} # column -> ascending distinct build keys of a small build side (PushdownStrategy::InList)
        self.dynamic_membership = {}  # column -> the built join table of a LARGE build side (PushdownStrategy::Map): asked `contains` per row group
        self.metrics = {}          # row_groups_total / row_groups_read of the last execute

    def project(self, columns) -> "ParquetExec":
        return ParquetExec(self.path, list(columns), self.label)

    def with_new_children(self, children):
        return self

    def execute(self, partition=0):
        from .parquet import read_table
        return read_table(self.path, self.projection, bounds=self.dynamic_bounds or None, stats=self.metrics, in_lists=self.dynamic_in_lists or None,
                          membership={k: v for k, v in self.dynamic_membership.items() if v is not None} or None)

    def detail(self):
        return f"{self.label or self.path}" + (f", projection={self.projection}" if self.projection else "")


class ArrowIpcExec(ExecutionPlan):
    """DataSourceExec over an ArrowSource (datasource-arrow/src/source.rs:260): an Arrow IPC file or stream scanned straight into
    HBM (ipc.read_table: no decoding, one H2D copy per buffer, batches concatenated on the device)"""

    def __init__(self, path: str, projection=None, name: str = ""):
        self.path, self.projection, self.label = path, projection, name
        self.metrics = {}

    def project(self, columns) -> "ArrowIpcExec":
        return ArrowIpcExec(self.path, list(columns), self.label)

    def children(self):
        return []

    def with_new_children(self, children):
        return self

    def execute(self, partition=0):
        from .ipc import read_table
        return read_table(self.path, self.projection, stats=self.metrics)

    def detail(self):
        return f"{self.label or self.path}" + (f", projection={self.projection}" if self.projection else "")


class _Unary(ExecutionPlan):
    def children(self):
        return [self.input]


class FilterExec(_Unary):
    """FilterExec::try_new(predicate, input) with an optional embedded projection (filter.rs:85)"""

    def __init__(self, predicate: PhysicalExpr, input: ExecutionPlan, projection=None):
        self.predicate, self.input, self.projection = predicate, input, projection

    def with_new_children(self, c):
        return FilterExec(self.predicate, c[0], self.projection)

    def execute(self, partition=0):
        t, owned = self._run_child(self.input)
        out = ops.filter(t, self.predicate, self.projection)
        if owned:
            t.free()
        return out

    def detail(self):
        return f"{self.predicate!r}" + (f", projection={self.projection}" if self.projection else "")


class ProjectionExec(_Unary):
    """ProjectionExec::try_new(exprs = [(expr, name)], input) (projection.rs:439)"""

    def __init__(self, exprs, input: ExecutionPlan):
        self.exprs, self.input = exprs, input

    def with_new_children(self, c):
        return ProjectionExec(self.exprs, c[0])

    def execute(self, partition=0):
        t, owned = self._run_child(self.input)
        out = ops.project(t, self.exprs)
        if owned:
            t.free()
        return out

    def detail(self):
        return ", ".join(f"{e!r} as {n}" for e, n in self.exprs)


class CoalesceBatchesExec(_Unary):
    """coalesce/mod.rs:63 — batch-size bookkeeping; a device partition is already one batch"""

    def __init__(self, input: ExecutionPlan, target_batch_size: int = 8192):
        self.input, self.target_batch_size = input, target_batch_size

    def with_new_children(self, c):
        return CoalesceBatchesExec(c[0], self.target_batch_size)

    def execute(self, partition=0):
        return self._pass_through(self.input)


class RepartitionExec(_Unary):
    """RepartitionExec::try_new(input, Partitioning::Hash(keys, n)) (repartition/mod.rs:1626).  One process per
    GPU: the exchange is RCCL (exchange.hash_exchange); with a single GPU there is one partition and nothing moves."""

    def __init__(self, input: ExecutionPlan, keys, n_partitions: int, group=None):
        self.input, self.keys, self.n_partitions, self.group = input, keys, n_partitions, group

    def with_new_children(self, c):
        return RepartitionExec(c[0], self.keys, self.n_partitions, self.group)

    def execute(self, partition=0):
        from .queries import _repartition, _world
        if _world(self.group) == 1:
            return self._pass_through(self.input)
        t, owned = self._run_child(self.input)
        out = _repartition(t, self.keys, self.group)
        if owned:
            t.free()
        return out

    def detail(self):
        return f"Hash({self.keys}, {self.n_partitions})"


class CoalescePartitionsExec(_Unary):
    """CoalescePartitionsExec::new(input) (coalesce_partitions.rs:50): all input partitions into one, in arrival
    order.  One partition per GPU: with one GPU nothing happens, with several every rank receives the
    concatenation of the ranks' partitions in rank order — a device all-gather (dfgpu_exchange_broadcast)."""

    def __init__(self, input: ExecutionPlan, group=None):
        self.input, self.group = input, group

    def with_new_children(self, c):
        return CoalescePartitionsExec(c[0], self.group)

    def execute(self, partition=0):
        from .queries import _world
        if _world(self.group) == 1:
            return self._pass_through(self.input)
        from .exchange import broadcast_table
        t, owned = self._run_child(self.input)
        out = broadcast_table(t, self.group)
        if owned and out is not t:
            t.free()
        return out


class SortPreservingMergeExec(_Unary):
    """SortPreservingMergeExec::new(expr, input).with_fetch(fetch) (sorts/sort_preserving_merge.rs:91): k-way merge
    of the sorted partitions.  One partition per GPU: a no-op on one GPU, otherwise queries._merge_sorted."""

    def __init__(self, expr, input: ExecutionPlan, fetch=None, group=None):
        self.expr, self.input, self.fetch, self.group = expr, input, fetch, group

    def with_new_children(self, c):
        return SortPreservingMergeExec(self.expr, c[0], self.fetch, self.group)

    def execute(self, partition=0):
        from .queries import _merge_sorted, _world
        if _world(self.group) == 1:
            return self._pass_through(self.input)
        t, owned = self._run_child(self.input)
        out = _merge_sorted(t, self.expr, self.fetch, self.group)
        if owned and out is not t:
            t.free()
        return out

    def detail(self):
        return str([(c, "DESC" if d else "ASC") for c, d, _ in self.expr]) + (f", fetch={self.fetch}" if self.fetch is not None else "")


class HashJoinExec(ExecutionPlan):
    """HashJoinExec::try_new(left = build, right = probe, on, filter = None, join_type, projection, mode,
    null_equality, null_aware) (joins/hash_join/exec.rs:752).  `projection` = (build columns, probe columns);
    `null_aware` = NOT IN semantics for LeftAnti / RightAnti on one key column (exec.rs:429-455)."""

    def __init__(self, left: ExecutionPlan, right: ExecutionPlan, on, join_type="Inner", projection=None, null_equality="NullEqualsNothing",
                 probe_mode=0, filter=None, null_aware=False):
        self.left, self.right, self.on, self.join_type = left, right, on, join_type
        self.projection, self.null_equality, self.probe_mode = projection, null_equality, probe_mode
        self.filter = filter   # JoinFilter: (expression over f0, f1, ..., [(column index, "Left" | "Right"), ...])
        self.null_aware = null_aware

    def children(self):
        return [self.left, self.right]

    def with_new_children(self, c):
        return HashJoinExec(c[0], c[1], self.on, self.join_type, self.projection, self.null_equality, self.probe_mode, self.filter, self.null_aware)

    # probe rows without a build match are dropped by these join types (JoinType::on_lr_is_preserved, common/src/join_type.rs:115-127:
    # the probe side accepts a pushed-down filter), so the build side's key bounds may prune the probe-side scan
    _DYNAMIC_FILTER_JOINS = ("Inner", "Left", "LeftSemi", "RightSemi", "LeftAnti", "LeftMark")
    _BUILD_EMITTING = ("Left", "Full", "LeftSemi", "LeftAnti", "LeftMark")      # join types that report build rows by their visited marks

    def _publish_membership(self, ht):
        """the Map strategy (hash_join/exec.rs:2727-2751: a build side beyond the IN-list limits pushes the hash table itself):
        the probe-side ParquetExec asks the built table `contains` for every row group's key chunk before it reads anything else.
        Only where the bounds were published (same join types / key restrictions) and no IN list was (that is the small-build case)."""
        node = self.right
        while isinstance(node, (FilterExec, CoalesceBatchesExec, RepartitionExec)):
            node = node.input
        if not isinstance(node, ParquetExec):
            return None
        probe_key = self.on[0][1]
        from .queries import _world
        if probe_key in node.dynamic_bounds and probe_key not in node.dynamic_in_lists and _world() == 1 and self.filter is None:
            node.dynamic_membership[probe_key] = ht
            return node, probe_key        # the caller withdraws the entry before it frees the table (the scan does not own it)
        node.dynamic_membership.pop(probe_key, None)
        return None

    def _publish_dynamic_bounds(self, build_table):
        """the join's dynamic filter (HashJoinExec::create_dynamic_filter, hash_join/exec.rs:869-875; bounds accumulated in
        hash_join/shared_bounds.rs:277-284): [min, max] of the build keys, handed to the probe-side scan, which prunes row groups
        with it before reading them.  Single integer key, no JoinFilter-independent restrictions of the reference apply here
        (one partition); a null-aware anti join never publishes (exec.rs:883-892)."""
        if self.join_type not in self._DYNAMIC_FILTER_JOINS or len(self.on) != 1 or self.null_aware or self.null_equality != "NullEqualsNothing":
            return
        node = self.right
        while isinstance(node, (FilterExec, CoalesceBatchesExec, RepartitionExec)):
            node = node.input
        if not isinstance(node, ParquetExec):
            return
        build_key, probe_key = self.on[0]
        if node.projection is not None and probe_key not in node.projection:
            return
        import pyarrow as pa
        ktype = build_table.schema.field(build_table.index_of(build_key)).type
        if ktype not in (pa.int64(), pa.int32()):
            return
        lo, hi, n, _ = ops.column_minmax(build_table, build_key)
        from .queries import _world
        if _world() > 1:
            # one process per GPU: this rank's build partition holds only the keys routed to it, while its probe-side scan still
            # holds rows bound for every rank — the filter must cover ALL partitions' build keys, as the reference's shared
            # accumulator waits for every partition before it updates the filter (hash_join/shared_bounds.rs: SharedBuildAccumulator)
            import torch.distributed as dist
            parts = [None] * dist.get_world_size()
            dist.all_gather_object(parts, (lo, hi, n))
            seen = [(a, b) for a, b, c in parts if c]
            n = len(seen)
            if n:
                lo, hi = min(a for a, _ in seen), max(b for _, b in seen)
        node.dynamic_bounds[probe_key] = (lo, hi) if n else (1, 0)     # an empty build side prunes the whole scan
        if _world() == 1:
            # the membership half (PushdownStrategy::InList for small build sides, else Map = bounds only); with several ranks the
            # lists of all partitions would have to be merged like the bounds — they stay on bounds
            values = ops.column_inlist(build_table, build_key)
            if values is not None:
                node.dynamic_in_lists[probe_key] = values
            else:
                node.dynamic_in_lists.pop(probe_key, None)     # a larger build side this time (Map strategy): a list of an earlier run must not prune

    def _probe(self, ht, probe_table, predicate=None):
        bc, pc = self.projection if self.projection else (None, None)
        return ht.probe(probe_table, [r for _, r in self.on], self.join_type, bc, pc, predicate=predicate, join_filter=self.filter)

    def execute(self, partition=0, probe_predicate=None):
        if self.filter is not None or self.join_type not in ("Inner", "RightSemi", "RightAnti", "Right", "RightMark"):
            # build-side emission (Left / Full / LeftSemi / LeftAnti / LeftMark): the general path of ops.hash_join
            assert probe_predicate is None
            b, bo = self._run_child(self.left)
            self._publish_dynamic_bounds(b)
            p, po = self._run_child(self.right)
            bc, pc = self.projection if self.projection else (None, None)
            shared_build = self.join_type in self._BUILD_EMITTING and replicated_build(self.left)
            if shared_build:
                # PartitionMode::CollectLeft with build-side emission: the reference's probe partitions mark ONE shared visited bitmap
                # and the last of them reports the build rows (hash_join/exec.rs:1312-1330, stream.rs ProcessUnmatchedBuild).  Here the
                # probe partitions sit on different GPUs and the build side is replicated: every rank probes ITS probe rows, the copies'
                # visited marks (and null-aware flags) are OR-ed across the ranks (dfgpu_exchange_join_visited), and the build rows the
                # marks select — the same on every rank, in build-row order — are split by position.  Nothing is computed twice, and
                # no rank depends on the order another rank's atomics built its chains in.
                import torch.distributed as dist

                from .exchange import comm_for
                ht = ops.JoinHashTable(b, [l for l, _ in self.on], self.null_equality, null_aware=self.null_aware)
                matched = ht.probe(p, [r for _, r in self.on], self.join_type, bc, pc, join_filter=self.filter)
                comm_for().merge_join_visited(ht)
                tail = ht.emit_unmatched(self.join_type, bc, ops.tail_probe_schema(p, self.join_type, pc))
                n, world, rank = tail.num_rows, dist.get_world_size(), dist.get_rank()
                mine = tail.slice(n * rank // world, n * (rank + 1) // world - n * rank // world)
                tail.free()
                if self.join_type in ("Left", "Full"):
                    out = ops.concat_tables([matched, mine])
                    mine.free()
                else:
                    out = mine
                matched.free()
                ht.free()
            else:
                out = ops.hash_join(b, p, self.on, self.join_type, self.null_equality, bc, pc, join_filter=self.filter, null_aware=self.null_aware)
            for t, o in ((b, bo), (p, po)):
                if o:
                    t.free()
            return out
        b, bo = self._run_child(self.left)
        ht = ops.JoinHashTable(b, [l for l, _ in self.on], self.null_equality, probe_mode=self.probe_mode, null_aware=self.null_aware)
        self._publish_dynamic_bounds(b)
        published = self._publish_membership(ht) if self.join_type in ("Inner", "RightSemi") and len(self.on) == 1 else None
        try:
            p, po = self._run_child(self.right)
        finally:
            # the membership entry is the live join table: it is withdrawn (the key stays, as a record that a table was pushed; the
            # scan skips entries without a table) once the probe child has run — a later execution of that scan, on its own or
            # through a re-used node, must not ask a freed table
            if published is not None and published[1] in published[0].dynamic_membership:
                published[0].dynamic_membership[published[1]] = None
        out = self._probe(ht, p, probe_predicate)
        ht.free()
        for t, o in ((b, bo), (p, po)):
            if o:
                t.free()
        return out

    def detail(self):
        return f"join_type={self.join_type}, on={self.on}" + (f", projection={self.projection}" if self.projection else "") + \
            (", null_aware" if self.null_aware else "")


class NestedLoopJoinExec(ExecutionPlan):
    """NestedLoopJoinExec::try_new(left = the collected side, right = the probe side, filter, join_type, projection)
    (joins/nested_loop_join.rs): the join of a condition without an equality.  `filter` = JoinFilter as in HashJoinExec (expression over
    f0, f1, ..., [(column index, "Left" | "Right"), ...]); None = every pair matches.  `projection` = (left columns, right columns).
    Output order: ops.nested_loop_join's (the filtered hash join's)."""

    def __init__(self, left: ExecutionPlan, right: ExecutionPlan, filter=None, join_type="Inner", projection=None):
        if join_type not in ops.JOIN_TYPES:
            raise ValueError(f"unknown join type {join_type!r}")
        self.left, self.right, self.filter, self.join_type, self.projection = left, right, filter, join_type, projection

    def children(self):
        return [self.left, self.right]

    def with_new_children(self, c):
        return NestedLoopJoinExec(c[0], c[1], self.filter, self.join_type, self.projection)

    def execute(self, partition=0):
        l, lo = self._run_child(self.left)
        r, ro = self._run_child(self.right)
        lc, rc = self.projection if self.projection else (None, None)
        try:
            return ops.nested_loop_join(l, r, self.join_type, self.filter, lc, rc)
        finally:
            for t, o in ((l, lo), (r, ro)):
                if o:
                    t.free()

    def detail(self):
        return f"join_type={self.join_type}" + (f", filter={self.filter[0]!r}" if self.filter is not None else "") + \
            (f", projection={self.projection}" if self.projection else "")


class CrossJoinExec(NestedLoopJoinExec):
    """CrossJoinExec::new(left, right) (joins/cross_join.rs): every pair — the inner nested-loop join without a filter"""

    def __init__(self, left: ExecutionPlan, right: ExecutionPlan):
        super().__init__(left, right, None, "Inner", None)

    def with_new_children(self, c):
        return CrossJoinExec(c[0], c[1])

    def detail(self):
        return ""


RANGE_JOIN_NO_BOUND = "a range join needs a lower or an upper bound"
RANGE_JOIN_DICT_KEY = "a range join key that is dictionary-encoded is not supported on the GPU path"
RANGE_JOIN_KEY_TYPE = "a range join key of a type other than Int32, Int64, Date32, UInt32, UInt64 or Float64 is not supported on the GPU path"
RANGE_JOIN_MIXED_KEYS = "a range join over keys of different types is not supported on the GPU path"


def _schema_field(schema, c):
    return schema.field(schema.get_field_index(c)) if isinstance(c, str) else schema.field(c)


class GpuRangeJoinExec(ExecutionPlan):
    """dfgpu_range_join as a plan node: the join `a <(=) x AND x <(=) b` of the left columns a, b against the right column x by sorting x
    and searching the bounds (no pair space).  `lower` = (left column a, inclusive) or None, `upper` = (left column b, inclusive) or None;
    `projection` = (left columns, right columns).  Deliberately not a NestedLoopJoinExec: the pair types come in LEFT-row-major order
    (ops.range_join), so GpuOffloadRule(range_joins=True) only puts it where that order is not observed, or for the one-sided types."""

    def __init__(self, left: ExecutionPlan, right: ExecutionPlan, x, lower=None, upper=None, join_type="Inner", projection=None):
        if join_type not in ops.JOIN_TYPES:
            raise ValueError(f"unknown join type {join_type!r}")
        self.left, self.right, self.x, self.lower, self.upper, self.join_type, self.projection = left, right, x, lower, upper, join_type, projection

    def children(self):
        return [self.left, self.right]

    def with_new_children(self, c):
        return GpuRangeJoinExec(c[0], c[1], self.x, self.lower, self.upper, self.join_type, self.projection)

    def execute(self, partition=0):
        l, lo = self._run_child(self.left)
        r, ro = self._run_child(self.right)
        lc, rc = self.projection if self.projection else (None, None)
        try:
            return ops.range_join(l, r, self.x, self.lower, self.upper, self.join_type, lc, rc)
        finally:
            for t, o in ((l, lo), (r, ro)):
                if o:
                    t.free()

    def _label(self, child, c):
        """name@index of a child's column, as far as the child's schema is known at plan time"""
        try:
            sch = plan_schema(child)
            i = sch.get_field_index(c) if isinstance(c, str) else int(c)
            return f"{sch.field(i).name}@{i}"
        except Exception:  # noqa: BLE001 - no schema at plan time: what the node was given
            return f"{c}@{None if isinstance(c, str) else c}"

    def detail(self):
        x, parts = self._label(self.right, self.x), []
        if self.lower is not None:
            parts.append(f"{self._label(self.left, self.lower[0])} {'<=' if self.lower[1] else '<'} {x}")
        if self.upper is not None:
            parts.append(f"{x} {'<=' if self.upper[1] else '<'} {self._label(self.left, self.upper[0])}")
        return f"join_type={self.join_type}, " + (" AND ".join(parts) if parts else "no bound") + (f", projection={self.projection}" if self.projection else "")


def range_condition(join_filter):
    """(x, lower, upper) when the JoinFilter is one comparison (<, <=, >, >=) of a bare left column with a bare right column, or an AND of
    two that name the same right column and give at most one lower and one upper bound on it: x = the right column's index, lower /
    upper = (left column index, inclusive) or None.  None for every other filter."""
    if join_filter is None:
        return None
    fexpr, fcols = join_filter
    comps = [fexpr.left, fexpr.right] if isinstance(fexpr, BinaryExpr) and fexpr.op == "and" else [fexpr]
    flipped = {"<": ">", "<=": ">=", ">": "<", ">=": "<="}

    def slot(c):
        if type(c) is not Column:
            return None
        k = c.index if c.index is not None else (int(c.name[1:]) if c.name[:1] == "f" and c.name[1:].isdigit() else None)
        return k if k is not None and 0 <= k < len(fcols) else None

    x, lower, upper = None, None, None
    for c in comps:
        if not isinstance(c, BinaryExpr) or c.op not in flipped:
            return None
        a, b = slot(c.left), slot(c.right)
        if a is None or b is None or fcols[a][1] == fcols[b][1]:
            return None
        op = c.op
        if fcols[a][1] == "Right":           # x op a  is  a flipped(op) x
            a, b, op = b, a, flipped[op]
        li, ri = int(fcols[a][0]), int(fcols[b][0])
        if x is not None and ri != x:
            return None
        x = ri
        if op in ("<", "<="):                # a <(=) x
            if lower is not None:
                return None
            lower = (li, op == "<=")
        else:                                # a >(=) x  is  x <(=) a
            if upper is not None:
                return None
            upper = (li, op == ">=")
    return x, lower, upper


def replicated_build(node: ExecutionPlan) -> bool:
    """several ranks and the build side is a CoalescePartitionsExec (every rank holds ALL build rows: PartitionMode::CollectLeft)"""
    from .queries import _world
    if _world() == 1:
        return False
    while isinstance(node, CoalesceBatchesExec):
        node = node.input
    return isinstance(node, CoalescePartitionsExec)


def _partial_below(node: ExecutionPlan, through=None):
    """the Partial aggregate feeding a Final one, through the exchange / bookkeeping nodes between them (`through`: the node types
    that may lie between, None = any node with one child)"""
    while node is not None:
        if isinstance(node, (AggregateExec, GpuFusedAggregateExec)):
            return node if node.mode == "Partial" else None
        if through is not None and not isinstance(node, through):
            return None
        kids = node.children()
        node = kids[0] if len(kids) == 1 else None
    return None


_EXCHANGE_NODES = (RepartitionExec, CoalesceBatchesExec, CoalescePartitionsExec, SortPreservingMergeExec)


def _has_distinct(node) -> bool:
    """has an aggregate without a device partial state: a DISTINCT aggregate or a MEDIAN (the reference's state is a List column)"""
    return any(f in ops.NO_PARTIAL_STATE_FUNCS for f, _, _, _ in ops.normalize_aggs(node.aggr_expr))


def _aggr_detail(aggr_expr):
    """the aggregates of a node's detail(): their names, a filtered one as `name FILTER (WHERE <filter>)`"""
    return ", ".join(n if flt is None else f"{n} FILTER (WHERE {flt!r})" for _, _, n, flt in ops.normalize_aggs(aggr_expr))


class AggregateExec(_Unary):
    """AggregateExec::try_new(mode, group_by = [(expr, name)], aggr_expr = [(func, arg | None, name)], input)
    (aggregates/mod.rs:839).  An aggregate with a FILTER (WHERE ...) is (func, arg | None, name, filter): AggregateExec::filter_expr,
    a Boolean PhysicalExpr over the input, or None.  `aggr_expr` is kept as it was given; ops.normalize_aggs gives the 4-tuples."""

    def __init__(self, mode: str, group_by, aggr_expr, input: ExecutionPlan):
        self.mode, self.group_by, self.aggr_expr, self.input = mode, group_by, aggr_expr, input
        self.return_types = None    # Partial: the aggregates' declared return types, typed over the raw input when it runs

    def with_new_children(self, c):
        return AggregateExec(self.mode, self.group_by, self.aggr_expr, c[0])

    def execute(self, partition=0):
        t, owned = self._run_child(self.input)
        rt = None
        if self.mode == "Partial":
            self.return_types = ops.aggregate_return_types(t, self.aggr_expr)
        elif self.mode in ("Final", "FinalPartitioned"):
            # AggregateFunctionExpr::return_field: the reference's Final node carries the types its Partial twin was planned with
            below = _partial_below(self.input)
            rt = below.return_types if below is not None else None
        out = ops.aggregate(t, self.group_by, self.aggr_expr, self.mode, return_types=rt)
        if owned:
            t.free()
        return out

    def detail(self):
        return f"mode={self.mode}, gby=[{', '.join(n for _, n in self.group_by)}], aggr=[{_aggr_detail(self.aggr_expr)}]"


class SortExec(_Unary):
    """SortExec::new(expr = [(column, descending, nulls_first)], input).with_fetch(fetch) (sorts/sort.rs:1366);
    with fetch it is the reference's TopK (topk/mod.rs:397)"""

    def __init__(self, expr, input: ExecutionPlan, fetch=None):
        self.expr, self.input, self.fetch = expr, input, fetch

    def with_new_children(self, c):
        return SortExec(self.expr, c[0], self.fetch)

    def execute(self, partition=0):
        t, owned = self._run_child(self.input)
        out = ops.sort(t, self.expr, self.fetch)
        if owned:
            t.free()
        return out

    def detail(self):
        return ("TopK(fetch=%d), " % self.fetch if self.fetch is not None else "") + str([(c, "DESC" if d else "ASC") for c, d, _ in self.expr])


class WindowAggExec(_Unary):
    """WindowAggExec / BoundedWindowAggExec (physical-plan/src/windows/): window_expr = [(func, arg | None, name, frame)] — func one of
    ops.WINDOW_FUNCS, ops.WINDOW_DIST_FUNCS or ops.WINDOW_VALUE_FUNCS (("ntile", n) and ("nth_value", n) carry their integer), frame
    one of ops.WINDOW_FRAMES (None = range_to_current, the default under an ORDER BY) — over
    PARTITION BY partition_by ORDER BY order_by.  partition_by = columns; order_by = columns or (column, descending, nulls_first) as
    SortExec takes them: direction and NULL placement are kept for display only, the operator looks at equality of neighbouring rows.
    The input must arrive ordered by (partition_by, order_by) — the SortExec the planner puts below; the two reference nodes differ
    in streaming, not in results, and this node is both."""

    def __init__(self, window_expr, partition_by, order_by, input: ExecutionPlan):
        self.window_expr, self.partition_by, self.input = window_expr, list(partition_by or []), input
        self.order_by = [o if isinstance(o, tuple) else (o, False, False) for o in (order_by or [])]

    def with_new_children(self, c):
        return WindowAggExec(self.window_expr, self.partition_by, self.order_by, c[0])

    def execute(self, partition=0):
        t, owned = self._run_child(self.input)
        out = ops.window(t, self.partition_by, [c for c, _, _ in self.order_by], self.window_expr)
        if owned:
            t.free()      # (the output's input columns hold their buffers themselves)
        return out

    def detail(self):
        def one(func, arg, name, frame):
            func, param = func if isinstance(func, tuple) else (func, None)
            over = "" if func in ops.WINDOW_RANKING or func in ops.WINDOW_DIST_FUNCS else f" {frame}"
            inside = ", ".join(([] if arg is None else [repr(arg)]) + ([] if param is None else [str(param)]))
            return f"{func}({inside}){over} AS {name}"
        order = ", ".join(f"{c} {'DESC' if d else 'ASC'} NULLS {'FIRST' if nf else 'LAST'}" for c, d, nf in self.order_by)
        return (f"wdw=[{', '.join(one(*w) for w in ops.normalize_window_exprs(self.window_expr))}], "
                f"partition_by=[{', '.join(str(c) for c in self.partition_by)}], order_by=[{order}]")


# ------------------------------------------------------------------------------ fused GPU nodes
class ScalarSubqueryExec(ExecutionPlan):
    """physical-plan/src/scalar_subquery.rs:85 — a pass-through over its main input that first runs every (uncorrelated) scalar
    subquery exactly once and stores its value where the ScalarSubqueryExprs of the main plan read it.  A subquery returns zero
    rows (NULL) or one; more is the reference's "Scalar subquery returned more than one row" error."""

    def __init__(self, input: ExecutionPlan, subqueries, results):
        self.input, self.subqueries, self.results = input, list(subqueries), results   # subqueries: [(plan, index)]

    def children(self):
        return [self.input] + [p for p, _ in self.subqueries]

    def with_new_children(self, c):
        return ScalarSubqueryExec(c[0], [(p, i) for p, (_, i) in zip(c[1:], self.subqueries)], self.results)

    def execute(self, partition=0):
        for plan, index in self.subqueries:
            t, owned = self._run_child(plan)
            if t.num_rows > 1:
                raise _lib.DfgpuError("Scalar subquery returned more than one row")
            self.results[index] = None if t.num_rows == 0 else t.select([0]).to_arrow().column(0)[0].as_py()
            if owned:
                t.free()
        return self._pass_through(self.input)

    def detail(self):
        return f"subqueries={len(self.subqueries)}"


class GpuFusedAggregateExec(_Unary):
    """FilterExec + ProjectionExec + AggregateExec as one node: predicate, inlined argument expressions and
    accumulation in a single pass over the input's referenced columns (dfgpu_agg_update_filtered; the kernel is
    specialised for the forest with hiprtc for large inputs, jit.hip).  Output schema = the AggregateExec's."""

    def __init__(self, mode, group_by, aggr_expr, predicate, input: ExecutionPlan):
        self.mode, self.group_by, self.aggr_expr, self.predicate, self.input = mode, group_by, aggr_expr, predicate, input
        self.return_types = None

    def with_new_children(self, c):
        return GpuFusedAggregateExec(self.mode, self.group_by, self.aggr_expr, self.predicate, c[0])

    def execute(self, partition=0):
        t, owned = self._run_child(self.input)
        if self.mode == "Partial":
            self.return_types = ops.aggregate_return_types(t, self.aggr_expr)
        out = ops.aggregate(t, self.group_by, self.aggr_expr, self.mode, predicate=self.predicate)
        if owned:
            t.free()
        return out

    def detail(self):
        return f"mode={self.mode}, predicate={self.predicate!r}, gby=[{', '.join(n for _, n in self.group_by)}], aggr=[{_aggr_detail(self.aggr_expr)}]"


class GpuHashJoinExec(HashJoinExec):
    """HashJoinExec with the FilterExec of its probe side fused below it (dfgpu_join_probe_filtered)"""

    def __init__(self, join: HashJoinExec, probe_predicate: PhysicalExpr, probe_input: ExecutionPlan, probe_mode=None):
        super().__init__(join.left, probe_input, join.on, join.join_type, join.projection, join.null_equality,
                         join.probe_mode if probe_mode is None else probe_mode, null_aware=join.null_aware)
        self.probe_predicate = probe_predicate

    def with_new_children(self, c):
        j = HashJoinExec(c[0], c[1], self.on, self.join_type, self.projection, self.null_equality, self.probe_mode, self.filter, self.null_aware)
        return GpuHashJoinExec(j, self.probe_predicate, c[1])

    def execute(self, partition=0):
        return super().execute(partition, probe_predicate=self.probe_predicate)

    def detail(self):
        return super().detail() + f", probe_predicate={self.probe_predicate!r}"


# --------------------------------------------------------------------------------------- the rule
class GpuOffloadRule:
    """PhysicalOptimizerRule (session/src/physical_optimizer.rs:52-84), appended with
    SessionStateBuilder::with_physical_optimizer_rule (core/src/execution/session_state.rs:1407-1415) so that it
    runs after the built-in rules have fixed distribution, ordering and join sides.  `unordered_probe=True` lets
    joins whose parent does not need the probe-side order (an aggregate or a repartition) take the single-pass
    unordered probe where it applies (probe_mode "order_not_needed": at most one match per probe row, non-nullable
    payload; the library falls back to the general path otherwise) — the rule knows the parent because it rewrites bottom-up and fixes the child when it
    visits the parent.  `range_joins=True` (one rank) turns a NestedLoopJoinExec whose filter is a range condition on one right column
    (range_condition) over keys the device takes into a GpuRangeJoinExec — for the one-sided join types, and for the pair types where
    the parent does not observe order, because the range join's pairs come left-row-major.  The default leaves every plan as it was."""

    def __init__(self, world_size: int = 1, unordered_probe: bool = True, range_joins: bool = False):
        self.world_size, self.unordered_probe, self.range_joins = world_size, unordered_probe, range_joins
        self.declined = []    # (node, reason) of operators the rule left to the CPU

    def _admits(self, node) -> bool:
        """spill-aware fallback: a hash join whose device footprint the pool cannot admit stays the reference's CPU
        operator, which can spill (MemoryReservation::try_grow failing is how the reference itself learns it, hash_join/exec.rs:2608).
        The estimate uses row-count upper bounds of the children (their statistics) and dfgpu_join_estimate_bytes."""
        if _lib._initialised_device is None:
            return True       # planning without a device (tests of the rewrite shapes): nothing to admit against
        try:
            b_rows, b_bytes = _row_bound(node.left)
            p_rows, p_bytes = _row_bound(node.right)
        except (TypeError, AttributeError):
            return True       # no statistics: decided at run time by the build's own reservation
        out_row = (b_bytes + p_bytes)
        need = ops.join_estimate_bytes(b_rows, b_bytes, p_rows, -1, out_row)
        try:
            ops.Reservation(need).release()
            return True
        except _lib.DfgpuError as e:
            self.declined.append((node, str(e)))
            return False

    def _admits_pairs(self, node) -> bool:
        """a pair-output nested-loop join without a filter (a cross join) is the one join whose output size is known at plan time:
        |L| x |R| rows of 16 bytes of row ids (plus the rows themselves).  One the pool cannot reserve stays the reference's operator."""
        if node.filter is not None or node.join_type not in ("Inner", "Left", "Right", "Full") or _lib._initialised_device is None:
            return True
        try:
            l_rows, l_bytes = _row_bound(node.left)
            r_rows, r_bytes = _row_bound(node.right)
        except (TypeError, AttributeError):
            return True
        try:
            ops.Reservation(l_rows * r_rows * (16 + l_bytes + r_bytes)).release()
            return True
        except _lib.DfgpuError as e:
            self.declined.append((node, str(e)))
            return False

    def name(self) -> str:
        return "gpu_offload_amd"

    def schema_check(self) -> bool:
        return True

    def optimize(self, plan: ExecutionPlan) -> ExecutionPlan:
        plan = self._rewrite(plan, parent_needs_order=True)
        self._decline_orphan_partials(plan)
        return plan

    def _decline_orphan_partials(self, node: ExecutionPlan):
        """a Partial node with a DISTINCT aggregate or a MEDIAN that no Final parent collapsed (see _rewrite) stays the reference's operator"""
        if isinstance(node, AggregateExec) and node.mode == "Partial" and _has_distinct(node) and not getattr(node, "kept_on_cpu", False):
            node.kept_on_cpu = True
            self.declined.append((node, unsupported_reason(node)))
        for c in node.children():
            self._decline_orphan_partials(c)

    # transform_up: children first (tree_node.rs), then this node.  `needs_order` = some ancestor observes this
    # node's output order (maintains_input_order / required_input_ordering in the reference's terms)
    def _rewrite(self, node: ExecutionPlan, parent_needs_order: bool) -> ExecutionPlan:
        kids = []
        for i, c in enumerate(node.children()):
            if isinstance(node, (AggregateExec, GpuFusedAggregateExec, RepartitionExec, SortExec)):
                need = False                                   # these consume their input in any order
            elif isinstance(node, WindowAggExec):
                need = True                                    # partitions and peer groups ARE the input's order, whatever the parent needs
            elif isinstance(node, (HashJoinExec, NestedLoopJoinExec, GpuRangeJoinExec)):
                need = parent_needs_order and i == 1           # only the probe side's order shows in the output
            else:
                need = parent_needs_order                      # FilterExec / ProjectionExec / CoalesceBatchesExec keep it
            kids.append(self._rewrite(c, need))
        if kids:
            node = node.with_new_children(kids)
        # bookkeeping nodes that have no meaning for whole-partition device tables
        if isinstance(node, CoalesceBatchesExec):
            return node.input
        if isinstance(node, (RepartitionExec, CoalescePartitionsExec, SortPreservingMergeExec)) and self.world_size == 1:
            return node.input                                  # one partition: nothing to exchange, gather or merge
        if isinstance(node, WindowAggExec) and self.world_size > 1 and not getattr(node, "kept_on_cpu", False):
            # a window over several ranks needs its partitions co-located first; that path is not exercised, so the node is not taken
            node.kept_on_cpu = True
            self.declined.append((node, f"WindowAggExec on {self.world_size} ranks: the window is only exercised on one rank"))
            return node
        if isinstance(node, NestedLoopJoinExec) and self.world_size > 1 and not getattr(node, "kept_on_cpu", False):
            # every rank would need the whole left side and a share of the right one: that path is not exercised, so the node is not taken
            node.kept_on_cpu = True
            self.declined.append((node, f"{node.name()} on {self.world_size} ranks: the nested loop join is only exercised on one rank"))
            return node
        if isinstance(node, AggregateExec) and self.world_size == 1 and _has_distinct(node) and not getattr(node, "kept_on_cpu", False):
            # DISTINCT aggregates and MEDIAN have no device partial state.  On one rank the exchange between Final and Partial is gone already and
            # Final o Partial == Single: the Partial is left as it is when it is visited, and the pair becomes ONE Single node — the
            # Partial's expressions over the Partial's input, the Final's output names — when its Final parent is
            if node.mode == "Partial":
                return node
            # (only through the exchange and bookkeeping nodes, which mean nothing on one rank: a filter, limit or sort between the two
            # would be lost with them, so such a pair is declined like any staged DISTINCT aggregate)
            below = _partial_below(node.input, _EXCHANGE_NODES) if node.mode in ("Final", "FinalPartitioned") else None
            if below is not None and isinstance(below, AggregateExec) and not getattr(below, "kept_on_cpu", False) \
                    and len(below.group_by) == len(node.group_by) and len(below.aggr_expr) == len(node.aggr_expr):
                gb = [(e, n) for (e, _), (_, n) in zip(below.group_by, node.group_by)]
                aggs = [(f, e, fin[2]) if flt is None else (f, e, fin[2], flt)
                        for (f, e, _, flt), fin in zip(ops.normalize_aggs(below.aggr_expr), ops.normalize_aggs(node.aggr_expr))]
                single = AggregateExec("Single", gb, aggs, below.input)
                try:
                    reason = unsupported_reason(single)
                except Exception:  # noqa: BLE001 - as below: a plan this layer cannot type is decided at run time
                    reason = None
                if reason is not None:                         # (an argument type the device refuses: the pair stays as it was)
                    node.kept_on_cpu = below.kept_on_cpu = True
                    self.declined.append((node, reason))
                    return node
                node = single                                  # and on through the usual handling of a Single node
        if not isinstance(node, (GpuHashJoinExec, GpuFusedAggregateExec)) and not getattr(node, "kept_on_cpu", False):
            try:
                reason = unsupported_reason(node)
            except Exception:  # noqa: BLE001 - a plan this layer cannot type (stand-in leaves of planning-only tests): decided at run time
                reason = None
            if reason is not None:                             # the reference's operator stays (it runs these inputs)
                node.kept_on_cpu = True
                self.declined.append((node, reason))
                return node
        if isinstance(node, HashJoinExec) and not isinstance(node, GpuHashJoinExec) and not self._admits(node):
            node.kept_on_cpu = True
            return node
        if isinstance(node, NestedLoopJoinExec) and not getattr(node, "kept_on_cpu", False) and not self._admits_pairs(node):
            node.kept_on_cpu = True
            return node
        if self.range_joins and self.world_size == 1 and type(node) is NestedLoopJoinExec and not getattr(node, "kept_on_cpu", False):
            cond = range_condition(node.filter)
            if cond is not None and (node.join_type not in ("Inner", "Left", "Right", "Full") or not parent_needs_order):
                rj = GpuRangeJoinExec(node.left, node.right, cond[0], cond[1], cond[2], node.join_type, node.projection)
                try:
                    taken = plan_schema(node.left) is not None and plan_schema(node.right) is not None and unsupported_reason(rj) is None
                except Exception:  # noqa: BLE001 - children that cannot be typed at plan time: the key types are unknown, the node stays
                    taken = False
                if taken:
                    return rj
        if isinstance(node, HashJoinExec) and not isinstance(node, GpuHashJoinExec):
            probe_mode = ops.PROBE_MODES["order_not_needed"] if (self.unordered_probe and not parent_needs_order and
                                                                      node.join_type in ("Inner", "RightSemi", "RightAnti")) else node.probe_mode
            node = HashJoinExec(node.left, node.right, node.on, node.join_type, node.projection, node.null_equality,
                                node.probe_mode if node.filter is not None else probe_mode, node.filter, node.null_aware)
            probe = node.right
            if node.filter is None and isinstance(probe, FilterExec) and node.join_type in ("Inner", "RightSemi", "RightAnti", "Right", "RightMark"):
                needed = set(r for _, r in node.on) | set((node.projection or (None, None))[1] or [])
                # the FilterExec's embedded projection must keep what the join reads (it always does in a valid plan)
                if probe.projection is None or needed <= set(probe.projection):
                    return GpuHashJoinExec(node, probe.predicate, probe.input, probe_mode)
            return node
        if isinstance(node, AggregateExec) and node.mode in ("Single", "SinglePartitioned", "Partial"):
            child, mapping, predicate = node.input, {}, None
            if isinstance(child, ProjectionExec):
                mapping = {n: e for e, n in child.exprs}
                child = child.input
            if isinstance(child, FilterExec):
                predicate = child.predicate
                child = child.input
            if mapping or predicate is not None:
                gb = [(substitute(e, mapping), n) for e, n in node.group_by]
                # (the projection's names are resolved inside the filters as inside the arguments; an aggregate without one keeps its 3-tuple)
                aggs = [(f, None if e is None else substitute(e, mapping), n) if flt is None else
                        (f, None if e is None else substitute(e, mapping), n, substitute(flt, mapping)) for f, e, n, flt in ops.normalize_aggs(node.aggr_expr)]
                return GpuFusedAggregateExec(node.mode, gb, aggs, predicate, child)
        return node


def _row_bound(node):
    """(upper bound of the output rows, bytes per row) of a subtree from its leaves' statistics"""
    if isinstance(node, MemoryExec):
        t = node.execute()
        return t.num_rows, (t.nbytes() // max(1, t.num_rows))
    if isinstance(node, (FilterExec, ProjectionExec, CoalesceBatchesExec, RepartitionExec, CoalescePartitionsExec, SortExec, SortPreservingMergeExec,
                         AggregateExec, GpuFusedAggregateExec)):
        return _row_bound(node.children()[0])
    if isinstance(node, WindowAggExec):   # every input row, 16 bytes more per window column at the most (a Decimal128 result)
        rows, width = _row_bound(node.input)
        return rows, width + 16 * len(node.window_expr)
    if isinstance(node, HashJoinExec):
        (br, bb), (pr, pb) = _row_bound(node.left), _row_bound(node.right)
        return max(br, pr), bb + pb
    if isinstance(node, (NestedLoopJoinExec, GpuRangeJoinExec)):
        (br, bb), (pr, pb) = _row_bound(node.left), _row_bound(node.right)
        if node.join_type in ("LeftSemi", "LeftAnti", "LeftMark"):
            return br, bb + 1
        if node.join_type in ("RightSemi", "RightAnti", "RightMark"):
            return pr, pb + 1
        return br * pr + br + pr, bb + pb
    raise TypeError(node.name())


# ------------------------------------------------------------------------------ plan-time schemas and declines
def plan_schema(node):
    """Output schema of a plan node (pa.Schema), or None when it cannot be told at plan time (a scan that has not opened its file,
    a node below one that could not be typed).  What ExecutionPlan::schema() is in the reference; here it only serves the rule's
    decisions — expression types come from the library (dfgpu_expr_type over an empty table of the input schema)."""
    import pyarrow as pa
    if isinstance(node, MemoryExec):
        sch = node.table.schema
        if node.projection is None:
            return sch
        idx = [node.table.index_of(c) for c in node.projection]
        return pa.schema([sch.field(i) for i in idx])
    if isinstance(node, GpuHashJoinExec) or isinstance(node, HashJoinExec):
        l, r = plan_schema(node.left), plan_schema(node.right)
        if l is None or r is None:
            return None
        bc, pc = node.projection if node.projection is not None else (None, None)
        lf = list(l) if bc is None else [l.field(l.get_field_index(c)) if isinstance(c, str) else l.field(c) for c in bc]
        rf = list(r) if pc is None else [r.field(r.get_field_index(c)) if isinstance(c, str) else r.field(c) for c in pc]
        jt = node.join_type
        if jt in ("LeftSemi", "LeftAnti"):
            return pa.schema(lf)
        if jt in ("RightSemi", "RightAnti"):
            return pa.schema(rf)
        if jt == "LeftMark":
            return pa.schema(lf + [pa.field("mark", pa.bool_())])
        if jt == "RightMark":
            return pa.schema(rf + [pa.field("mark", pa.bool_())])
        return pa.schema(lf + rf)
    if isinstance(node, (NestedLoopJoinExec, GpuRangeJoinExec)):
        l, r = plan_schema(node.left), plan_schema(node.right)
        if l is None or r is None:
            return None
        lc, rc = node.projection if node.projection is not None else (None, None)
        lf = list(l) if lc is None else [l.field(l.get_field_index(c)) if isinstance(c, str) else l.field(c) for c in lc]
        rf = list(r) if rc is None else [r.field(r.get_field_index(c)) if isinstance(c, str) else r.field(c) for c in rc]
        jt = node.join_type
        if jt in ("LeftSemi", "LeftAnti"):
            return pa.schema(lf)
        if jt in ("RightSemi", "RightAnti"):
            return pa.schema(rf)
        if jt == "LeftMark":
            return pa.schema(lf + [pa.field("mark", pa.bool_(), nullable=False)])
        if jt == "RightMark":
            return pa.schema(rf + [pa.field("mark", pa.bool_(), nullable=False)])
        # build_join_schema (joins/utils.rs): the side that unmatched rows of the other side extend with NULLs becomes nullable
        if jt in ("Right", "Full"):
            lf = [f.with_nullable(True) for f in lf]
        if jt in ("Left", "Full"):
            rf = [f.with_nullable(True) for f in rf]
        return pa.schema(lf + rf)
    kids = node.children()
    if len(kids) != 1:
        return None
    inp = plan_schema(kids[0])
    if inp is None:
        return None
    if isinstance(node, FilterExec):
        if node.projection is None:
            return inp
        return pa.schema([inp.field(inp.get_field_index(c)) if isinstance(c, str) else inp.field(c) for c in node.projection])
    if isinstance(node, (CoalesceBatchesExec, RepartitionExec, CoalescePartitionsExec, SortPreservingMergeExec, SortExec)):
        return inp
    try:
        empty = DeviceTable.from_arrow(inp.empty_table())
    except Exception:  # noqa: BLE001 - no device (planning-only tests): nothing can be typed
        return None
    try:
        if isinstance(node, WindowAggExec):
            fields = list(inp)
            for func, e, n, _ in ops.normalize_window_exprs(node.window_expr):
                func = func[0] if isinstance(func, tuple) else func
                if func in ops.WINDOW_RANKING or func == "ntile":
                    fields.append(pa.field(n, pa.uint64(), nullable=False))
                elif func in ops.WINDOW_DIST_FUNCS:
                    fields.append(pa.field(n, pa.float64(), nullable=False))
                elif func in ops.WINDOW_VALUE_FUNCS:
                    t = ops.expr_type(empty, e)
                    if isinstance(e, Column):      # a dictionary-encoded column keeps its dictionary (the device types its codes)
                        src = inp.field(inp.get_field_index(e.name) if e.index is None else e.index).type
                        t = src if pa.types.is_dictionary(src) else t
                    fields.append(pa.field(n, t, nullable=True))
                else:
                    fields.append(pa.field(n, _agg_type(func, None if e is None else ops.expr_type(empty, e)), nullable=func != "count"))
            return pa.schema(fields)
        if isinstance(node, ProjectionExec):
            return pa.schema([pa.field(n, ops.expr_type(empty, e)) for e, n in node.exprs])
        if isinstance(node, (AggregateExec, GpuFusedAggregateExec)):
            if node.mode in ("Final", "FinalPartitioned"):
                # a Final node's aggregate expressions are its Partial twin's (over the RAW input): typed there, named here
                below = _partial_below(node.input)
                if below is None:
                    return None
                raw = plan_schema(AggregateExec("Single", below.group_by, below.aggr_expr, below.input))
                if raw is None or len(raw) != len(node.group_by) + len(node.aggr_expr):
                    return None
                names = [n for _, n in node.group_by] + [a[2] for a in node.aggr_expr]
                return pa.schema([pa.field(n, f.type) for n, f in zip(names, raw)])
            fields = [pa.field(n, ops.expr_type(empty, e)) for e, n in node.group_by]
            for func, e, n, _ in ops.normalize_aggs(node.aggr_expr):   # (a FILTER changes no type: the state schema is the unfiltered one)
                t = None if e is None else ops.expr_type(empty, e)
                if node.mode == "Partial":      # state fields (sum.rs:281-301, average.rs:317-360, count.rs): AVG = count + sum
                    if func in ops.VARIANCE_FUNCS:   # variance.rs state_fields: count, mean, m2
                        fields += [pa.field(n + "[count]", pa.uint64()), pa.field(n + "[mean]", pa.float64()), pa.field(n + "[m2]", pa.float64())]
                    elif func == "avg":
                        fields.append(pa.field(n + "[count]", pa.uint64()))
                        # avg_sum_data_type (average.rs:131-172): the input precision + 13 digits, never narrower than Decimal128's 38
                        fields.append(pa.field(n + "[sum]", pa.decimal128(38, t.scale) if pa.types.is_decimal128(t) else pa.float64()))
                    else:   # one state column (bit_* / bool_*: of the argument's type, named like the aggregate)
                        fields.append(pa.field(n, _agg_type(func, t)))
                else:
                    fields.append(pa.field(n, _agg_type(func, t)))
            return pa.schema(fields)
    except (_lib.DfgpuError, KeyError, TypeError, ValueError):
        return None   # an expression this layer cannot type: the node's schema stays unknown and nothing is decided on it
    finally:
        empty.free()
    return None


def _sum_type(t):
    import pyarrow as pa
    if pa.types.is_decimal128(t):
        return pa.decimal128(min(38, t.precision + 10), t.scale)      # sum.rs:232-260
    if pa.types.is_floating(t):
        return pa.float64()
    return pa.uint64() if pa.types.is_unsigned_integer(t) and t != pa.uint8() else pa.int64()


def _agg_type(func, t):
    import pyarrow as pa
    if func in ("count", "count_distinct"):
        return pa.int64()
    if func in ("sum", "sum_distinct"):
        return _sum_type(t)
    if func == "avg":
        return pa.decimal128(min(38, t.precision + 4), min(38, t.scale + 4)) if pa.types.is_decimal128(t) else pa.float64()   # average.rs:219-252
    if func in ops.VARIANCE_FUNCS:
        return pa.float64()     # variance.rs / stddev.rs return_type
    return t    # min / max; bit_and / bit_or / bit_xor and bool_and / bool_or; median: the argument's type (bit_and_or_xor.rs, bool_and_or.rs, median.rs)


def _device_type_name(t):
    """runtime.hip type_name: how the library's messages spell a column type.  A type the device does not have (no table holds one) is
    spelled as pyarrow spells it."""
    import pyarrow as pa
    if pa.types.is_decimal128(t):
        return f"Decimal128({t.precision},{t.scale})"
    names = {pa.int32(): "Int32", pa.int64(): "Int64", pa.float64(): "Float64", pa.uint8(): "UInt8", pa.uint32(): "UInt32", pa.uint64(): "UInt64",
             pa.date32(): "Date32", pa.bool_(): "Boolean"}
    return names.get(t, str(t))


def _argument_type(node, inp, e, t):
    """the type an aggregate's type check sees for argument `e` typed as `t`: the device types a dictionary-encoded string column by its
    codes (Int32), while the library's checks know the column has a dictionary (aggregate.hip distinct_check_type, median_check_type:
    `v.dict`).  The input's schema says so for an Arrow source, the device table itself for a scan of one; anything else is `t`."""
    import pyarrow as pa
    if not isinstance(e, Column):
        return t
    src = inp.field(inp.get_field_index(e.name) if e.index is None else e.index).type
    if pa.types.is_dictionary(src):
        return src
    scan = node.input
    if isinstance(scan, MemoryExec) and scan.projection is None and hasattr(scan.table, "dictionary_size") \
            and scan.table.dictionary_size(e.name if e.index is None else e.index) is not None:
        return pa.dictionary(pa.int32(), pa.string())
    return t


def _key_bits(t):
    """upper bound of the bits a sort key column of this type takes in the packed key (sort.hip packs value ranges; the type is
    what is known at plan time), plus one bit for NULL placement"""
    import pyarrow as pa
    if pa.types.is_boolean(t):
        return 2
    if pa.types.is_string(t) or pa.types.is_large_string(t) or pa.types.is_dictionary(t):
        return 33
    return t.bit_width + 1


def unsupported_reason(node):
    """Why an operator the reference can run has no device form (None = it has one).  The library refuses these inputs when it
    meets them at run time (the DFGPU_CHECKs named below); the rule asks first, so that such an operator STAYS the reference's CPU
    operator instead of failing the query — every entry here has a test that feeds a plan through GpuOffloadRule."""
    import pyarrow as pa
    if isinstance(node, (AggregateExec, GpuFusedAggregateExec)):
        # aggregate.hip dfgpu_agg_create: a DISTINCT aggregate's and a MEDIAN's partial state is a List column in the reference, so the device takes
        # the single-stage modes only (known without typing anything: a plan without a device is told the same)
        for func, e, n, _ in ops.normalize_aggs(node.aggr_expr):
            if func in ops.NO_PARTIAL_STATE_FUNCS and e is None:
                return f"{ops.NO_PARTIAL_STATE_NAMES[func]} (aggregate {n}) needs an argument"
            if func in ops.NO_PARTIAL_STATE_FUNCS and node.mode not in ("Single", "SinglePartitioned"):
                return f"{ops.NO_PARTIAL_STATE_NAMES[func]} (aggregate {n}) is not supported in mode {node.mode} on the GPU path: its partial state is a List column"
    if isinstance(node, (AggregateExec, GpuFusedAggregateExec)) and node.mode in ("Single", "SinglePartitioned", "Partial"):
        inp = plan_schema(node.input)
        if inp is None:
            return None
        try:
            empty = DeviceTable.from_arrow(inp.empty_table())
        except Exception:  # noqa: BLE001
            return None
        try:
            for func, e, n, flt in ops.normalize_aggs(node.aggr_expr):
                if flt is not None:
                    # aggregate.hip: "the FILTER expression must be Boolean"; one the expression layer cannot lower keeps the node here too
                    try:
                        ft = ops.expr_type(empty, flt)
                    except _lib.DfgpuError as err:
                        return f"{func.upper()}({n}) FILTER (WHERE {flt!r}): {err}"
                    except (KeyError, TypeError, ValueError) as err:
                        return f"{func.upper()}({n}) FILTER (WHERE {flt!r}) cannot be lowered: {err}"
                    if not pa.types.is_boolean(ft):
                        return f"{func.upper()}({n}) FILTER (WHERE {flt!r}): the filter is {ft}, not Boolean"
                if e is None:
                    continue
                try:
                    t = ops.expr_type(empty, e)
                except _lib.DfgpuError as err:
                    return f"{func}({e!r}): {err}"
                except (KeyError, TypeError, ValueError):
                    continue   # not typable from this schema (a name the input does not carry): decided at run time
                if func in ops.NO_PARTIAL_STATE_FUNCS:
                    t = _argument_type(node, inp, e, t)
                if func in ops.HOLISTIC_FUNCS:
                    # aggregate.hip median_check_type, in its words
                    if pa.types.is_boolean(t):
                        return "MEDIAN over Boolean is not supported on the GPU path"
                    if pa.types.is_string(t) or pa.types.is_large_string(t) or pa.types.is_dictionary(t):
                        return "MEDIAN over Utf8 is not supported on the GPU path"
                    if not (pa.types.is_decimal128(t) or t in (pa.int32(), pa.int64(), pa.uint8(), pa.uint32(), pa.uint64(), pa.float64())):
                        return f"MEDIAN over {_device_type_name(t)} is not supported on the GPU path"
                    continue
                if func in ops.DISTINCT_FUNCS:
                    # aggregate.hip distinct_check_type, in its words (type_name's spelling for every type the device has)
                    what, stringy = ops.DISTINCT_NAMES[func], pa.types.is_string(t) or pa.types.is_large_string(t) or pa.types.is_dictionary(t)
                    summable = pa.types.is_decimal128(t) or t in (pa.int32(), pa.int64(), pa.uint8(), pa.uint32(), pa.uint64())
                    if pa.types.is_boolean(t):
                        return f"{what} over Boolean is not supported on the GPU path"
                    if func == "sum_distinct" and stringy:
                        return f"{what} over Utf8 is not supported on the GPU path"
                    if func == "sum_distinct" and t == pa.float64():
                        return f"{what} over Float64 is not supported on the GPU path"
                    if not (summable or (func == "count_distinct" and (stringy or t in (pa.date32(), pa.float64())))):
                        return f"{what} over {_device_type_name(t)} is not supported on the GPU path"
                    continue
                if func == "avg" and pa.types.is_decimal128(t) and t.precision + 13 > 38:
                    # aggregate.hip avg_sum_type: avg_sum_data_type (average.rs:131-172) widens to Decimal256 beyond 38 digits
                    return f"AVG({n}) over {t} accumulates in Decimal256 in the reference (no device representation)"
                if func in ("min", "max") and pa.types.is_decimal128(t) and t.precision > 18:
                    # aggregate.hip wide_minmax_values_fit: the device compares 64-bit words; values beyond them are only found at run time
                    return f"{func.upper()}({n}) over {t}: values of more than 18 digits do not fit the device's 64-bit comparison"
                if func in ("min", "max") and t == pa.uint64():
                    # aggregate.hip plan_for: MIN / MAX use signed 64-bit atomics (tests/test_gpu_edge_values.py::test_min_max_over_uint64_is_refused_and_stays_on_the_cpu)
                    return f"{func.upper()}({n}) over UInt64 is not supported on the GPU path"
                if func in ("sum", "avg", "min", "max") and (pa.types.is_boolean(t) or pa.types.is_string(t) or pa.types.is_large_string(t)):
                    return f"{func.upper()}({n}) over {t} is not supported on the GPU path"
                if func in ops.VARIANCE_FUNCS and t not in (pa.float64(), pa.int32(), pa.int64()):
                    # aggregate.hip plan_for: the device reads a Float64, Int32 or Int64 argument (the planner casts to Float64)
                    return f"{func.upper()}({n}) over {t} is not supported on the GPU path"
                if func in ops.BITWISE_FUNCS and t not in (pa.int32(), pa.int64(), pa.uint8(), pa.uint32(), pa.uint64()):
                    # aggregate.hip plan_for: BIT_AND / BIT_OR / BIT_XOR take the integer types the device has
                    return f"{func.upper()}({n}) over {t} is not supported on the GPU path"
                if func in ops.BOOLEAN_FUNCS and not pa.types.is_boolean(t):
                    # aggregate.hip plan_for: BOOL_AND / BOOL_OR take a Boolean
                    return f"{func.upper()}({n}) over {t} is not supported on the GPU path"
        finally:
            empty.free()
        return None
    if isinstance(node, WindowAggExec):
        inp = plan_schema(node.input)
        if inp is None:
            return None
        for c in node.partition_by + [c for c, _, _ in node.order_by]:
            t = inp.field(inp.get_field_index(c) if isinstance(c, str) else c).type
            # window.hip window_keys: keys are compared by value bits plus validity.  How the reference treats +0.0 / -0.0 and NaN as
            # peers cannot be checked here, so Float64 keys are not taken; Boolean keys are bit-packed, Utf8 keys have no fixed width
            if pa.types.is_floating(t):
                return "Float64 window keys are not supported on the GPU path"
            if pa.types.is_boolean(t):
                return "Boolean window keys are not supported on the GPU path"
            if pa.types.is_string(t) or pa.types.is_large_string(t):
                return "Utf8 window keys are not supported on the GPU path"
        try:
            empty = DeviceTable.from_arrow(inp.empty_table())
        except Exception:  # noqa: BLE001
            return None
        try:
            for func, e, n, _ in ops.normalize_window_exprs(node.window_expr):
                func = func[0] if isinstance(func, tuple) else func
                if e is None or func == "count":
                    continue
                try:
                    t = ops.expr_type(empty, e)
                except _lib.DfgpuError as err:
                    return f"{func}({e!r}): {err}"
                except (KeyError, TypeError, ValueError):
                    continue
                if func in ops.WINDOW_VALUE_FUNCS:
                    # window.hip window_table: the argument's bytes are picked whatever they mean (dictionary codes too); Boolean columns
                    # are bit-packed and Utf8 columns have no fixed width
                    if pa.types.is_boolean(t):
                        return f"{func.upper()}({n}) over Boolean is not supported on the GPU path"
                    if pa.types.is_string(t) or pa.types.is_large_string(t):
                        return f"{func.upper()}({n}) over Utf8 is not supported on the GPU path"
                    continue
                if func == "avg" and pa.types.is_decimal128(t) and t.precision + 13 > 38:
                    # window.hip plan_window: the aggregate's refusal (avg_sum_data_type widens to Decimal256 beyond 38 digits)
                    return f"AVG({n}) over {t} accumulates in Decimal256 in the reference (no device representation)"
                # window.hip plan_window: the argument types of the GPU AggregateExec (MIN / MAX over Decimal128 at any precision)
                ok = {"sum": (pa.int32(), pa.int64(), pa.uint8(), pa.uint32(), pa.uint64(), pa.float64()),
                      "avg": (pa.int32(), pa.int64(), pa.float64()),
                      "min": (pa.int32(), pa.int64(), pa.uint8(), pa.uint32(), pa.float64(), pa.date32()),
                      "max": (pa.int32(), pa.int64(), pa.uint8(), pa.uint32(), pa.float64(), pa.date32())}[func]
                if not (pa.types.is_decimal128(t) or t in ok):
                    return f"{func.upper()}({n}) over {t} is not supported on the GPU path"
        finally:
            empty.free()
        return None
    if isinstance(node, SortExec):
        inp = plan_schema(node.input)
        if inp is None:
            return None
        bits = sum(_key_bits(inp.field(inp.get_field_index(c) if isinstance(c, str) else c).type) for c, _, _ in node.expr)
        if bits > 192:   # sort.hip: "packed sort key longer than 192 bits"
            return f"sort key of up to {bits} bits: the device packs at most 192"
        return None
    if isinstance(node, GpuRangeJoinExec):
        # nlj.hip range_join: the same checks in the same order, with the same messages
        if node.lower is None and node.upper is None:
            return RANGE_JOIN_NO_BOUND
        l, r = plan_schema(node.left), plan_schema(node.right)
        if l is None or r is None:
            return None
        sides = [(node.right, r, node.x)] + [(node.left, l, bound[0]) for bound in (node.lower, node.upper) if bound is not None]
        try:
            keys = [_schema_field(sch, c) for _, sch, c in sides]
        except (KeyError, IndexError, ValueError) as err:
            return f"range join key column out of range: {err}"
        taken = (pa.int32(), pa.int64(), pa.date32(), pa.uint32(), pa.uint64(), pa.float64())
        for (child, sch, c), f in zip(sides, keys):
            encoded = pa.types.is_dictionary(f.type)
            if not encoded and isinstance(child, MemoryExec) and hasattr(child.table, "dictionary_size"):
                # a device table's schema shows a dictionary-encoded column as its index type: the table itself knows
                i = sch.get_field_index(c) if isinstance(c, str) else int(c)
                encoded = child.table.dictionary_size(i if child.projection is None else child.table.index_of(child.projection[i])) is not None
            if encoded:
                return RANGE_JOIN_DICT_KEY
            if f.type not in taken:
                return RANGE_JOIN_KEY_TYPE
        if any(f.type != keys[0].type for f in keys):
            return RANGE_JOIN_MIXED_KEYS
        return None
    if isinstance(node, NestedLoopJoinExec):
        if node.filter is None:
            return None
        l, r = plan_schema(node.left), plan_schema(node.right)
        if l is None or r is None:
            return None
        fexpr, fcols = node.filter
        try:
            inter = pa.schema([pa.field(f"f{k}", (l if side == "Left" else r).field(int(i)).type) for k, (i, side) in enumerate(fcols)])
        except (KeyError, IndexError, ValueError) as err:
            return f"join filter column index out of range: {err}"
        try:
            empty = DeviceTable.from_arrow(inter.empty_table())
        except Exception:  # noqa: BLE001
            return None
        try:
            # nlj.hip nested_loop_join: "join filter expression must be Boolean"; a filter the expression layer cannot lower stays here too
            try:
                ft = ops.expr_type(empty, fexpr)
            except _lib.DfgpuError as err:
                return f"join filter {fexpr!r}: {err}"
            except (KeyError, TypeError, ValueError) as err:
                return f"join filter {fexpr!r} cannot be lowered: {err}"
            if not pa.types.is_boolean(ft):
                return f"join filter expression must be Boolean: {fexpr!r} is {ft}"
        finally:
            empty.free()
        return None
    if isinstance(node, HashJoinExec):
        try:
            b_rows, _ = _row_bound(node.left)
        except (TypeError, AttributeError):
            return None
        if b_rows >= 0xFFFFFFFF:   # join.hip: the reference switches to JoinHashMapU64 (joins/join_hash_map.rs:224); row ids here are 32 bits
            return f"build side of up to {b_rows} rows: the device addresses build rows with 32 bits (JoinHashMapU64 is not built)"
        return None
    return None


def displayable(plan: ExecutionPlan, indent: int = 0) -> str:
    """DisplayableExecutionPlan::indent (display.rs): one line per node, children indented"""
    line = "  " * indent + plan.name() + (": " + plan.detail() if plan.detail() else "")
    return "\n".join([line] + [displayable(c, indent + 1) for c in plan.children()])


def collect(plan: ExecutionPlan) -> DeviceTable:
    """physical_plan::collect for a single-partition plan; the caller owns the result"""
    out = plan.execute(0)
    return out.select(list(range(out.num_columns))) if isinstance(plan, MemoryExec) else out
