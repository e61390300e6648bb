"""TEST INFRASTRUCTURE: what the key statistics and the join's dynamic filters mean, restated in plain Python over `to_pylist()` values
(no numpy reduction, no Arrow compute kernel, none of the oracle's code): the reference tests/test_zz_gpu_key_stats.py and
tests/test_zz_gpu_dynamic_filter.py hold dfgpu_column_minmax, its readers (join build, sort, aggregate), dfgpu_column_inlist,
dfgpu_join_contains and the probe-side scan's pruning to.  tests/test_key_stats_reference.py checks this file itself, without a GPU.

Everything here is exact integer (or bit pattern) work."""
import struct

import pyarrow as pa


def values_of(column) -> list:
    """the rows of an Arrow column as Python values that compare the way the kernels compare keys: integers as themselves (Date32 as its
    day number), Float64 by its bits, everything else as to_pylist() gives it; None = NULL"""
    column = column.combine_chunks() if isinstance(column, pa.ChunkedArray) else column
    t = column.type
    if pa.types.is_dictionary(t):
        column, t = column.cast(t.value_type), t.value_type
    if pa.types.is_date32(t):
        column = column.cast(pa.int32())
    vals = column.to_pylist()
    if pa.types.is_floating(t):
        return [None if v is None else ("f64", struct.unpack("<Q", struct.pack("<d", v))[0]) for v in vals]
    return vals


def minmax(column):
    """(min, max, valid, ascending, nondecreasing) of an integer column; min / max are None without a value.
    ascending = no NULL and k[i-1] < k[i] for every i >= 1; nondecreasing the same with <=.  One NULL-free row is both, a column with a
    NULL (or without a row) is neither."""
    return minmax_values(values_of(column))


def minmax_values(vals: list):
    """minmax() over the rows as values_of() gives them"""
    lo = hi = None
    valid = 0
    ascending = nondecreasing = len(vals) > 0
    prev = None
    for i, v in enumerate(vals):
        if v is None:
            ascending = nondecreasing = False
            prev = None
            continue
        valid += 1
        if lo is None or v < lo:
            lo = v
        if hi is None or v > hi:
            hi = v
        if i > 0 and prev is not None:
            if not prev < v:
                ascending = False
            if not prev <= v:
                nondecreasing = False
        prev = v
    return lo, hi, valid, ascending, nondecreasing


def in_list(column, max_size: int = 128 * 1024, max_distinct: int = 150):
    """the ascending distinct non-NULL values of a small integer column, or None beyond the limits of dfgpu_column_inlist:
    rows * width > max_size, more than max_distinct distinct values, max_distinct <= 0.  An empty table gives []."""
    vals = values_of(column)
    if len(vals) == 0:
        return []
    width = column.type.bit_width // 8
    if max_distinct <= 0 or len(vals) * width > max_size:
        return None
    seen = set()
    for v in vals:
        if v is not None:
            seen.add(v)
    out = sorted(seen)
    return None if len(out) > max_distinct else out


def _rows(table: pa.Table) -> list:
    cols = [values_of(table.column(i)) for i in range(table.num_columns)]
    return [tuple(c[r] for c in cols) for r in range(table.num_rows)]


def contains(build_keys: pa.Table, probe_keys: pa.Table, null_equality: str = "NullEqualsNothing") -> list:
    """one bool per probe row: does a build row carry the same key (column by column, by position)?  NullEqualsNothing: a row with a
    NULL component matches nothing; NullEqualsNull: NULL matches NULL in the same component.  Float64 keys compare by their bits."""
    assert build_keys.num_columns == probe_keys.num_columns and null_equality in ("NullEqualsNothing", "NullEqualsNull")
    null_matches = null_equality == "NullEqualsNull"
    have = set()
    for row in _rows(build_keys):
        if null_matches or all(v is not None for v in row):
            have.add(row)
    return [(null_matches or all(v is not None for v in row)) and row in have for row in _rows(probe_keys)]


def row_groups_kept(probe_table: pa.Table, row_group_size: int, key: str, bounds=None, in_list=None) -> list:
    """the row groups (of `row_group_size` rows each, in order) a scan must keep: those whose own [min, max] over the non-NULL keys
    meets the closed range `bounds` and holds room for one value of `in_list` (ascending).  A group without a non-NULL key has no
    min / max and is kept; an empty range (lo > hi) or an empty list keeps nothing; None = no such filter."""
    vals = values_of(probe_table.column(key))
    keep = []
    for g, start in enumerate(range(0, len(vals), row_group_size)):
        if bounds is not None and bounds[0] > bounds[1]:
            continue
        if in_list is not None and len(in_list) == 0:
            continue
        lo = hi = None
        for v in vals[start:start + row_group_size]:
            if v is None:
                continue
            if lo is None or v < lo:
                lo = v
            if hi is None or v > hi:
                hi = v
        if lo is not None:
            if bounds is not None and (hi < bounds[0] or lo > bounds[1]):
                continue
            if in_list is not None and not any(lo <= v <= hi for v in in_list):
                continue
        keep.append(g)
    return keep
