"""The truth the nested-loop join tests compare with: the join a row at a time, in plain Python.

The |L| x |R| intermediate table of the filter's columns is built in right-row-major order, the pairs whose filter value is TRUE come
from tests/expr_ref.py's `filter_rows` (the exact expression reference), and the ten join types and the output order of
dfgpu_nested_loop_join (include/dfgpu.h) are put together from Python lists:

  Inner / Left / Right / Full   the passing pairs, ascending right row and ascending left row within one right row; then the unmatched
                                right rows, ascending (Right / Full); then the unmatched left rows, ascending (Left / Full)
  RightSemi / RightAnti / RightMark   right-row order;      LeftSemi / LeftAnti / LeftMark   left-row order

A filter is (expression in the oracle's tuple form over f0, f1, ..., [(column index, "Left" | "Right"), ...]) or None (every pair
passes).  One form expr_ref does not have is added here: ("like", column name, pattern) over a dictionary-encoded or string column —
SQL LIKE with % and _ on the decoded strings, NULL for a NULL row."""
import re
import struct

import pyarrow as pa

from tests import expr_ref

PAIR_TYPES = ("Inner", "Left", "Right", "Full")
LEFT_ONE_SIDED = ("LeftSemi", "LeftAnti", "LeftMark")
RIGHT_ONE_SIDED = ("RightSemi", "RightAnti", "RightMark")
ALL_TYPES = PAIR_TYPES + ("LeftSemi", "RightSemi", "LeftAnti", "RightAnti", "LeftMark", "RightMark")


def _flat(col):
    col = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    return col


def _take(col, idx):
    return _flat(col).take(pa.array(idx, type=pa.int64()))


def _like_values(col, pattern):
    col = _flat(col)
    if pa.types.is_dictionary(col.type):
        col = col.cast(pa.string())
    rx = re.compile("".join(".*" if ch == "%" else "." if ch == "_" else re.escape(ch) for ch in pattern) + r"\Z", re.S)
    return [None if s is None else rx.match(s) is not None for s in col.to_pylist()]


def _values(expr, table):
    """expr_ref.evaluate plus the ("like", column, pattern) leaf under not / and / or"""
    if expr[0] == "like":
        return _like_values(table.column(expr[1]), expr[2])
    if expr[0] == "not" and expr[1][0] == "like":
        return [None if v is None else not v for v in _values(expr[1], table)]
    if expr[0] == "bin" and expr[1] in ("and", "or") and ("like" in (expr[2][0], expr[3][0])):
        return [expr_ref._kleene(expr[1], a, b) for a, b in zip(_values(expr[2], table), _values(expr[3], table))]
    return expr_ref._decided(expr_ref.evaluate(expr, table).vals, "a join filter")


def pair_values(left: pa.Table, right: pa.Table, join_filter):
    """[(left row, right row, value)] for every pair in right-row-major order; value is True, False or None (NULL)"""
    nl, nr = left.num_rows, right.num_rows
    li = [l for _ in range(nr) for l in range(nl)]
    ri = [r for r in range(nr) for _ in range(nl)]
    if join_filter is None:
        return [(l, r, True) for l, r in zip(li, ri)]
    expr, cols = join_filter
    arrays = {"__pair": pa.array(range(len(li)), type=pa.int64())}    # a table without columns has no rows: literal-only filters need them
    for k, (i, side) in enumerate(cols):
        arrays[f"f{k}"] = _take((left if side == "Left" else right).column(int(i)), li if side == "Left" else ri)
    vals = _values(expr, pa.table(arrays))
    assert len(vals) == len(li)
    return list(zip(li, ri, vals))


def passing_pairs(left, right, join_filter):
    """[(left row, right row)] of the pairs whose filter value is TRUE, in right-row-major order"""
    return [(l, r) for l, r, v in pair_values(left, right, join_filter) if v is True]


def index_rows(nl, nr, passing, join_type):
    """(left row ids, right row ids, marks): one entry per output row, None = the NULL-extended side; marks only for the Mark types"""
    l_hit, r_hit = [False] * nl, [False] * nr
    for l, r in passing:
        l_hit[l] = True
        r_hit[r] = True
    if join_type in PAIR_TYPES:
        li, ri = [l for l, _ in passing], [r for _, r in passing]
        if join_type in ("Right", "Full"):
            un = [r for r in range(nr) if not r_hit[r]]
            li, ri = li + [None] * len(un), ri + un
        if join_type in ("Left", "Full"):
            un = [l for l in range(nl) if not l_hit[l]]
            li, ri = li + un, ri + [None] * len(un)
        return li, ri, None
    hit, n = (l_hit, nl) if join_type in LEFT_ONE_SIDED else (r_hit, nr)
    if join_type.endswith("Semi"):
        rows, marks = [i for i in range(n) if hit[i]], None
    elif join_type.endswith("Anti"):
        rows, marks = [i for i in range(n) if not hit[i]], None
    else:
        rows, marks = list(range(n)), list(hit)
    return (rows, None, marks) if join_type in LEFT_ONE_SIDED else (None, rows, marks)


def materialise(left, right, li, ri, marks, join_type, left_cols=None, right_cols=None):
    lc = list(range(left.num_columns)) if left_cols is None else [c if isinstance(c, int) else left.schema.get_field_index(c) for c in left_cols]
    rc = list(range(right.num_columns)) if right_cols is None else [c if isinstance(c, int) else right.schema.get_field_index(c) for c in right_cols]
    if join_type in LEFT_ONE_SIDED:
        rc = []
    if join_type in RIGHT_ONE_SIDED:
        lc = []
    arrays = [_take(left.column(c), li) for c in lc] + [_take(right.column(c), ri) for c in rc]
    names = [left.schema.names[c] for c in lc] + [right.schema.names[c] for c in rc]
    if marks is not None:
        arrays.append(pa.array(marks, type=pa.bool_()))
        names.append("mark")
    return pa.Table.from_arrays(arrays, names=names)


def nested_loop_join(left, right, join_type="Inner", join_filter=None, left_cols=None, right_cols=None, passing=None):
    """`passing` = passing_pairs(left, right, join_filter) when the caller has it already (it is the same for every join type)"""
    if passing is None:
        passing = passing_pairs(left, right, join_filter)
    li, ri, marks = index_rows(left.num_rows, right.num_rows, passing, join_type)
    return materialise(left, right, li, ri, marks, join_type, left_cols, right_cols)


# ------------------------------------------------------------------------------------------------------------------ comparison
def _cells(col):
    """a column as comparable Python values: Float64 by its bits, dictionary-encoded strings as strings, None = NULL"""
    col = _flat(col)
    if pa.types.is_dictionary(col.type):
        col = col.cast(col.type.value_type)
    if pa.types.is_large_string(col.type):
        col = col.cast(pa.string())
    if pa.types.is_float64(col.type):
        return [None if v is None else struct.unpack("<q", struct.pack("<d", v))[0] for v in col.to_pylist()], "float64 bits"
    return col.to_pylist(), str(col.type)


def difference(got: pa.Table, want: pa.Table):
    """None when the tables agree position by position (names, value types, validity, values; Float64 by bits), else the first difference"""
    if got.column_names != want.column_names:
        return f"columns {got.column_names} != {want.column_names}"
    if got.num_rows != want.num_rows:
        return f"{got.num_rows} rows != {want.num_rows}"
    for name, g, w in zip(got.column_names, got.columns, want.columns):
        (gv, gt), (wv, wt) = _cells(g), _cells(w)
        if gt != wt:
            return f"column {name}: type {gt} != {wt}"
        for i, (a, b) in enumerate(zip(gv, wv)):
            if a != b:
                return f"column {name} row {i}: got {a!r}, want {b!r}"
    return None


def multiset(table: pa.Table):
    """the rows as a sorted list (order-insensitive comparison form), Float64 by bits"""
    cols = [_cells(c)[0] for c in table.columns]
    key = lambda row: tuple((v is None, 0 if v is None else v) for v in row)
    return sorted((tuple(c[i] for c in cols) for i in range(table.num_rows)), key=key)
