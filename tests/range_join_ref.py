"""The truth the range join tests compare with: dfgpu_range_join (include/dfgpu.h) a row at a time, in plain Python.

A pair (l, r) matches when x[r] is not NULL and every bound that is present holds: a[l] is not NULL and a[l] <(=) x[r]; b[l] is not
NULL and x[r] <(=) b[l].  Values are compared as Python integers; Float64 by tests/expr_ref.py's total-order key of its bits
(-NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN).  The output order is the entry point's:

  Inner / Left / Right / Full   the matching pairs in LEFT-row-major order: ascending left row; within one left row ascending x in the
                                key order, equal x by ascending right row; then the unmatched right rows, ascending (Right / Full);
                                then the unmatched left rows, ascending (Left / Full)
  LeftSemi / LeftAnti / LeftMark   left-row order;      RightSemi / RightAnti / RightMark   right-row order

The non-NULL x are sorted once and a left row's matches are read off between two bisections, so the cost is linear in the output; the
join types and the materialisation are tests/nlj_ref.py's.  tests/test_range_join_reference.py holds this file to the pair-space
reference (nlj_ref.nested_loop_join with the equivalent JoinFilter) on every case small enough for it."""
import bisect

import numpy as np
import pyarrow as pa

from tests import expr_ref, nlj_ref


def key_values(col):
    """a key column as comparable Python integers, None = NULL: integers and dates by value, Float64 by the total-order key of its bits"""
    col = nlj_ref._flat(col)
    if pa.types.is_float64(col.type):
        bits = np.frombuffer(col.buffers()[1], dtype=np.uint64)[col.offset:col.offset + len(col)]
        valid = col.is_valid().to_pylist()
        return [expr_ref.total_key(int(b)) if ok else None for b, ok in zip(bits, valid)]
    if pa.types.is_date32(col.type):
        col = col.cast(pa.int32())
    assert pa.types.is_integer(col.type), f"{col.type} is not a range join key type"
    return col.to_pylist()


def _index(table, c):
    return c if isinstance(c, int) else table.schema.get_field_index(c)


def matching_pairs(left, right, x, lower=None, upper=None):
    """[(left row, right row)] of the matching pairs in the entry point's order"""
    assert lower is not None or upper is not None, "a range join needs a lower or an upper bound"
    xs = key_values(right.column(_index(right, x)))
    a = None if lower is None else key_values(left.column(_index(left, lower[0])))
    b = None if upper is None else key_values(left.column(_index(left, upper[0])))
    order = sorted((r for r in range(right.num_rows) if xs[r] is not None), key=lambda r: (xs[r], r))
    keys = [xs[r] for r in order]
    pairs = []
    for l in range(left.num_rows):
        if (a is not None and a[l] is None) or (b is not None and b[l] is None):
            continue
        lo = 0 if a is None else (bisect.bisect_left(keys, a[l]) if lower[1] else bisect.bisect_right(keys, a[l]))
        hi = len(keys) if b is None else (bisect.bisect_right(keys, b[l]) if upper[1] else bisect.bisect_left(keys, b[l]))
        pairs.extend((l, order[p]) for p in range(lo, hi))
    return pairs


def range_join(left, right, x, lower=None, upper=None, join_type="Inner", left_cols=None, right_cols=None, pairs=None):
    """`pairs` = matching_pairs(left, right, x, lower, upper) when the caller has them already (they are the same for every join type)"""
    if pairs is None:
        pairs = matching_pairs(left, right, x, lower, upper)
    li, ri, marks = nlj_ref.index_rows(left.num_rows, right.num_rows, pairs, join_type)
    return nlj_ref.materialise(left, right, li, ri, marks, join_type, left_cols, right_cols)


difference = nlj_ref.difference
multiset = nlj_ref.multiset
