"""percent_rank, cume_dist, ntile and first_value / last_value / nth_value restated row at a time in plain Python: the truth
tests/test_window_value_reference.py holds to known answers and to tests/window_ref.py, and tests/test_gpu_window_value.py compares the
device operator with.  Python ints and `a / b` (one IEEE division of two ints below 2^53) only; no code shared with the library.  The
partition and peer boundaries are window_ref.boundaries.

With s / e the first / last row of the row's partition, rows = e - s + 1, ps / pe the first / last row of its peer group, i the row:
  percent_rank  (ps - s) / max(rows - 1, 1)
  cume_dist     (pe - s + 1) / rows
  ntile(n)      k = min(n, rows); (i - s) * k // rows + 1          (NOT "larger buckets first": 6 rows, n = 4 -> 1,1,2,3,3,4)
and over the frame [s, f], f = i (rows_to_current), pe (range_to_current, the default) or e (partition), RESPECT NULLS:
  first_value   the argument at s
  last_value    the argument at f
  nth_value(n)  n > 0: the argument at s + n - 1 if that is <= f, else None;  n < 0: the argument at f + n + 1 if that is >= s, else None
The picked argument is returned as it is (None = NULL)."""
from tests.window_ref import boundaries

DIST = ("percent_rank", "cume_dist", "ntile")
VALUE = ("first_value", "last_value", "nth_value")
FRAMES = ("range_to_current", "rows_to_current", "partition")


def positions(cols, partition_by, order_by, n):
    """per row (s, e, ps, pe)"""
    part_head = boundaries(cols, partition_by, n)
    peer_head = boundaries(cols, order_by, n, inside=part_head)
    out = [[0, 0, 0, 0] for _ in range(n)]
    for heads, at in ((part_head, 0), (peer_head, 2)):
        start = 0
        for i in range(n):
            if heads[i]:
                start = i
            out[i][at] = start
        end = n - 1
        for i in range(n - 1, -1, -1):
            if i == n - 1 or heads[i + 1]:
                end = i
            out[i][at + 1] = end
    return [tuple(p) for p in out]


def window(cols: dict, partition_by, order_by, exprs) -> dict:
    """cols = {name: list}, exprs = [(func | (func, n), argument column | None, name, frame | None)] -> {name: list}"""
    n = len(next(iter(cols.values()))) if cols else 0
    pos = positions(cols, partition_by, order_by, n)
    out = {}
    for func, arg, name, frame in exprs:
        func, param = func if isinstance(func, tuple) else (func, None)
        frame = "range_to_current" if frame is None else frame
        assert frame in FRAMES and func in DIST + VALUE, (func, frame)
        res = []
        for i, (s, e, ps, pe) in enumerate(pos):
            rows = e - s + 1
            if func == "percent_rank":
                res.append((ps - s) / max(rows - 1, 1))
            elif func == "cume_dist":
                res.append((pe - s + 1) / rows)
            elif func == "ntile":
                assert param >= 1
                res.append((i - s) * min(param, rows) // rows + 1)
            else:
                f = {"rows_to_current": i, "range_to_current": pe, "partition": e}[frame]
                if func == "first_value":
                    p = s
                elif func == "last_value":
                    p = f
                else:
                    assert param != 0
                    p = s + param - 1 if param > 0 else f + param + 1
                    if not s <= p <= f:
                        p = None
                res.append(None if p is None else cols[arg][p])
        out[name] = res
    return out
