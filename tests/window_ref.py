"""WindowAggExec restated row at a time in plain Python: the truth tests/test_window_reference.py holds to known answers and to the
oracle, and tests/test_gpu_window.py compares the device operator with.  Python ints and Fractions only; no code shared with the library.

Input rows are already ordered by (partition keys, order keys); only equality of neighbouring rows is looked at.
  partition  = maximal run of adjacent rows whose partition keys are all equal (None equals None); no keys: everything
  peer group = maximal run of adjacent rows of one partition whose order keys are all equal (None equals None); no keys: the partition
  row_number = 1-based position in the partition; rank = position of the peer group's first row; dense_rank = peer groups so far
  sum / count / min / max / avg over a frame that starts at the partition's first row and ends at
      rows_to_current: the row itself;  range_to_current: the row's last peer;  partition: the partition's last row
  None arguments are skipped; a frame without a value gives None (count: 0); count without an argument counts rows.

Values: ints for the integer types, Date32 (days) and Decimal128 (UNSCALED), floats for Float64, None for NULL.  Types are tags:
"int32" "int64" "uint8" "uint32" "uint64" "date32" "float64" or ("decimal", precision, scale).  Results:
  sum     int32 / int64 / uint8 -> wraps to Int64; uint32 / uint64 -> wraps to UInt64; decimal -> unscaled, wraps at 128 bits
          (precision + 10, same scale); float64 -> FloatSum (the exact rational sum, what a double summation is held to)
  avg     int32 / int64 -> the correctly rounded double of sum / count (asserts |sum| < 2^53: then a double summation is exact);
          float64 -> FloatSum; decimal -> unscaled at scale + 4 (capped at 38), (sum * 10^k) / count truncated toward zero
  min/max the argument's type; float64 ordered by IEEE totalOrder (-NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN)
"""
import struct
from fractions import Fraction

RANKING = ("row_number", "rank", "dense_rank")
FRAMES = ("range_to_current", "rows_to_current", "partition")


class FloatSum:
    """a Float64 frame's truth: `exact` = the rational sum of its m non-NULL values, S = the sum of their magnitudes"""
    __slots__ = ("exact", "S", "m")

    def __init__(self, exact, S, m):
        self.exact, self.S, self.m = exact, S, m

    def __eq__(self, other):
        return isinstance(other, FloatSum) and (self.exact, self.S, self.m) == (other.exact, other.S, other.m)

    def __repr__(self):
        return f"FloatSum({float(self.exact)!r}, m={self.m})"


def total_order_key(x: float) -> int:
    b = struct.unpack("<q", struct.pack("<d", x))[0]
    return b ^ (((b >> 63) & 0xFFFFFFFFFFFFFFFF) >> 1)


def _wrap(v: int, bits: int, signed: bool) -> int:
    v &= (1 << bits) - 1
    return v - (1 << bits) if signed and v >> (bits - 1) else v


def boundaries(cols, keys, n, inside=None):
    """head[i] = row i starts a run of equal `keys` (or `inside`[i] is set: runs never cross the enclosing runs' heads)"""
    head = []
    for i in range(n):
        h = i == 0 or (inside is not None and inside[i])
        if not h:
            for k in keys:
                a, b = cols[k][i - 1], cols[k][i]
                if (a is None) != (b is None) or (a is not None and a != b):
                    h = True
                    break
        head.append(h)
    return head


class _Running:
    """one partition's aggregate, fed its rows' arguments in row order (None = NULL); value() = the aggregate over the rows fed so far.
    func count with typ None counts rows."""

    def __init__(self, func, typ):
        self.func, self.typ, self.rows, self.m = func, typ, 0, 0
        self.sum, self.S, self.best = 0, 0, None
        if typ == "float64":
            self.sum, self.S = Fraction(0), Fraction(0)

    def feed(self, v):
        self.rows += 1
        if v is None:
            return
        self.m += 1
        if self.func in ("sum", "avg"):
            if self.typ == "float64":
                self.sum += Fraction(v)
                self.S += abs(Fraction(v))
            else:
                self.sum += v
        elif self.func in ("min", "max"):
            key = total_order_key if self.typ == "float64" else (lambda x: x)
            if self.best is None or (key(v) < key(self.best) if self.func == "min" else key(v) > key(self.best)):
                self.best = v

    def value(self):
        func, typ, dec = self.func, self.typ, isinstance(self.typ, tuple)
        if func == "count":
            return self.rows if typ is None else self.m
        if self.m == 0:
            return None
        if func in ("min", "max"):
            if not (typ == "float64" or dec or typ in ("int32", "int64", "uint8", "uint32", "date32")):
                raise TypeError(f"{func} over {typ}")
            return self.best
        if typ == "float64":
            return FloatSum(self.sum, self.S, self.m)
        if func == "sum":
            if dec:
                return _wrap(self.sum, 128, True)
            if typ in ("int32", "int64", "uint8"):
                return _wrap(self.sum, 64, True)
            if typ in ("uint32", "uint64"):
                return _wrap(self.sum, 64, False)
        if func == "avg":
            if dec:
                k = min(38, typ[2] + 4) - typ[2]
                s = _wrap(self.sum, 128, True) * 10 ** k
                q = abs(s) // self.m
                return q if s >= 0 else -q
            if typ in ("int32", "int64"):
                assert abs(self.sum) < 2 ** 53, "keep integer AVG inputs where a double summation is exact"
                return float(Fraction(self.sum, self.m))
        raise TypeError(f"{func} over {typ}")


def window(cols: dict, types: dict, partition_by, order_by, exprs) -> dict:
    """cols = {name: list}, exprs = [(func, argument column | None, name, frame | None)] -> {name: list}"""
    n = len(next(iter(cols.values()))) if cols else 0
    part_head = boundaries(cols, partition_by, n)
    peer_head = boundaries(cols, order_by, n, inside=part_head)
    ends = {}
    for which, head in (("partition", part_head), ("range_to_current", peer_head)):      # the last row before the next head
        e = [0] * n
        for i in range(n - 1, -1, -1):
            e[i] = i if i == n - 1 or head[i + 1] else e[i + 1]
        ends[which] = e
    out = {}
    for func, arg, name, frame in exprs:
        frame = "range_to_current" if frame is None else frame
        assert frame in FRAMES and (func in RANKING or func in ("sum", "count", "min", "max", "avg"))
        res = []
        start = peer_start = dense = 0
        running = []      # of the current partition: running[j - start] = the aggregate over rows start .. j
        for i in range(n):
            if part_head[i]:
                start, dense = i, 0
                if func not in RANKING:
                    acc, running, j = _Running(func, None if arg is None else types[arg]), [], i
                    while j < n and (j == i or not part_head[j]):
                        acc.feed(None if arg is None else cols[arg][j])
                        running.append(acc.value())
                        j += 1
            if peer_head[i]:
                peer_start, dense = i, dense + 1
            if func == "row_number":
                res.append(i - start + 1)
            elif func == "rank":
                res.append(peer_start - start + 1)
            elif func == "dense_rank":
                res.append(dense)
            else:
                end = i if frame == "rows_to_current" else ends[frame][i]
                res.append(running[end - start])
        out[name] = res
    return out
