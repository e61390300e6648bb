"""Reference for aggregates with FILTER (WHERE ...): a plain-Python restatement over lists of Python values, and the tables the
CPU and the GPU tests share.

The semantics (DataFusion's AggregateExec::filter_expr, GroupsAccumulator::update_batch opt_filter):
  * a row reaches an aggregate only where the aggregate's filter is True; False and None (NULL) both exclude it;
  * filters never decide which groups exist: every row that passes the NODE's predicate creates or joins its group;
  * a group none of whose rows reach an aggregate gives its "nothing seen" value: None, and 0 for COUNT;
  * COUNT(*) FILTER counts the rows where the filter is True, COUNT(x) FILTER those where x is not None as well;
  * without GROUP BY there is one output row, whatever is filtered out;
  * an aggregate without a filter is untouched by its neighbours' filters.

A table is {column name: list of Python values}; an aggregate is (func, argument column | None, output name, filter column | None):
arguments and filters are columns here, so that nothing of an expression evaluator is restated — a test that filters on an
expression puts the expression's truth values into a column of the table it hands to this module.

Values: Int32 / Int64 -> int, Decimal128 -> decimal.Decimal, Float64 -> float (integer-valued, every partial sum below 2^53: any
order of additions is exact), Boolean -> bool.  Results are exact: AVG over Decimal128(p, s) is the truncating division the reference's
DecimalAverager makes, at scale s + 4; AVG over the others is one IEEE division of the exact sum by the count; VAR / STDDEV are computed
in exact rationals and rounded once (their test inputs have dyadic means, so that a two-pass evaluation in doubles rounds at the
same single place)."""
import math
import random
from decimal import Decimal
from fractions import Fraction

FUNCS = ("sum", "min", "max", "count", "avg", "var_samp", "var_pop", "stddev_samp", "stddev_pop", "bit_and", "bit_or", "bit_xor", "bool_and", "bool_or")


def _avg(values):
    s = sum(values)
    if isinstance(s, Decimal):
        # DecimalAverager::avg: (sum * 10^(target scale - sum scale)) / count, truncating; target scale = s + 4
        scale = -values[0].as_tuple().exponent
        unscaled = int(s.scaleb(scale)) * 10**4
        q = abs(unscaled) // len(values)
        return Decimal(q if unscaled >= 0 else -q).scaleb(-(scale + 4))
    return float(s) / float(len(values))


def _variance(values, sample, root):
    n = len(values)
    if n - (1 if sample else 0) <= 0:
        return None                      # VAR_SAMP / STDDEV_SAMP of one value: NULL (variance.rs); VAR_POP of one value: 0.0
    xs = [Fraction(v) for v in values]
    mean = sum(xs) / n
    m2 = sum((x - mean) ** 2 for x in xs)
    assert float(m2) == m2, "the test inputs keep the sum of squared deviations exact in a double"
    v = float(m2) / float(n - 1 if sample else n)          # one rounding
    return math.sqrt(v) if root else v                      # and one more, correctly rounded on both sides


def reduce(func, values):
    """`func` over the non-None values that reached the aggregate, in row order; `values` may be empty"""
    if func == "count":
        return len(values)
    if not values:
        return None
    if func == "sum":
        s = sum(values)
        return float(s) if isinstance(values[0], float) else s
    if func == "min":
        return min(values)
    if func == "max":
        return max(values)
    if func == "avg":
        return _avg(values)
    if func in ("var_samp", "var_pop", "stddev_samp", "stddev_pop"):
        return _variance(values, func.endswith("samp"), func.startswith("stddev"))
    out = values[0]
    for v in values[1:]:
        if func in ("bit_and", "bool_and"):
            out = out & v
        elif func in ("bit_or", "bool_or"):
            out = out | v
        elif func == "bit_xor":
            out = out ^ v
        else:
            raise KeyError(func)
    return out


def aggregate(table, keys, aggs, predicate=None):
    """-> [{key columns..., output names...}], one dict per group in first-seen order.  `predicate`: the column of the node-level
    predicate (dfgpu_agg_update_filtered), rows where it is not True neither create groups nor reach any aggregate."""
    n = len(next(iter(table.values()))) if table else 0
    groups = {}
    for i in range(n):
        if predicate is not None and table[predicate][i] is not True:
            continue
        groups.setdefault(tuple(table[k][i] for k in keys), []).append(i)          # the group exists, whatever the filters say
    if not keys and not groups:
        groups[()] = []                                                            # no GROUP BY: one row even over nothing
    out = []
    for kt, rows in groups.items():
        row = dict(zip(keys, kt))
        for a in aggs:
            func, arg, name = a[:3]
            flt = a[3] if len(a) > 3 else None
            kept = [i for i in rows if flt is None or table[flt][i] is True]       # False and None both exclude the row
            if arg is None:
                values = [1] * len(kept)                                           # COUNT(*): the rows themselves
            else:
                values = [table[arg][i] for i in kept if table[arg][i] is not None]
            row[name] = reduce(func, values)
        out.append(row)
    return out


# ------------------------------------------------------------------------------ the shared tables
RUNS = (1, 63, 64, 65)               # run lengths of the group key: groups that straddle the 64-row words of a bitmap
ROW_COUNTS = (0, 1, 63, 64, 65, 4097)
FILTERS = ("p", "pf", "pt")          # FALSE / NULL / TRUE mixed, all FALSE, all TRUE


def run_gids(n):
    g, out = 0, []
    while len(out) < n:
        out += [g] * RUNS[g % len(RUNS)]
        g += 1
    return out[:n]


def make_table(n, seed=0):
    """n rows: the key `k` in runs of 1, 63, 64 and 65 rows; arguments i32 / i64 / f64 / dec / b (each nullable) and u (Int64 bit
    patterns); the filters p (FALSE, NULL and TRUE rows), pf (all FALSE), pt (all TRUE); `np_` a node predicate (mostly TRUE, some FALSE
    and NULL); `row` the row number.  Forced rows: every group g with g % 8 == 2 (64-row runs) and g % 8 == 4 (single rows) has no row
    where p is TRUE — its filtered aggregates see nothing while an unfiltered neighbour sees all of its rows; in every group of more than
    two rows the first row has p TRUE and NULL arguments, the second p NULL and arguments that are not NULL."""
    rng = random.Random(1000 * seed + n)
    gids = run_gids(n)
    t = {"k": [g * 3 - 40 for g in gids], "row": list(range(n))}
    def column(make, null_frac=0.15):
        return [None if rng.random() < null_frac else make() for _ in range(n)]
    t["i32"] = column(lambda: rng.randrange(-2**31, 2**31))
    t["i64"] = column(lambda: rng.randrange(-2**40, 2**40))
    t["f64"] = column(lambda: float(rng.randrange(-2**30, 2**30)))
    t["dec"] = column(lambda: Decimal(rng.randrange(-10**12, 10**12)).scaleb(-2))
    t["b"] = column(lambda: rng.random() < 0.5)
    t["u"] = column(lambda: rng.randrange(-2**63, 2**63))
    t["p"] = [rng.choice((True, True, False, None)) for _ in range(n)]
    t["pf"] = [False] * n
    t["pt"] = [True] * n
    t["np_"] = [rng.choice((True, True, True, True, False, None)) for _ in range(n)]
    start = 0
    while start < n:
        g = gids[start]
        end = start
        while end < n and gids[end] == g:
            end += 1
        if g % 8 in (2, 4):
            for i in range(start, end):
                t["p"][i] = rng.choice((False, None))
                t["np_"][i] = True
        elif end - start > 2:
            t["p"][start], t["p"][start + 1] = True, None
            t["np_"][start] = t["np_"][start + 1] = True
            for c in ("i32", "i64", "f64", "dec", "b", "u"):
                t[c][start] = None
            t["i32"][start + 1], t["i64"][start + 1], t["f64"][start + 1] = 7, -7, 7.0
            t["dec"][start + 1], t["b"][start + 1], t["u"][start + 1] = Decimal("7.07"), True, 0x55
        start = end
    return t


# the aggregates of the main tests: every function over every argument type; `sum_i64` and `cnt` share the filter p with most of
# the others, `plain_*` have no filter, `none_*` are filtered out entirely and `all_*` by a filter that is always TRUE
def main_aggs(flt="p"):
    aggs = []
    for typ in ("i32", "i64", "f64", "dec"):
        for func in ("sum", "min", "max", "count", "avg"):
            aggs.append((func, typ, f"{func}_{typ}", flt))
    aggs += [("count", None, "cnt", flt), ("count", None, "plain_cnt", None), ("sum", "i64", "plain_sum", None), ("count", "i64", "plain_count_i64", None),
             ("bit_and", "u", "and_u", flt), ("bit_xor", "u", "xor_u", flt), ("bool_and", "b", "band", flt), ("bool_or", "b", "bor", flt),
             ("sum", "i64", "none_sum", "pf"), ("count", None, "none_cnt", "pf"), ("max", "dec", "all_max", "pt"), ("count", None, "all_cnt", "pt")]
    return aggs


def variance_table():
    """VAR / STDDEV under a filter, exactly: the rows a filter keeps are 0, 1, 2 or 4 small integers per group, so the mean is
    dyadic, every deviation and square is an exact double and the result rounds once (the division) or twice (the root)."""
    rows = []   # (k, x, p)
    def group(k, kept, dropped):
        for x in kept:
            rows.append((k, x, True))
        for x, p in dropped:
            rows.append((k, x, p))
    group(1, [1.0, 3.0], [(100.0, False), (-50.0, None)])
    group(2, [2.0, 4.0, 6.0, 8.0], [(1000.0, False)])
    group(3, [5.0], [(9.0, None), (11.0, False)])                 # one value: VAR_SAMP NULL, VAR_POP 0.0
    group(4, [], [(1.0, False), (2.0, None)])                     # nothing reaches the aggregate: NULL
    group(5, [10.0, None, 14.0], [(None, False)])                 # a NULL argument where the filter is TRUE
    group(6, [-3.0, -1.0, 1.0, 7.0], [])
    order = list(range(len(rows)))
    random.Random(5).shuffle(order)
    rows = [rows[i] for i in order]
    return {"k": [r[0] for r in rows], "x": [r[1] for r in rows], "p": [r[2] for r in rows]}
