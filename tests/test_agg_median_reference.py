"""tests/median_ref.py, the restatement the GPU MEDIAN is held to, held to something itself: the hand-worked answers of the contract
(include/dfgpu.h), `statistics.median_low` / `median_high` for the two middles, numpy.median where the middles average exactly — and,
for each mistake an implementation is likely to make, a table on which that mistake gives another answer than the restatement."""
import math
import random
import statistics

import numpy as np

from tests import edge_values as E
from tests import median_ref as R

B = R.f64_bits


def test_the_contract_examples():
    assert R.median([2147483647, 2147483647], "i32") == -1                     # the sum wraps at 32 bits: -2 / 2
    assert R.median([200, 200], "u8") == 72                                    # 400 mod 256 = 144, / 2
    assert R.median([-3, 0], "i64") == -1                                      # truncation toward zero, not a floor (-2)
    assert R.median([2**63 - 1, 2**63 - 1], "i64") == -1
    assert R.median([2**32 - 1, 2**32 - 1], "u32") == 2**31 - 1                 # (2^33 - 2) mod 2^32 = 2^32 - 2
    assert R.median([2**64 - 1, 1], "u64") == 0
    assert R.median([10**38 - 1, 10**38 - 1], "dec") == (2 * (10**38 - 1) - 2**128) // 2   # wraps at 128 bits (the sum is even)
    assert R.median([-3, 0], "dec") == -1
    assert R.median([B(1e308), B(1e308)], "f64") == B(math.inf)                 # the addition overflows before the division
    assert R.median([], "i64") is None and R.median([None, None], "f64") is None
    assert R.median([5, None, 1, 9], "i32") == 5 and R.median([None, 7], "u8") == 7
    assert R.median([1, 2, 3, 4], "i32") == 2 and R.median([-1, -2, -3, -4], "i32") == -2  # 5 / 2 = 2, -5 / 2 = -2


def test_float64_total_order_and_unchanged_bits():
    nz, pz = B(-0.0), B(0.0)
    assert R.ordered([pz, nz, E.QNAN_BITS, B(-math.inf), E.NEG_QNAN_BITS, B(1.0), E.PAYLOAD_NAN_BITS], "f64") == \
        [E.NEG_QNAN_BITS, B(-math.inf), nz, pz, B(1.0), E.QNAN_BITS, E.PAYLOAD_NAN_BITS]
    assert R.median([pz, nz, pz], "f64") == pz and R.median([nz, nz, pz], "f64") == nz     # -0.0 survives, and sorts below +0.0
    assert R.median([E.PAYLOAD_NAN_BITS], "f64") == E.PAYLOAD_NAN_BITS                      # a payload survives an odd count
    assert R.median([B(1.0), E.QNAN_BITS, E.PAYLOAD_NAN_BITS], "f64") == E.QNAN_BITS        # +NaN is above every number
    assert R.median([E.NEG_QNAN_BITS, B(-5.0), B(7.0)], "f64") == B(-5.0)                   # -NaN below
    assert R.median([nz, pz], "f64") == pz                                                  # -0.0 + 0.0 = +0.0
    assert R.median([nz, nz], "f64") == nz
    assert R.median([B(math.inf), B(-math.inf)], "f64") is R.COMPUTED_NAN
    assert R.median([B(1.0), E.QNAN_BITS], "f64") is R.COMPUTED_NAN
    assert R.median([B(5e-324), B(5e-324)], "f64") == B(5e-324) and R.median([B(5e-324), B(0.0)], "f64") == B(0.0)   # 5e-324 / 2 rounds to even
    assert R.same(E.QNAN_BITS, R.COMPUTED_NAN) and R.same(E.NEG_QNAN_BITS, R.COMPUTED_NAN) and not R.same(B(1.0), R.COMPUTED_NAN) and not R.same(None, R.COMPUTED_NAN)
    assert not R.same(None, 0) and not R.same(0, None) and R.same(None, None)


def test_the_two_middles_are_those_of_the_statistics_module():
    rng = random.Random(11)
    for t, lo, hi in (("i32", -2**31, 2**31 - 1), ("i64", -2**63, 2**63 - 1), ("u8", 0, 255), ("u32", 0, 2**32 - 1), ("u64", 0, 2**64 - 1), ("dec", -10**38 + 1, 10**38 - 1)):
        for c in list(range(1, 12)) + [63, 64, 65, 1000, 1001]:
            values = [rng.choice((lo, hi, 0, 1)) if rng.random() < 0.2 else rng.randint(lo, hi) for _ in range(c)]
            a, b = statistics.median_low(values), statistics.median_high(values)
            want = a if c % 2 else R.wrap(R.div2(R.wrap(a + b, t)), t)
            nulled = values + [None] * 3
            rng.shuffle(nulled)
            assert R.median(nulled, t) == want, (t, c)
            if c % 2 == 0 and -2**62 < a + b < 2**62 and t in ("i64", "dec") and (a + b) % 2 == 0:
                assert want == (a + b) // 2


def test_numpy_median_where_the_middles_average_exactly():
    rng = np.random.default_rng(5)
    for c in (1, 2, 3, 4, 63, 64, 65, 1000, 1001):
        x = rng.integers(-4000, 4000, c) / 8.0                                  # dyadic: the sum and its half are exact
        assert R.median([B(float(v)) for v in x], "f64") == B(float(np.median(x))), c
    x = np.array([-1.5, -0.25, 3.0, 1e300, -1e300, 2.0**-1070])
    assert R.median([B(float(v)) for v in x], "f64") == B(float(np.median(x)))


# ------------------------------------------------------------------------------------------------ the mistakes and the tables that catch them
def _wrong(table, keys, arg, t, flt=None, *, floor=False, wide_sum=False, upper=False, count_nulls=False, ieee_lt=False, ignore_filter=False, whole=False):
    out = []
    for _, rows in R.groups_of(table, [] if whole else keys):
        rows = [i for i in rows if ignore_filter or R.passes(table, flt, i)]
        values = [table[arg][i] for i in rows if table[arg][i] is not None]
        if ieee_lt:                                                              # a comparison sort with `<` on doubles
            import functools
            values = sorted(values, key=functools.cmp_to_key(lambda a, b: -1 if R.f64(a) < R.f64(b) else 1 if R.f64(b) < R.f64(a) else 0))
        else:
            values = R.ordered(values, t)
        c = len(rows) if count_nulls else len(values)
        values = values + [values[-1]] * (c - len(values)) if values else values  # (NULLs counted: the positions move)
        if not values:
            out.append(None)
        elif c % 2 or upper:
            out.append(values[c // 2])
        elif t == "f64":
            out.append(R.middle(values, t))
        else:
            s = values[c // 2 - 1] + values[c // 2]
            s = s if wide_sum else R.wrap(s, t)
            out.append(R.wrap(s // 2 if floor else R.div2(s), t))
    return out * (len(R.groups_of(table, keys)) if whole else 1)


def _right(table, keys, arg, t, flt=None):
    return [r["m"] for r in R.aggregate(table, keys, [("median", arg, "m", flt)], {arg: t})]


def test_each_mistake_differs_on_its_table():
    k = [1, 1, 2, 2, 2]
    cases = [
        ("floor", {"k": k, "x": [-3, 0, 1, 2, 3]}, "i64", None, dict(floor=True)),
        ("wide_sum", {"k": k, "x": [2**31 - 1, 2**31 - 1, 1, 2, 3]}, "i32", None, dict(wide_sum=True)),
        ("wide_sum", {"k": k, "x": [200, 200, 1, 2, 3]}, "u8", None, dict(wide_sum=True)),
        ("upper", {"k": k, "x": [10, 20, 1, 2, 3]}, "i64", None, dict(upper=True)),
        ("count_nulls", {"k": k, "x": [10, 20, 1, 5, None]}, "i64", None, dict(count_nulls=True)),
        ("ieee_lt", {"k": k, "x": [B(0.0), B(-0.0), E.QNAN_BITS, B(1.0), B(2.0)]}, "f64", None, dict(ieee_lt=True)),
        ("ieee_lt", {"k": k, "x": [B(1.0), B(2.0), B(0.0), B(-0.0), B(1.0)]}, "f64", None, dict(ieee_lt=True)),
        ("ignore_filter", {"k": k, "x": [10, 20, 1, 2, 30], "p": [True, False, True, None, True]}, "i64", "p", dict(ignore_filter=True)),
        ("whole", {"k": k, "x": [10, 20, 1, 2, 3]}, "i64", None, dict(whole=True)),
    ]
    seen = set()
    for name, table, t, flt, bug in cases:
        right, wrong = _right(table, ["k"], "x", t, flt), _wrong(table, ["k"], "x", t, flt, **bug)
        assert _wrong(table, ["k"], "x", t, flt) == right, name                  # the harness itself, without a mistake, is the restatement
        assert wrong != right, (name, right)
        seen.add(name)
    assert seen == {"floor", "wide_sum", "upper", "count_nulls", "ieee_lt", "ignore_filter", "whole"}


def test_the_generated_tables_have_the_groups_the_gpu_test_counts_on():
    t = R.make_table(4097)
    sizes = {}
    for key, rows in R.groups_of(t, ["k"]):
        sizes[key] = len(rows)
    assert {1, 2, 3, 4} <= set(sizes.values())
    want = R.aggregate(t, ["k"], [("median", name, name, None) for name in R.MEDIAN_TYPES], R.TYPES)
    assert any(all(r[name] is None for name in R.MEDIAN_TYPES) for r in want)                      # the all-NULL group
    for name in R.MEDIAN_TYPES:
        pairs = [e for a in R.EDGES[name] for b in R.EDGES[name] for e in (a, b)]                      # the cross product opens the column
        head = t[name][:len(pairs)]
        assert all(v is None or v == p for v, p in zip(head, pairs)) and sum(v is not None for v in head) > len(head) // 2, name
        back = R.raw_column(R.column(t[name], name), name)
        assert back == t[name], name                                             # Arrow in and out loses nothing, bit patterns included
