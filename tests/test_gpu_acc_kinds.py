"""Every accumulator kind of the GPU AggregateExec at once, on every accumulation site (the plans of tests/test_gpu_float_sums.py, whose
profile name must show in ops.profile_stats()): SUM over Int64, over Decimal128(15,2), over Decimal128(38,4) with values beyond 64 bits
and over Float64, MIN(Int64), MAX(Float64), COUNT(x), COUNT(*), bit_and / bit_or / bit_xor over Int64 — one accumulator of each kind
side by side in one call, so a site that takes one kind's neutral element, atomic, fold or scan for another's shows here.

The reference is Python integers and numpy over the group numbers; everything is compared exactly.  The Float64 column holds
integer-valued doubles with |v| < 2^20, so its sums are exact in any order of addition and are compared by their bits; Decimals are
compared as unscaled integers.  Sizes and NULL fractions are those of test_gpu_bitwise.BOOL_CASES: 4097 rows where the plan has that
size (the smallest that crosses the wave, word and window edges), else the plan's first size; no NULLs and about 10 %."""
import functools
import struct
from decimal import Decimal

import numpy as np
import pyarrow as pa
import pytest

from tests import bitwise_ref as B
from tests.test_gpu_bitwise import Spec, _family_specs, _keys, _run_plan
from tests.test_gpu_float_sums import PLANS, _shape

pytestmark = pytest.mark.gpu

D15, D38 = pa.decimal128(15, 2), pa.decimal128(38, 4)
# output name -> (function, input column); "rows" is COUNT(*)
AGGS = {"si": ("sum", "i"), "s15": ("sum", "d15"), "s38": ("sum", "d38"), "sf": ("sum", "f"), "mn": ("min", "i"), "mx": ("max", "f"), "cx": ("count", "i"),
        "rows": ("count", None), "a": ("bit_and", "a_in"), "o": ("bit_or", "o_in"), "x": ("bit_xor", "i")}
# One list per plan: all eleven.  A plan listed here takes another site than the one it names when it is handed all eleven at once (seen
# at the commit before this file as well), so its list is cut in two and every kind still passes the named site.
SPLIT = {}
CASES = sorted({(p.shape, 4097 if 4097 in p.sizes else p.sizes[0], nf, name) for name, p in PLANS.items() for nf in (0.0, B.NULL_FRACTIONS[-1])})


def _f64_bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def _decimal(unscaled, scale):
    """exact at any width (Decimal.scaleb and arithmetic round to the context's 28 digits)"""
    return Decimal((int(unscaled < 0), tuple(map(int, str(abs(unscaled)))), -scale))


def _unscaled(value, scale):
    sign, digits, exponent = value.as_tuple()
    assert exponent == -scale, (value, scale)
    return (-1 if sign else 1) * int("".join(map(str, digits)))


def _decimal_array(unscaled, valid, typ):
    return pa.array([_decimal(int(v), typ.scale) if ok else None for v, ok in zip(unscaled, valid)], typ)


@functools.lru_cache(maxsize=4)
def _case(shape, n, null_frac):
    """the input table of a (shape, size, NULL fraction) and {key tuple: {output name: exact result}}"""
    rng = np.random.default_rng([n, sum(map(ord, shape)), int(null_frac * 100)])
    gids, keys = _shape(shape, n, rng)
    n = len(gids)
    dead = B.all_null_group(gids) if null_frac > 0 else None       # the group bitwise_ref.family leaves without a value: without one here too

    def valid():
        v = rng.random(n) >= null_frac
        if dead is not None:
            v[gids == dead] = False
        return v
    ints = rng.integers(-2**40, 2**40, n)
    ints[rng.permutation(n)[:4]] = [2**40, -2**40, 0, -1]
    d15 = rng.integers(-10**14, 10**14, n)
    d38 = np.array([int(hi) * 2**64 + int(lo) for hi, lo in zip(rng.integers(-2**36, 2**36, n), rng.integers(0, 2**63, n))], object)     # |v| < 2^100 < 10^31
    flt = rng.integers(-2**20 + 1, 2**20, n).astype(np.float64)
    vi, v15, v38, vf = valid(), valid(), valid(), valid()
    bits = _family_specs(gids, null_frac, [("a", "bit_and", pa.int64()), ("o", "bit_or", pa.int64())])
    mask = (lambda v: ~v) if null_frac > 0 else (lambda v: None)           # (no NULLs: no validity bitmap either, as bitwise_ref.to_arrow makes its columns)
    table = pa.table({**keys, "i": pa.array(ints, pa.int64(), mask=mask(vi)), "d15": _decimal_array(d15, v15, D15), "d38": _decimal_array(d38, v38, D38),
                      "f": pa.array(flt, pa.float64(), mask=mask(vf)), "a_in": bits[0].arrow(), "o_in": bits[1].arrow(), "row": pa.array(np.arange(n, dtype=np.int64))})
    key_rows = list(zip(*[keys[k].to_pylist() for k in keys])) if keys else [()] * n
    ids = {}
    gnum = np.array([ids.setdefault(k, len(ids)) for k in key_rows], np.int64)
    by_bits = {s.name: B.reduce_groups(s.func, gnum, s.values, s.valid, s.typ) for s in bits + [Spec("x", "bit_xor", pa.int64(), ints, vi)]}
    order = np.argsort(gnum, kind="stable")
    bounds = np.r_[0, np.cumsum(np.bincount(gnum, minlength=len(ids)))]
    want = {}
    for kt, g in ids.items():
        idx = order[bounds[g]:bounds[g + 1]]
        i_, d15_, d38_, f_ = ints[idx][vi[idx]], d15[idx][v15[idx]], d38[idx][v38[idx]], flt[idx][vf[idx]]
        want[kt] = {"si": sum(map(int, i_)) if len(i_) else None, "s15": sum(map(int, d15_)) if len(d15_) else None, "s38": sum(d38_) if len(d38_) else None,
                    "sf": _f64_bits(float(sum(map(int, f_)))) if len(f_) else None, "mn": int(i_.min()) if len(i_) else None,
                    "mx": _f64_bits(float(f_.max())) if len(f_) else None, "cx": len(i_), "rows": len(idx), **{name: red[g] for name, red in by_bits.items()}}
    return table, list(keys), want


def _exact(column):
    """a result column as exact Python values: Float64 as its bits, a Decimal as its unscaled integer"""
    typ, values = column.type, column.to_pylist()
    if pa.types.is_floating(typ):
        return [None if v is None else _f64_bits(v) for v in values]
    if pa.types.is_decimal(typ):
        return [None if v is None else _unscaled(v, typ.scale) for v in values]
    return values


@pytest.mark.parametrize("shape, n, null_frac, plan", CASES)
def test_every_kind_on_every_accumulation_site(shape, n, null_frac, plan):
    from datafusion_amd.expr import col
    p = PLANS[plan]
    table, key_names, want = _case(shape, n, null_frac)
    site = p.kernel_nulls if null_frac > 0 else p.kernel
    for names in SPLIT.get(plan, (tuple(AGGS),)):
        label = f"{plan} / nulls {null_frac} / {table.num_rows} rows / {' '.join(names)}"
        got, stats = _run_plan(p, table, key_names, [(AGGS[a][0], None if AGGS[a][1] is None else col(AGGS[a][1]), a) for a in names])
        assert site in stats, (label, "the accumulation site did not run", sorted(stats))
        assert got.column_names == key_names + list(names), (label, got.column_names)
        for a in names:      # SUM(Decimal128(p, s)) is Decimal128(min(38, p + 10), s); MIN / MAX and the bitwise results are of the argument's type
            want_type = {"si": pa.int64(), "s15": pa.decimal128(25, 2), "s38": D38, "sf": pa.float64(), "mn": pa.int64(), "mx": pa.float64(), "cx": pa.int64(),
                         "rows": pa.int64(), "a": pa.int64(), "o": pa.int64(), "x": pa.int64()}[a]
            assert got.schema.field(a).type == want_type, (label, a, got.schema.field(a).type)
        keys = list(zip(*[got.column(k).to_pylist() for k in key_names])) if key_names else [()] * got.num_rows
        assert len(keys) == len(set(keys)) and set(keys) == set(want), (label, "group keys differ", len(keys), len(want))
        cols = {a: _exact(got.column(a)) for a in names}
        for r, kt in enumerate(keys):
            row = {a: cols[a][r] for a in names}
            assert row == {a: want[kt][a] for a in names}, f"{label}: group {kt}: {row}, want { {a: want[kt][a] for a in names} }"
