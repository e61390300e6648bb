"""tests/bitwise_ref.py against functools.reduce over Python ints, and the proof that its input families tell a wrong evaluator from a
right one: every mistake an accumulation site can make with an AND / OR / XOR cell changes at least one group of the family built
for it.  The last test pins the function ids of ops.AGG_FUNCS to the header's enum."""
import functools
import operator
import os
import re

import numpy as np
import pyarrow as pa
import pytest

from tests import bitwise_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = dict(B.INT_TYPES, bool=pa.bool_())
OPS = {"bit_and": operator.and_, "bit_or": operator.or_, "bit_xor": operator.xor, "bool_and": lambda a, b: a and b, "bool_or": lambda a, b: a or b}
CASES = [(f, t) for f in B.BIT_FUNCS for t in B.INT_TYPES] + [(f, "bool") for f in B.BOOL_FUNCS]


def _gids(shape, n=6000):
    """random: 48 groups in no order, one of a single row, and a last one (which `family` leaves without a value when it makes NULLs);
    runs: ordered runs whose lengths walk over the word edges, among them runs of one row"""
    rng = np.random.default_rng(3)
    if shape == "random":
        g = rng.integers(0, 48, n)
        g[n // 2] = 48
        g[[5, 700, n - 2000 if n > 2000 else n - 9]] = 49
        return g
    lengths, total = [], 0
    while total < n:
        lengths.append((1, 63, 64, 65, 130, 7, 2)[len(lengths) % 7])
        total += lengths[-1]
    return np.repeat(np.arange(len(lengths)), lengths)[:n]


def _all_ones(typ):
    return True if pa.types.is_boolean(typ) else -1 if pa.types.is_signed_integer(typ) else 2**typ.bit_width - 1


def _python(func, gids, values, valid, start=None, null_as=None, drop=None):
    """the same reduction over Python ints, with the mistakes the tests below switch on"""
    groups = {int(g): [] for g in np.unique(gids)}
    for i, (g, v) in enumerate(zip(np.asarray(gids).tolist(), np.asarray(values).tolist())):
        if i == drop:
            continue
        if valid is None or valid[i]:
            groups[g].append(v)
        elif null_as is not None:
            groups[g].append(null_as)
    out = {}
    for g, vals in groups.items():
        if start is not None:
            out[g] = functools.reduce(OPS[func], vals, start) if vals else None
        else:
            out[g] = functools.reduce(OPS[func], vals) if vals else None
    return out


def _differs(a, b):
    assert a.keys() == b.keys()
    return [g for g in a if a[g] != b[g] or type(a[g]) is not type(b[g])]


@pytest.mark.parametrize("shape", ["random", "runs"])
@pytest.mark.parametrize("null_frac", B.NULL_FRACTIONS)
@pytest.mark.parametrize("func, tname", CASES)
def test_reference_agrees_with_reduce_over_python_ints(func, tname, null_frac, shape):
    typ, gids = TYPES[tname], _gids(shape)
    values, valid, witnesses = B.family(func, typ, gids, null_frac)
    got = B.reduce_groups(func, gids, values, valid, typ)
    want = _python(func, gids, values, valid)
    assert not _differs(got, want)
    if null_frac > 0:
        assert got[B.all_null_group(gids)] is None and sum(v is None for v in got.values()) >= 1
    else:
        assert all(v is not None for v in got.values())
    if func != "bit_xor":
        # the witnesses sit where the family says: the table's word edges and last row, every group's first and last row
        n = len(gids)
        dead = B.all_null_group(gids) if null_frac > 0 else None
        if tname != "bool":
            for r in B.WORD_EDGE_ROWS + (n - 1,):
                assert r in witnesses or gids[r] == dead, r
            for g, rows in B.witness_rows(gids).items():
                assert g == dead or (rows[0] in witnesses and rows[-1] in witnesses), g
        assert len(set(got.values()) - {None}) >= 2        # no family is a constant


def test_edge_values_reduce_at_the_types_width():
    for tname, typ in B.INT_TYPES.items():
        e = B.edge_values(typ)
        w = typ.bit_width
        assert len(set(e)) == 4 and all(pa.array([v], typ)[0].as_py() == v for v in e), tname
        vals = np.array(e, B.np_dtype(typ))
        one = np.zeros(4, np.int64)
        assert B.reduce_groups("bit_and", one, vals, None, typ) == {0: 0}
        assert B.reduce_groups("bit_or", one, vals, None, typ) == {0: e[1]}            # all ones: -1 signed, 2^w - 1 unsigned
        assert B.reduce_groups("bit_xor", one[:2], vals[1:3], None, typ) == {0: e[3]}      # all ones ^ the sign bit = the largest positive
        assert e[2] == (-2**(w - 1) if pa.types.is_signed_integer(typ) else 2**(w - 1))
    assert B.edge_values(pa.uint64())[1:3] == [2**64 - 1, 2**63] and B.edge_values(pa.uint32())[1:3] == [2**32 - 1, 2**31] and B.edge_values(pa.uint8())[1] == 255
    assert B.edge_values(pa.int32())[2] == -2**31 and B.edge_values(pa.int64())[2] == -2**63


def test_states_merge_to_the_whole():
    gids = _gids("random")
    for func, tname in CASES:
        typ = TYPES[tname]
        values, valid, _ = B.family(func, typ, gids, 0.1)
        whole = B.reduce_groups(func, gids, values, valid, typ)
        cuts = [0, 700, 701, 2500, len(gids)]
        parts = [B.reduce_groups(func, gids[a:b], values[a:b], valid[a:b], typ) for a, b in zip(cuts, cuts[1:])]
        merged = {}
        for p in parts:
            for g, s in p.items():
                merged[g] = B.merge(func, merged.get(g), s)
        assert not _differs(merged, whole), (func, tname)
    assert B.merge("bit_xor", None, None) is None and B.merge("bit_and", None, 5) == 5 and B.merge("bool_or", False, None) is False


# ---------------------------------------------------------------------- wrong evaluators
@pytest.mark.parametrize("tname", list(TYPES))
@pytest.mark.parametrize("null_frac", B.NULL_FRACTIONS)
def test_an_and_that_starts_from_zero_and_an_or_that_starts_from_all_ones_show(tname, null_frac):
    typ, gids = TYPES[tname], _gids("random")
    for func, start in ((("bool_and", False), ("bool_or", True)) if tname == "bool" else (("bit_and", 0), ("bit_or", _all_ones(typ)))):
        values, valid, _ = B.family(func, typ, gids, null_frac)
        ref = B.reduce_groups(func, gids, values, valid, typ)
        assert _differs(_python(func, gids, values, valid, start=start), ref), func


@pytest.mark.parametrize("func, tname", [c for c in CASES if c[0] in ("bit_and", "bool_and")])
def test_a_null_read_as_zero_shows(func, tname):
    typ, gids = TYPES[tname], _gids("random")
    values, valid, _ = B.family(func, typ, gids, 0.1)
    ref = B.reduce_groups(func, gids, values, valid, typ)
    zero = False if tname == "bool" else 0
    bad = _python(func, gids, values, valid, null_as=zero)
    assert _differs(bad, ref) and bad[B.all_null_group(gids)] == zero
    # and the value that lies UNDER a NULL is poison too: reading the column without its validity changes a group
    assert _differs(_python(func, gids, values, None), ref)


@pytest.mark.parametrize("shape", ["random", "runs"])
@pytest.mark.parametrize("func, tname", [c for c in CASES if c[0] != "bit_xor"])
def test_every_dropped_witness_row_shows(func, tname, shape):
    typ, gids = TYPES[tname], _gids(shape, 1500)
    values, valid, witnesses = B.family(func, typ, gids, 0.1)
    ref = B.reduce_groups(func, gids, values, valid, typ)
    assert witnesses
    for r, g in witnesses.items():
        keep = np.ones(len(gids), bool)
        keep[r] = False
        bad = B.reduce_groups(func, gids[keep], values[keep], valid[keep], typ)
        bad.setdefault(g, None)           # (a group of one row disappears with it)
        assert bad[g] != ref[g], (r, g)


@pytest.mark.parametrize("tname", list(B.INT_TYPES))
def test_a_lost_or_doubled_row_and_a_state_merged_twice_show_under_xor(tname):
    typ, gids = B.INT_TYPES[tname], _gids("random", 1500)
    values, valid, _ = B.family("bit_xor", typ, gids, 0.1)
    ref = B.reduce_groups("bit_xor", gids, values, valid, typ)
    for r in np.flatnonzero(valid & (values != 0))[:200]:
        assert _python("bit_xor", gids, values, valid, drop=int(r))[int(gids[r])] != ref[int(gids[r])], r
    half = len(gids) // 2
    s1 = B.reduce_groups("bit_xor", gids[:half], values[:half], valid[:half], typ)
    s2 = B.reduce_groups("bit_xor", gids[half:], values[half:], valid[half:], typ)
    twice = {g: B.merge("bit_xor", B.merge("bit_xor", s1.get(g), s2.get(g)), s2.get(g)) for g in ref}
    assert len(_differs(twice, ref)) >= len(ref) // 2


@pytest.mark.parametrize("func", B.BIT_FUNCS)
def test_a_uint32_result_with_bits_above_31_and_an_int32_result_without_its_sign_show(func):
    gids = _gids("random")
    values, valid, _ = B.family(func, pa.uint32(), gids, 0.1)
    ref = B.reduce_groups(func, gids, values, valid, pa.uint32())
    sign_extended = values.view(np.int32).astype(np.int64)         # the cell of an accumulator that sign-extended the UInt32 value ...
    cell = _python(func, gids, sign_extended, valid)
    as_u64 = {g: None if v is None else v & (2**64 - 1) for g, v in cell.items()}
    assert _differs(as_u64, ref)                                   # ... written out whole carries bits above 31
    assert not _differs({g: None if v is None else v & (2**32 - 1) for g, v in cell.items()}, ref)    # its low 32 bits are the result
    values, valid, _ = B.family(func, pa.int32(), gids, 0.1)
    ref = B.reduce_groups(func, gids, values, valid, pa.int32())
    assert any(v is not None and v < 0 for v in ref.values())
    zero_extended = {g: None if v is None else v & (2**32 - 1) for g, v in ref.items()}
    assert _differs(zero_extended, ref)


@pytest.mark.parametrize("func, tname", CASES)
def test_a_count_where_the_value_belongs_shows(func, tname):
    typ, gids = TYPES[tname], _gids("random")
    values, valid, _ = B.family(func, typ, gids, 0.1)
    ref = B.reduce_groups(func, gids, values, valid, typ)
    counts = {int(g): int(valid[gids == g].sum()) or None for g in np.unique(gids)}
    if tname == "bool":
        counts = {g: None if c is None else bool(c & 1) for g, c in counts.items()}       # what the emit keeps of a cell: its low bit
    assert _differs(counts, ref)


# ---------------------------------------------------------------------- the function ids
def test_the_function_ids_are_the_headers():
    from datafusion_amd import ops
    header = open(os.path.join(ROOT, "include", "dfgpu.h")).read()
    enum = re.search(r"typedef enum dfgpu_agg_func \{(.*?)\} dfgpu_agg_func;", header, re.S).group(1)
    ids = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"DFGPU_AGG_(\w+) = (\d+)", enum)}
    for name in B.FUNCS:
        assert ops.AGG_FUNCS[name] == ids[name], name
    assert [ids[f] for f in B.FUNCS] == [9, 10, 11, 12, 13]
    assert ops.VARIANCE_FUNCS == {"var", "var_samp", "var_sample", "var_pop", "var_population", "stddev", "stddev_samp", "stddev_pop"}
    assert int(re.search(r"#define DFGPU_ABI_VERSION (\d+)", header).group(1)) >= 15
