"""Key statistics on the GPU (dfgpu_column_minmax: k_key_minmax in join.hip, cached on the column) against the plain reference of
tests/key_stats_ref.py, and their readers — the join build, the sort and the ordered-input aggregate, which take the cached answer as
it is — on keys that are ascending but for one pair (tests/key_stats_cases.py): the only inputs on which a subtly wrong statistic
shows, as a join that misses rows, a sort with two rows swapped or an aggregate with a group emitted twice.  Exact integer work."""
import numpy as np
import pyarrow as pa
import pytest

from tests import edge_values as E
from tests import key_stats_cases as K
from tests import key_stats_ref as R
from tests.util import assert_tables_equal

pytestmark = pytest.mark.gpu

FAMILIES = ("clean_runs_nulls", "equal", "descent")


def _dev(t):
    from datafusion_amd.table import DeviceTable
    return DeviceTable.from_arrow(t)


def _family(cid: str) -> str:
    return "equal" if cid.startswith("equal") else "descent" if cid.startswith("descent") else "clean_runs_nulls"


def _want(values) -> tuple:
    """what ops.column_minmax returns: the reference's first four fields, (None, None, 0, False) without a value"""
    lo, hi, valid, asc, _ = R.minmax_values(values)
    return (lo, hi, valid, asc) if valid else (None, None, 0, False)


def _key_table(values, typ) -> pa.Table:
    return pa.table({"k": K.column(values, typ), "row": pa.array(np.arange(len(values), dtype=np.int64))})


# ------------------------------------------------------------------------------------------------------ 1. dfgpu_column_minmax
SHAPE_PARAMS = [(t, n, f) for t, typ in K.TYPES.items() for n in K.sizes_of(typ) for f in FAMILIES if f == "clean_runs_nulls" or n >= 2]


@pytest.mark.parametrize("tname, n, family", SHAPE_PARAMS)
def test_column_minmax_order_shapes(tname, n, family):
    """every order shape at every size, from the type's minimum and up to its maximum (UInt32 also across 2^31, which must come back
    unsigned; UInt8 up to 255): min, max, non-null count and `strictly ascending` as the reference has them — also asked a second time
    (the cached answer) and of a zero-copy selection of the column"""
    from datafusion_amd import ops
    typ = K.TYPES[tname]
    cases = [c for c in K.order_cases(typ, n, rotate=n == K.LARGE) if _family(c[0]) == family]
    assert cases
    for cid, values, (asc, _) in cases:
        want = _want(values)
        assert want[3] == asc, cid
        t = _dev(_key_table(values, typ))
        assert ops.column_minmax(t, "k") == want, (cid, want)
        assert ops.column_minmax(t, "k") == want, (cid, "second call")
        assert ops.column_minmax(t.select(["k"]), "k") == want, (cid, "selection")


@pytest.mark.parametrize("tname, n", [(t, n) for t, typ in K.TYPES.items() for n in K.sizes_of(typ)])
def test_column_minmax_null_layouts(tname, n):
    """5 % random NULLs, all NULL, only the first / only the last row valid, and a descent whose predecessor is NULL (the NULL alone
    must already clear the flag)"""
    from datafusion_amd import ops
    typ = K.TYPES[tname]
    rng = np.random.default_rng(n + len(tname))
    layouts = []
    for lname, lo in K.lows(typ, n).items():
        base = K.clean(lo, n, K.step_of(typ))
        layouts.append((f"random-{lname}", [None if rng.random() < 0.05 else v for v in base]))
        layouts.append((f"first_valid-{lname}", [base[0]] + [None] * (n - 1)))
        layouts.append((f"last_valid-{lname}", [None] * (n - 1) + [base[-1]]))
    layouts.append(("all_null", [None] * n))
    starts = list(K.lows(typ, n).values())
    # (the large size: the positions only it has, and both ends)
    for s, p in enumerate(K.positions(n) if n < K.LARGE else [1, K.GRID * K.BLOCK - 1, K.GRID * K.BLOCK, K.UNROLL * K.GRID * K.BLOCK, n - 1]):
        base = K.clean(starts[s % len(starts)], n, K.step_of(typ))
        layouts.append((f"null_before_descent_at_{p}", K.null_at(K.descent_at(base, p), p - 1)))
    for lid, values in layouts:
        want = _want(values)
        assert want[3] is False or None not in values      # (one row: "only the first row valid" is a NULL-free column)
        if lid == "all_null":
            assert want == (None, None, 0, False)
        t = _dev(_key_table(values, typ))
        assert ops.column_minmax(t, "k") == want, (lid, want)
        assert ops.column_minmax(t, "k") == want, (lid, "second call")


def _view_positions(n):
    return K.positions(n) if n < K.LARGE else [K.GRID * K.BLOCK, n // 2]


@pytest.mark.parametrize("whole_first", [True, False], ids=["whole_first", "whole_last"])
@pytest.mark.parametrize("tname, n", [(t, n) for t, typ in K.TYPES.items() for n in K.sizes_of(typ) if n >= 2])
def test_column_minmax_views_answer_for_their_own_rows(tname, n, whole_first):
    """a column with one descent is not ascending, the rows behind the descent and the rows before it are: a slice answers for its own
    rows whether or not the whole column has cached its answer, a selection shares it, and every output of a hash partition (columns
    that share one buffer) answers for the rows it holds"""
    from datafusion_amd import ops
    from oracle import oracle
    typ = K.TYPES[tname]
    starts = list(K.lows(typ, n).values())
    for s, p in enumerate(_view_positions(n)):
        values = K.descent_at(K.clean(starts[s % len(starts)], n, K.step_of(typ)), p)
        host = _key_table(values, typ)
        t = _dev(host)
        whole = _want(values)
        assert whole[3] is False
        if whole_first:
            assert ops.column_minmax(t, "k") == whole, p
        tail, head = values[p + 1:], values[:p]
        assert ops.column_minmax(t.slice(p + 1, n - p - 1), "k") == _want(tail) and (not tail or _want(tail)[3]), (p, "tail")
        assert ops.column_minmax(t.slice(0, p), "k") == _want(head) and _want(head)[3], (p, "head")
        assert ops.column_minmax(t.slice(p - 1, 2), "k") == _want(values[p - 1:p + 1]), (p, "the pair")
        parts = ops.partition(t, ["k"], 3)
        exp, _ = oracle.hash_partition(host, ["k"], 3)
        for part, e in zip(parts, exp):
            assert_tables_equal(part.to_arrow(), e, ordered=True)
            assert ops.column_minmax(part, "k") == _want(R.values_of(e.column("k"))), (p, "partition")
            assert ops.column_minmax(part, "k") == _want(R.values_of(e.column("k"))), (p, "partition, second call")
        assert ops.column_minmax(t.select(["row", "k"]), "k") == whole, (p, "selection")
        assert ops.column_minmax(t, "k") == whole, (p, "whole")


def test_column_minmax_refuses_other_types():
    from decimal import Decimal

    from datafusion_amd import _lib, ops
    t = _dev(pa.table({"u": pa.array([1, 2], pa.uint64()), "f": pa.array([1.0, 2.0]), "d": pa.array([Decimal("1.00"), Decimal("2.00")], pa.decimal128(20, 2))}))
    for name in ("u", "f", "d"):
        with pytest.raises(_lib.DfgpuError, match="integer columns only"):
            ops.column_minmax(t, name)


# --------------------------------------------------------------------------------- 2. the readers on "ascending but for one pair"
N = 4097
BIG_P = K.GRID * K.BLOCK


def _pair_shapes(n):
    """[(id, p, maker)]: clean and one flaw at every position (the large size: clean and one flaw of each kind at 512 * 256)"""
    ps = K.positions(n) if n < K.LARGE else [BIG_P]
    out = [("clean", None, list)]
    for p in ps:
        out.append((f"equal_at_{p}", p, lambda k, p=p: K.equal_at(k, p)))
        out.append((f"descent_at_{p}", p, lambda k, p=p: K.descent_at(k, p)))
    return out


# every flaw at 4 097 rows over Int64 and Int32 keys; the large size once, over Int64 keys
PAIR_PARAMS = [(n, sid, t) for n, types in ((N, ("int64", "int32")), (K.LARGE, ("int64",))) for sid, _, _ in _pair_shapes(n) for t in types]
START = {"int32": "at_min", "int64": "to_max", "date32": "at_min", "uint32": "cross", "uint8": "at_min"}


def _shape(tname, n, sid):
    typ = K.TYPES[tname]
    (p, make), = [(p, m) for s, p, m in _pair_shapes(n) if s == sid]
    return p, make(K.clean(K.lows(typ, n)[START[tname]], n, K.step_of(typ)))


@pytest.mark.parametrize("measured_first", [True, False], ids=["cached", "unmeasured"])
@pytest.mark.parametrize("n, sid, tname", PAIR_PARAMS)
def test_join_build_reads_the_statistics(n, sid, tname, measured_first):
    """the join build takes `ascending` for "rank == row id" (and so for unique keys) and max - min for the size of its table: the rank
    map (asked for by name and through `auto`), with the statistics cached by dfgpu_column_minmax beforehand, measured by the build,
    and with the cache switched off, reports the order and uniqueness the reference sees and returns the oracle's rows — the payload
    is the build row number, which a rank map that wrongly took rank for row id would get wrong"""
    from datafusion_amd import _lib, ops
    from oracle import oracle
    typ = K.TYPES[tname]
    p, values = _shape(tname, n, sid)
    ref = R.minmax_values(values)
    unique = len(set(values)) == len(values)
    tmin, tmax = K.type_range(typ)
    rng = np.random.default_rng(n % 1000 + len(sid))
    lo, hi = max(tmin, min(values) - 5), min(tmax, max(values) + 5)
    pkeys = [lo + int(rng.random() * (hi - lo)) for _ in range(3000)] + [lo, hi]
    if p is not None:
        pkeys += [values[p - 1], values[p]]
    build = pa.table({"k": K.column(values, typ), "payload": pa.array(np.arange(n, dtype=np.int64))})
    probe = pa.table({"j": K.column(pkeys, typ), "p_row": pa.array(np.arange(len(pkeys), dtype=np.int64))})
    inner, left = oracle.hash_join(build, probe, [("k", "j")], "Inner"), oracle.hash_join(build, probe, [("k", "j")], "Left")
    dprobe = _dev(probe)
    for cached in (None, "0"):
        ops.set_options(join__cached_key_stats=cached)
        for mode in (3, 0):
            dbuild = _dev(build)       # a fresh column: nothing cached but what this round leaves on it
            if measured_first:
                assert ops.column_minmax(dbuild, "k") == (ref[0], ref[1], ref[2], ref[3])
            may_refuse = mode == 3 and sid.startswith("equal_at")     # a rank map holds unique keys only
            try:
                ht = ops.JoinHashTable(dbuild, ["k"], table_mode=mode)
            except _lib.DfgpuError as err:
                assert may_refuse and "not applicable" in str(err), (mode, cached, err)
                continue
            info = ht.info()
            assert bool(info.build_keys_ascending) == ref[3], (mode, cached)
            assert bool(info.build_keys_unique) == unique, (mode, cached)
            assert_tables_equal(ht.probe(dprobe, ["j"], "Inner").to_arrow(), inner, ordered=False)
            ht.free()
            assert_tables_equal(ops.hash_join(dbuild, dprobe, [("k", "j")], "Left", table_mode=mode).to_arrow(), left, ordered=False)


def _profiled(fn):
    from datafusion_amd import ops
    ops.profile_enable(True)
    ops.profile_reset()
    try:
        return fn(), ops.profile_stats()
    finally:
        ops.profile_enable(False)


@pytest.mark.parametrize("measured_first", [True, False], ids=["cached", "unmeasured"])
@pytest.mark.parametrize("desc", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("n, sid, tname", PAIR_PARAMS)
def test_sort_drops_a_key_only_when_it_ascends(n, sid, tname, desc, measured_first):
    """ORDER BY a, k [DESC], v DESC: the carried LSD sort drops `k` and `v` from its key when the statistics call `k` strictly
    ascending.  Rows p-1 and p share `a`; under equal_at they tie on `k` too and only the third key puts them in order (v[p-1] < v[p],
    descending: they swap), under descent_at they are out of order on `k` itself.  Position by position as the oracle sorts."""
    from datafusion_amd import ops
    from oracle import oracle
    typ = K.TYPES[tname]
    p, values = _shape(tname, n, sid)
    rng = np.random.default_rng(n % 1000 + len(sid) + desc)
    a = rng.integers(0, 7, n).astype(np.int32)
    v = rng.integers(0, 1000, n).astype(np.int32)
    if p is not None:
        a[p] = a[p - 1]
        v[p - 1], v[p] = 1, 2
    t = pa.table({"a": pa.array(a), "k": K.column(values, typ), "v": pa.array(v), "row": pa.array(np.arange(n, dtype=np.int64))})
    keys = [("a", False, False), ("k", desc, False), ("v", True, False)]
    ops.set_options(sort__carried_min_rows="0")
    dt = _dev(t)
    if measured_first:
        assert ops.column_minmax(dt, "k")[3] == (sid == "clean")
    got, stats = _profiled(lambda: ops.sort(dt, keys).to_arrow())
    assert_tables_equal(got, oracle.sort(t, keys), ordered=True)
    if sid == "clean":
        assert "sort_lsd_pass_out" in stats, sorted(stats)
    assert_tables_equal(ops.sort(dt, keys, fetch=10).to_arrow(), oracle.sort(t, keys, 10), ordered=True)
    assert_tables_equal(ops.sort(_dev(t), keys, fetch=10).to_arrow(), oracle.sort(t, keys, 10), ordered=True)


def _agg_shapes(tname):
    n = 256 if tname == "uint8" else N
    out = [(n, "clean"), (n, "runs")] + [(n, sid) for sid, _, _ in _pair_shapes(n) if sid != "clean"]
    if tname == "int64":
        out += [(K.LARGE, sid) for sid, _, _ in _pair_shapes(K.LARGE)]
    return out


@pytest.mark.parametrize("measured_first", [True, False], ids=["cached", "unmeasured"])
@pytest.mark.parametrize("tname, n, sid", [(t, n, sid) for t in K.TYPES for n, sid in _agg_shapes(t)])
def test_aggregate_takes_the_runs_node_only_over_ordered_keys(tname, n, sid, measured_first):
    """GROUP BY k over non-decreasing keys (clean, runs, every equal_at) takes the ordered-input node, over a descent it must not — a
    run per group would emit the group of the swapped pair twice.  UInt32 keys cross 2^31 upwards: non-decreasing as unsigned, a descent
    if read as signed; they take the node and are right.  The oracle's groups in every case.  (One UInt8 key alone goes to the 256-slot
    table of 1-byte keys before the ordered-input node is asked: it is grouped with a second key that it determines, which is how a
    UInt8 column becomes that node's ordering key.)"""
    from datafusion_amd import ops
    from datafusion_amd.expr import col
    from oracle import oracle
    typ = K.TYPES[tname]
    if sid == "runs":
        values = K.runs(K.lows(typ, n)[START[tname]], n, K.step_of(typ))
    else:
        _, values = _shape(tname, n, sid)
    ref = R.minmax_values(values)
    if tname == "uint32":
        assert values[0] < 2**31 <= values[-1]
    rng = np.random.default_rng(n % 1000 + len(sid))
    t = pa.table({"k": K.column(values, typ), "x": pa.array(rng.integers(-10**12, 10**12, n))})
    names = ["k"]
    if tname == "uint8":
        t, names = t.append_column("k2", pa.array([v * 3 + 1 for v in values], pa.int32())), ["k", "k2"]
    ops.set_options(jit="1", jit__min_rows="0", jit__strict="1", agg__runs="1")
    dt = _dev(t)
    if measured_first:
        assert ops.column_minmax(dt, "k") == _want(values)
    aggs = [("count", None, "cnt"), ("sum", col("x"), "sx"), ("min", col("x"), "mn"), ("max", col("x"), "mx")]
    got, stats = _profiled(lambda: ops.aggregate(dt, [(col(c), c) for c in names], aggs, "Single").to_arrow())
    assert ("agg_runs_accumulate" in stats) == ref[4], (ref, sorted(stats))
    assert ref[4] == (not sid.startswith("descent"))
    exp = oracle.aggregate(t, [(("col", c), c) for c in names], [("count", None, "cnt"), ("sum", ("col", "x"), "sx"), ("min", ("col", "x"), "mn"), ("max", ("col", "x"), "mx")])
    E.assert_exact(got, exp, ordered=False)      # (by the columns' words: day numbers at the ends of Date32 are no Python dates)
