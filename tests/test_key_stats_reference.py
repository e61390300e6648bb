"""The reference of the key-statistics tests (tests/key_stats_ref.py) and their cases (tests/key_stats_cases.py), checked without a GPU:
the reference tells the order shapes apart — which is why a kernel that did not would fail tests/test_zz_gpu_key_stats.py — and agrees
with independent statements of the same things: a brute force over all pairs of neighbours, the oracle's RightSemi join, and the
statistics pyarrow writes into a Parquet footer."""
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from tests import key_stats_cases as K
from tests import key_stats_ref as R

TYPE_IDS = list(K.TYPES)


def test_every_parametrised_list_has_cases():
    assert K.SIZES[-1] == 512 * 256 * 4 + 1025 == 525_313
    for name, typ in K.TYPES.items():
        sizes = K.sizes_of(typ)
        assert sizes and (name == "uint8" or sizes == K.SIZES), name
        for n in sizes:
            cases = K.order_cases(typ, n, rotate=n == K.LARGE)
            assert cases and len({c[0] for c in cases}) == len(cases)
            tmin, tmax = K.type_range(typ)
            clean = {c[0]: c[1] for c in cases if c[0].startswith("clean")}
            assert clean["clean-at_min"][0] == tmin and clean["clean-to_max"][-1] == tmax, (name, n)
            for _, values, _ in cases:
                assert len(values) == n and (n == K.LARGE or all(v is None or tmin <= v <= tmax for v in values))
    assert K.positions(K.LARGE) == [1, 63, 64, 255, 256, 257, K.LARGE // 2, K.LARGE - 1, 512 * 256 - 1, 512 * 256, 4 * 512 * 256]
    assert K.positions(1) == [] and K.positions(2) == [1] and K.positions(65) == [1, 63, 64, 32]
    assert K.KEY_SETS and K.PROBE_SIZES and K.BUILD_SIDES and K.DYNAMIC_BUILDS and K.DYNAMIC_KEY_TYPES


@pytest.mark.parametrize("tname", TYPE_IDS)
def test_reference_tells_the_order_shapes_apart(tname):
    """clean (True, True); runs and every equal_at (False, True); every descent_at and null_at (False, False) — at every size, the
    large one included; min / max / valid are those of the base key"""
    typ = K.TYPES[tname]
    for n in K.sizes_of(typ):
        seen = set()
        for cid, values, want in K.order_cases(typ, n, rotate=n == K.LARGE):
            # (the large size: over the values themselves, which is what to_pylist() of their column gives — checked at the other sizes)
            lo, hi, valid, asc, nondec = R.minmax_values(values) if n == K.LARGE else R.minmax(K.column(values, typ))
            assert (asc, nondec) == want, (tname, n, cid)
            present = [v for v in values if v is not None]
            assert valid == len(present) and (lo, hi) == ((min(present), max(present)) if present else (None, None)), (tname, n, cid)
            seen.add(cid.split("-")[0].rstrip("0123456789").rstrip("_"))
        assert seen == ({"clean", "null_at"} if n == 1 else {"clean", "runs", "equal_at", "descent_at", "null_at"}), (tname, n, seen)


def _brute(values):
    """no running state: every statistic straight from its definition"""
    present = [v for v in values if v is not None]
    whole = len(values) > 0 and len(present) == len(values)
    asc = whole and all(values[i - 1] < values[i] for i in range(1, len(values)))
    nondec = whole and all(values[i - 1] <= values[i] for i in range(1, len(values)))
    return (min(present) if present else None, max(present) if present else None, len(present), asc, nondec)


@pytest.mark.parametrize("tname", TYPE_IDS)
def test_minmax_agrees_with_brute_force_on_small_cases(tname):
    typ = K.TYPES[tname]
    rng = np.random.default_rng(len(tname))
    for n in [n for n in K.sizes_of(typ) if n <= 65]:
        for cid, values, _ in K.order_cases(typ, n):
            assert R.minmax(K.column(values, typ)) == _brute(values), (tname, n, cid)
        base = K.clean(K.lows(typ, n)["at_min"], n, K.step_of(typ))
        for values in ([None] * n, [base[0]] + [None] * (n - 1), [None] * (n - 1) + [base[-1]], [v if rng.random() > 0.05 else None for v in base],
                       [int(v) for v in rng.permutation(base)]):
            assert R.minmax(K.column(values, typ)) == _brute(values), (tname, n)
    assert R.minmax(K.column([], typ)) == (None, None, 0, False, False)


def test_in_list_limits():
    c = pa.array([5, -3, None, 5, 7, -3], pa.int32())
    assert R.in_list(c) == [-3, 5, 7] and R.in_list(c, max_distinct=3) == [-3, 5, 7] and R.in_list(c, max_distinct=2) is None
    assert R.in_list(c, max_size=24) == [-3, 5, 7] and R.in_list(c, max_size=23) is None and R.in_list(c, max_distinct=0) is None
    assert R.in_list(pa.array([None, None], pa.int64())) == [] and R.in_list(pa.array([], pa.int64()), max_distinct=0) == []
    assert R.in_list(pa.array([2**32 - 1, 2**31, 0], pa.uint32())) == [0, 2**31, 2**32 - 1]
    assert R.in_list(K.column([3, None, -2**31], pa.date32())) == [-2**31, 3]


def _oracle_form(build: pa.Table, probe: pa.Table, bk, pk):
    """the oracle has neither strings nor Booleans: such key columns go to it as the index of the value in the sorted values of both sides"""
    def surrogate(t, names, others):
        for a, b in zip(names, others[1]):
            typ = t.schema.field(a).type
            if pa.types.is_string(typ) or pa.types.is_dictionary(typ) or pa.types.is_boolean(typ):
                mine, theirs = R.values_of(t.column(a)), R.values_of(others[0].column(b))
                order = sorted({v for v in mine + theirs if v is not None})
                t = t.set_column(t.schema.get_field_index(a), a, pa.array([None if v is None else order.index(v) for v in mine], pa.int32()))
        return t
    return surrogate(build, bk, (probe, pk)), surrogate(probe, pk, (build, bk))


@pytest.mark.parametrize("key_set", K.KEY_SETS)
def test_contains_agrees_with_the_oracles_right_semi_join(key_set):
    from oracle import oracle
    bk, pk = K.key_names(key_set)
    for which in K.BUILD_SIDES:
        for unique in (False, True):
            rng = np.random.default_rng(len(key_set) * 7 + len(which) + unique)
            build = K.build_side(key_set, which, unique, rng)
            for n in (0, 1, 65, 1025):
                probe = K.probe_side(key_set, n, rng)
                ob, op = _oracle_form(build, probe, bk, pk)
                for ne in ("NullEqualsNothing", "NullEqualsNull"):
                    got = R.contains(build.select(bk), probe.select(pk), ne)
                    semi = set(oracle.hash_join(ob, op, list(zip(bk, pk)), "RightSemi", ne).column("p_row").to_pylist())
                    assert got == [r in semi for r in range(n)], (key_set, which, unique, n, ne)
                    if which == "many" and n == 1025 and key_set != "bool":
                        assert 300 < sum(got) < 700      # about half of the probe keys are present


def test_contains_float_keys_compare_by_their_bits():
    from tests.edge_values import from_raw
    build = pa.table({"k": from_raw(K.F64_SPECIAL[0:1] + K.F64_SPECIAL[2:3], pa.float64())})            # +0.0, NaN
    probe = pa.table({"j": from_raw(K.F64_SPECIAL + [0], pa.float64(), [False] * 4 + [True])})
    assert R.contains(build, probe) == [True, False, True, False, False]


def _kept_by_footer(path, bounds, values):
    """row groups kept, from the min / max pyarrow wrote into the file (exact for Int32 / Int64)"""
    meta = pq.ParquetFile(path).metadata
    keep = []
    for g in range(meta.num_row_groups):
        st = meta.row_group(g).column(0).statistics
        if (bounds is not None and bounds[0] > bounds[1]) or (values is not None and not values):
            continue
        if st is not None and st.has_min_max:
            if bounds is not None and (st.max < bounds[0] or st.min > bounds[1]):
                continue
            if values is not None and not [v for v in values if st.min <= v <= st.max]:
                continue
        keep.append(g)
    return keep


@pytest.mark.parametrize("kname", list(K.DYNAMIC_KEY_TYPES))
def test_row_groups_kept_agrees_with_the_parquet_footer(tmp_path, kname):
    typ = K.DYNAMIC_KEY_TYPES[kname]
    probe = K.dynamic_probe(typ)
    path = K.write_dynamic_probe(probe, str(tmp_path / "probe.parquet"))
    meta = pq.ParquetFile(path).metadata
    assert meta.num_row_groups == 12 and not meta.row_group(K.NULL_GROUP).column(0).statistics.has_min_max
    assert R.row_groups_kept(probe, K.ROW_GROUP, "l_k") == list(range(12))
    kept = {}
    for which in K.DYNAMIC_BUILDS:
        build = K.dynamic_build(which, typ)
        lo, hi, valid, _, _ = R.minmax(build.column("o_k"))
        bounds = (lo, hi) if valid else (1, 0)
        values = R.in_list(build.column("o_k"))
        for b, v in ((bounds, values), (bounds, None), (None, values)):
            assert R.row_groups_kept(probe, K.ROW_GROUP, "l_k", b, v) == _kept_by_footer(path, b, v), (which, b is None, v is None)
        kept[which] = R.row_groups_kept(probe, K.ROW_GROUP, "l_k", bounds, values)
    # the build sides prune what they were made to prune
    assert kept["clustered"] == [5, 6, 7] and kept["empty"] == kept["all_null"] == [] and kept["below"] == [5]
    assert kept["far_apart"] == [0, 5, 7, 11] and R.row_groups_kept(probe, K.ROW_GROUP, "l_k", (10, 3990), None) == list(range(12))
    assert R.in_list(K.dynamic_build("two_clusters", typ).column("o_k")) is None and kept["two_clusters"] == list(range(0, 11))
