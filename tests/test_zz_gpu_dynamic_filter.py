"""The hash join's dynamic filter against the plain reference of tests/key_stats_ref.py: the IN list of a small build side
(dfgpu_column_inlist), the built table asked for membership (dfgpu_join_contains: every table kind, key set and NullEquality), and
what HashJoinExec publishes to a probe-side ParquetExec — bounds, list, table — for all ten join types, with the row groups and rows
the scan then reads.  A wrong bound or membership bit raises no error: it is a join that silently misses rows."""
import numpy as np
import pyarrow as pa
import pytest

from tests import key_stats_cases as K
from tests import key_stats_ref as R
from tests.util import assert_tables_equal

pytestmark = pytest.mark.gpu

NULL_EQUALITIES = ("NullEqualsNothing", "NullEqualsNull")


def _dev(t):
    from datafusion_amd.table import DeviceTable
    return DeviceTable.from_arrow(t)


# ------------------------------------------------------------------------------------------------------ dfgpu_column_inlist
def _inlist_columns():
    rng = np.random.default_rng(17)
    i64 = [int(v) for v in rng.integers(-50, 50, 400)]
    return {
        "int32_negative": K.column([-2**31, -7, -7, 3, 2**31 - 1, -1, 0], pa.int32()),
        "date32": K.column([9000, -2**31, 12, 9000, 2**31 - 1], pa.date32()),
        "uint8": K.column([255, 0, 7, 255, 128, 127], pa.uint8()),
        "uint32_above_2_31": K.column([2**32 - 1, 2**31, 2**31 - 1, 0, 2**31], pa.uint32()),
        "int64_extremes": K.column([2**63 - 1, -2**63, 0, -1, 2**63 - 1], pa.int64()),
        "duplicates": K.column(i64, pa.int64()),
        "nulls_20_percent": K.column([None if rng.random() < 0.2 else v for v in i64], pa.int64()),
        "all_null": K.column([None] * 9, pa.int32()),
        "empty": K.column([], pa.int64()),
    }


@pytest.mark.parametrize("name", list(_inlist_columns()))
def test_column_inlist_values(name):
    from datafusion_amd import ops
    column = _inlist_columns()[name]
    want = R.in_list(column)
    assert want is not None and (want == [] if name in ("all_null", "empty") else len(want) >= 3)
    assert ops.column_inlist(_dev(pa.table({"k": column})), "k") == want


def test_column_inlist_limits_from_both_sides():
    from datafusion_amd import _lib, ops
    for typ, width in ((pa.int32(), 4), (pa.int64(), 8), (pa.uint8(), 1)):
        rows = 100
        values = [i % 40 for i in range(rows + 1)]
        at, over = K.column(values[:rows], typ), K.column(values, typ)
        assert R.in_list(at, max_size=rows * width) == list(range(40)) and R.in_list(over, max_size=rows * width) is None
        assert ops.column_inlist(_dev(pa.table({"k": at})), "k", max_size=rows * width) == list(range(40))        # rows * width == max_size
        assert ops.column_inlist(_dev(pa.table({"k": over})), "k", max_size=rows * width) is None                 # one more row
    for limit in (150, 7):
        at, over = K.column([i % limit for i in range(400)], pa.int64()), K.column([i % (limit + 1) for i in range(400)], pa.int64())
        assert R.in_list(at, max_distinct=limit) == list(range(limit)) and R.in_list(over, max_distinct=limit) is None
        assert ops.column_inlist(_dev(pa.table({"k": at})), "k", max_distinct_values=limit) == list(range(limit))
        assert ops.column_inlist(_dev(pa.table({"k": over})), "k", max_distinct_values=limit) is None
    small = _dev(pa.table({"k": K.column([1, 2], pa.int64())}))
    assert R.in_list(K.column([1, 2], pa.int64()), max_distinct=0) is None and ops.column_inlist(small, "k", max_distinct_values=0) is None
    assert ops.column_inlist(small, "k", max_distinct_values=2) == [1, 2] and ops.column_inlist(small, "k", max_distinct_values=1) is None
    with pytest.raises(_lib.DfgpuError, match="integer columns only"):
        ops.column_inlist(_dev(pa.table({"k": pa.array([1, 2], pa.uint64())})), "k")


# ------------------------------------------------------------------------------------------------------ dfgpu_join_contains
KINDS = {"auto": 0, "hash_map": 1, "array_map": 2, "rank_map": 3, "flat": 5}
RADIX = 4


def must_answer(kind: int, key_set: str, null_equality: str, build: pa.Table) -> bool:
    """Does the table kind answer membership for the key set?  Every other combination refuses the build when the kind is asked for by name.
      one integer column                              auto, hash map, ArrayMap, rank map, flat
      (Int32, Int64), Decimal128(20, 2), Float64      auto, hash map, flat — ArrayMap and rank map address by ONE integer's value
      Utf8, dictionary-encoded, Boolean               as one integer column: the join interns strings into dictionary indices and widens
                                                      Booleans to bytes on entry, and builds its table over that integer column
    Two refusals inside those rows follow from how the tables are laid out (include/dfgpu.h: modes 2 / 3 / 5 are an error where they do
    not apply), not from the key set:
      * ArrayMap and rank map are sized by max - min of the build keys and have no slot for NULL: they do not apply to a build side
        without a key (no range), nor to NULL build keys that must match (NULL == NULL) — the reference's own gate for its ArrayMap
        (hash_join/exec.rs try_create_array_map);
      * the flat table packs key and NULL flags into 16 bytes: a 16-byte key whose build column carries NULLs has no room for the flag
        NULL == NULL needs (tests/test_gpu_join.py test_flat_table_packed_keys)."""
    if kind in (0, 1):
        return True
    has_null = any(build.column(c).null_count > 0 for c in range(build.num_columns - 1))
    if key_set in K.WIDE_SETS:
        return kind == 5 and not (key_set == "dec20_2" and null_equality == "NullEqualsNull" and has_null)
    if kind in (2, 3):
        return build.num_rows > 0 and not (null_equality == "NullEqualsNull" and has_null)
    return True


TABLE_KIND_OF_MODE = {1: (0,), 2: (1,), 3: (2,), 5: (4, 5)}     # JoinInfo.table_kind of a table asked for by name


@pytest.mark.parametrize("null_equality", NULL_EQUALITIES)
@pytest.mark.parametrize("which", K.BUILD_SIDES)
@pytest.mark.parametrize("key_set", K.KEY_SETS)
def test_join_contains_every_kind_and_key_set(key_set, which, null_equality):
    """JoinHashTable.contains == the reference's membership for every probe size, asked of every table kind that must answer for the
    key set; a kind outside its row of the table refuses (`not applicable` / `do not pack`), the LDS radix table says that it answers
    pairs — exactly these refusals, in both directions"""
    from datafusion_amd import _lib, ops
    bk, pk = K.key_names(key_set)
    seed = K.KEY_SETS.index(key_set) * 10 + K.BUILD_SIDES.index(which) % 3
    probes = [K.probe_side(key_set, n, np.random.default_rng(seed + n)) for n in K.PROBE_SIZES]
    dprobes = [_dev(p) for p in probes]
    builds = {u: K.build_side(key_set, which, u, np.random.default_rng(seed)) for u in (False, True)}
    if which.startswith("many"):
        for u, b in builds.items():
            keys = [r for r in R._rows(b.select(bk))]
            assert (len(set(keys)) < len(keys)) or u
            assert any(v is None for r in keys for v in r) == (which == "many")
    problems = []
    for kname, kind in KINDS.items():
        build = builds[kind == 3]                  # a rank map holds unique keys: it gets every key once, in no order
        try:
            ht = ops.JoinHashTable(_dev(build), bk, null_equality, table_mode=kind)
        except _lib.DfgpuError as err:
            if must_answer(kind, key_set, null_equality, build):
                problems.append(f"{kname}: refused where it must answer: {err}")
            elif not ("not applicable" in str(err) or "do not pack" in str(err)):
                problems.append(f"{kname}: refused in other words: {err}")
            continue
        if not must_answer(kind, key_set, null_equality, build):
            problems.append(f"{kname}: built (table kind {ht.info().table_kind}) where it must refuse")
            continue
        if kind in TABLE_KIND_OF_MODE and ht.info().table_kind not in TABLE_KIND_OF_MODE[kind]:
            problems.append(f"{kname}: built table kind {ht.info().table_kind}")
        for probe, dprobe in zip(probes, dprobes):
            got = ht.contains(dprobe, pk).to_arrow()
            assert got.column_names == ["contains"] and got.schema.field(0).type == pa.bool_() and got.num_rows == probe.num_rows
            assert got.column(0).null_count == 0
            want = R.contains(build.select(bk), probe.select(pk), null_equality)
            if got.column(0).to_pylist() != want:
                bad = [r for r, (g, w) in enumerate(zip(got.column(0).to_pylist(), want)) if g != w]
                problems.append(f"{kname}: {len(bad)} of {probe.num_rows} probe rows differ, first at row {bad[0]}: {probe.slice(bad[0], 1).to_pylist()}")
        ht.free()
    assert not problems, problems
    # the LDS radix table builds over any key set and answers pairs only
    ht = ops.JoinHashTable(_dev(builds[False]), bk, null_equality, table_mode=RADIX)
    with pytest.raises(_lib.DfgpuError, match="answers pairs, not membership"):
        ht.contains(dprobes[-1], pk)
    ht.free()


@pytest.mark.parametrize("kname", list(KINDS))
def test_contains_leaves_the_table_as_it_found_it(kname):
    """membership marks no build row and leaves nothing half-made: after `contains` alone LeftSemi's unmatched pass reports nothing
    and LeftAnti's every build row; a probe after `contains` gives the oracle's rows — also over a rank map of keys in no order,
    whose rank -> row permutation is built by the first probe that needs build rows, which `contains` is not"""
    from datafusion_amd import ops
    from oracle import oracle
    rng = np.random.default_rng(5)
    bk, pk = K.key_names("int64")
    build = K.build_side("int64", "many", kname == "rank_map", rng)
    probe = K.probe_side("int64", 4097, rng)
    dbuild, dprobe = _dev(build), _dev(probe)
    ht = ops.JoinHashTable(dbuild, bk, table_mode=KINDS[kname])
    if kname == "rank_map":
        assert ht.info().table_kind == 2 and not ht.info().build_keys_ascending
    want = R.contains(build.select(bk), probe.select(pk))
    assert ht.contains(dprobe, pk).to_arrow().column(0).to_pylist() == want
    assert ht.emit_unmatched("LeftSemi").num_rows == 0
    assert_tables_equal(ht.emit_unmatched("LeftAnti").to_arrow(), build, ordered=False)
    ht.free()
    ht = ops.JoinHashTable(dbuild, bk, table_mode=KINDS[kname])
    assert ht.contains(dprobe, pk).to_arrow().column(0).to_pylist() == want
    assert_tables_equal(ht.probe(dprobe, pk, "Inner").to_arrow(), oracle.hash_join(build, probe, list(zip(bk, pk)), "Inner"), ordered=False)
    assert ht.contains(dprobe, pk).to_arrow().column(0).to_pylist() == want
    ht.free()


# --------------------------------------------------------------------------------- the dynamic filter through the node
PUBLISHING = ("Inner", "Left", "LeftSemi", "RightSemi", "LeftAnti", "LeftMark")
SILENT = ("Right", "RightAnti", "RightMark", "Full")
COLUMNS = ["l_k", "l_pay", "l_tag"]


@pytest.fixture(scope="module")
def probe_files(tmp_path_factory):
    """{key type: (the probe table, its Parquet file, the same table as the oracle's plan takes it)} — written once"""
    out = {}
    for kname, typ in K.DYNAMIC_KEY_TYPES.items():
        table = K.dynamic_probe(typ)
        path = K.write_dynamic_probe(table, str(tmp_path_factory.mktemp("dynamic") / f"probe_{kname}.parquet"))
        out[kname] = (table, path, _string_columns_encoded(table))
    return out


def _string_columns_encoded(t: pa.Table) -> pa.Table:
    """string columns dictionary-encoded with an ascending dictionary: how the scan delivers them, and what the oracle's plan takes"""
    for i, f in enumerate(t.schema):
        if pa.types.is_string(f.type):
            values = sorted({v for v in t.column(i).to_pylist() if v is not None})
            at = {v: k for k, v in enumerate(values)}
            idx = pa.array([None if v is None else at[v] for v in t.column(i).to_pylist()], pa.int32())
            t = t.set_column(i, f.name, pa.DictionaryArray.from_arrays(idx, pa.array(values, pa.string())))
    return t


def _plain(t: pa.Table) -> pa.Table:
    return pa.table({n: (c.cast(pa.string()) if pa.types.is_dictionary(c.type) else c) for n, c in zip(t.column_names, t.columns)})


def _pay_filter():
    from datafusion_amd.expr import col, lit
    return col("l_pay") > lit(10, pa.int32())


def _join_filter():
    from datafusion_amd.expr import col
    return (col("f0") > col("f1"), [(1, "Left"), (1, "Right")])     # o_pay > l_pay


def _plans(build_dev, build_host, path, probe_host, on, join_type, with_filter, join_filter=None, columns=COLUMNS, **kw):
    """(the plan over the Parquet scan, its scan, the same plan over in-memory tables for the oracle)"""
    from datafusion_amd import physical_plan as P
    scan = P.ParquetExec(path, columns, "probe")
    right = P.FilterExec(_pay_filter(), scan) if with_filter else scan
    mem = P.MemoryExec(probe_host.select(columns), "probe")
    mem_right = P.FilterExec(_pay_filter(), mem) if with_filter else mem
    j = P.HashJoinExec(P.MemoryExec(build_dev, "build"), right, on, join_type, filter=join_filter, **kw)
    o = P.HashJoinExec(P.MemoryExec(build_host, "build"), mem_right, on, join_type, filter=join_filter, **kw)
    return j, scan, o


def _reference_of(build: pa.Table, probe: pa.Table):
    """(bounds, IN list, row groups kept by the statistics step, membership per probe row) of a build side"""
    lo, hi, valid, _, _ = R.minmax(build.column("o_k"))
    bounds = (lo, hi) if valid else (1, 0)
    values = R.in_list(build.column("o_k"))
    kept = R.row_groups_kept(probe, K.ROW_GROUP, "l_k", bounds, values)
    return bounds, values, kept, R.contains(build.select(["o_k"]), probe.select(["l_k"]))


def _check_published(scan, join_type, join_filter, ref, what):
    bounds, values, kept, member = ref
    m = scan.metrics
    assert m["row_groups_total"] == 12, what
    if join_type in SILENT:
        assert scan.dynamic_bounds == {} and scan.dynamic_in_lists == {} and scan.dynamic_membership == {} and m["row_groups_read"] == 12, (what, m)
        return
    assert scan.dynamic_bounds == {"l_k": bounds}, (what, scan.dynamic_bounds)
    assert scan.dynamic_in_lists == ({} if values is None else {"l_k": values}), (what, scan.dynamic_in_lists)
    assert m["row_groups_read"] == len(kept), (what, m, kept)
    if join_type in ("Inner", "RightSemi") and join_filter is None and values is None:
        # the Map strategy: the built table itself, asked per row group; withdrawn (the key stays) once the probe side has run
        assert scan.dynamic_membership == {"l_k": None}, what
        hits = [sum(member[g * K.ROW_GROUP:(g + 1) * K.ROW_GROUP]) for g in kept]
        assert m["rows_passed"] == sum(hits) and m["row_groups_skipped_by_membership"] == sum(1 for h in hits if h == 0), (what, m, hits)
        assert m["rows_scanned"] == len(kept) * K.ROW_GROUP, (what, m)
    else:
        assert scan.dynamic_membership == {}, (what, scan.dynamic_membership)


@pytest.mark.parametrize("which", K.DYNAMIC_BUILDS)
@pytest.mark.parametrize("kname", list(K.DYNAMIC_KEY_TYPES))
def test_dynamic_filter_all_join_types(probe_files, kname, which):
    """HashJoinExec over a probe-side ParquetExec, every join type, plain and with a FilterExec between the join and the scan: the
    oracle's rows over the unpruned probe side; bounds, IN list and membership published exactly where the reference's rules allow it
    and equal to the reference's; as many row groups read (and, for the Map strategy, rows passed) as the reference keeps"""
    from datafusion_amd import ops, physical_plan as P
    from tests import plan_oracle
    typ = K.DYNAMIC_KEY_TYPES[kname]
    probe, path, probe_host = probe_files[kname]
    build = K.dynamic_build(which, typ)
    dbuild = _dev(build)
    ref = _reference_of(build, probe)
    jf = _join_filter() if which == "clustered_join_filter" else None
    assert {"clustered": ref[1] is None and len(ref[2]) == 3, "far_apart": ref[1] == [10, 2500, 3990] and ref[2] == [0, 5, 7, 11],
            "two_clusters": ref[1] is None and len(ref[2]) == 11, "empty": ref[0] == (1, 0) and ref[2] == [], "all_null": ref[0] == (1, 0) and ref[2] == [],
            "below": ref[0] == (-100, -1) and ref[2] == [5], "clustered_join_filter": len(ref[2]) == 3}[which]
    assert list(ops.JOIN_TYPES) and set(ops.JOIN_TYPES) == set(PUBLISHING) | set(SILENT)
    for join_type in ops.JOIN_TYPES:
        for with_filter in (False, True):
            what = (kname, which, join_type, with_filter)
            j, scan, o = _plans(dbuild, build, path, probe_host, [("o_k", "l_k")], join_type, with_filter, jf)
            got = P.collect(j).to_arrow()
            assert_tables_equal(_plain(got), _plain(plan_oracle.collect(o)), ordered=False)
            _check_published(scan, join_type, jf, ref, what)


@pytest.mark.parametrize("join_type", ["Left", "Full"])
@pytest.mark.parametrize("matches", [True, False], ids=["some_match", "none_match"])
def test_unmatched_build_rows_beside_dictionary_encoded_probe_columns(join_type, matches):
    """the NULL-filled probe columns behind the unmatched build rows are made from the columns' types alone: beside a dictionary-encoded
    probe column (every string column of a Parquet scan) they are a plain all-NULL index column, which the concatenation with the
    matched rows has to take into that column's dictionary"""
    from datafusion_amd import physical_plan as P
    from tests import plan_oracle
    build = pa.table({"k": pa.array([1, 2, 3, None, 2], pa.int64()), "b": pa.array([10, 20, 30, 40, 50], pa.int32())})
    tag = pa.DictionaryArray.from_arrays(pa.array([1, 0, None, 1, 0], pa.int32()), pa.array(["x", "y"], pa.string()))
    probe = pa.table({"j": pa.array([2, 2, 5, None, 3] if matches else [7, 8, 9, None, 7], pa.int64()), "tag": tag})
    got = P.collect(P.HashJoinExec(P.MemoryExec(_dev(build), "b"), P.MemoryExec(_dev(probe), "p"), [("k", "j")], join_type)).to_arrow()
    exp = plan_oracle.collect(P.HashJoinExec(P.MemoryExec(build, "b"), P.MemoryExec(probe, "p"), [("k", "j")], join_type))
    assert pa.types.is_dictionary(got.schema.field("tag").type)
    assert_tables_equal(_plain(got), _plain(exp), ordered=False)


def _nothing_published(scan):
    assert scan.dynamic_bounds == {} and scan.dynamic_in_lists == {} and scan.dynamic_membership == {} and scan.metrics["row_groups_read"] == 12, \
        (scan.dynamic_bounds, scan.metrics)


@pytest.mark.parametrize("kname", list(K.DYNAMIC_KEY_TYPES))
def test_nothing_is_published_where_the_reference_forbids_it(probe_files, tmp_path, kname):
    from datafusion_amd import physical_plan as P
    from tests import plan_oracle
    typ = K.DYNAMIC_KEY_TYPES[kname]
    probe, path, probe_host = probe_files[kname]
    build = K.dynamic_build("far_apart", typ)
    dbuild = _dev(build)

    def run(on, join_type, path=path, probe_host=probe_host, build=build, dbuild=dbuild, **kw):
        j, scan, o = _plans(dbuild, build, path, probe_host, on, join_type, False, **kw)
        assert_tables_equal(_plain(P.collect(j).to_arrow()), _plain(plan_oracle.collect(o)), ordered=False)
        return scan
    # published here: the same plan is then run under each of the conditions that forbid it
    assert run([("o_k", "l_k")], "Inner").dynamic_bounds == {"l_k": (10, 3990)}
    _nothing_published(run([("o_k", "l_k")], "Inner", null_equality="NullEqualsNull"))
    _nothing_published(run([("o_k", "l_k")], "LeftAnti", null_aware=True))
    assert run([("o_k", "l_k")], "LeftAnti").dynamic_bounds == {"l_k": (10, 3990)}
    _nothing_published(run([("o_k", "l_k"), ("o_pay", "l_pay")], "Inner"))
    # a Date32 key: the same day numbers
    dates = probe.set_column(0, "l_k", probe.column("l_k").cast(pa.int32()).cast(pa.date32()))
    dpath = K.write_dynamic_probe(dates, str(tmp_path / "dates.parquet"))
    dbuild_t = build.set_column(0, "o_k", build.column("o_k").cast(pa.int32()).cast(pa.date32()))
    _nothing_published(run([("o_k", "l_k")], "Inner", path=dpath, probe_host=_string_columns_encoded(dates), build=dbuild_t, dbuild=_dev(dbuild_t)))
    # a scan that does not read the key column: the join above it cannot run, what it would publish is asked of the node itself
    scan = P.ParquetExec(path, ["l_pay", "l_tag"], "probe")
    j = P.HashJoinExec(P.MemoryExec(dbuild, "build"), scan, [("o_k", "l_k")], "Inner")
    j._publish_dynamic_bounds(dbuild)
    assert j._publish_membership(None) is None
    assert scan.dynamic_bounds == {} and scan.dynamic_in_lists == {} and scan.dynamic_membership == {}
    whole = P.ParquetExec(path, None, "probe")
    j = P.HashJoinExec(P.MemoryExec(dbuild, "build"), whole, [("o_k", "l_k")], "Inner")
    j._publish_dynamic_bounds(dbuild)
    assert whole.dynamic_bounds == {"l_k": (10, 3990)} and whole.dynamic_in_lists == {"l_k": [10, 2500, 3990]}


@pytest.mark.parametrize("join_type", ["Inner", "RightSemi"])
@pytest.mark.parametrize("kname", list(K.DYNAMIC_KEY_TYPES))
def test_a_node_run_again_over_another_build_side_keeps_nothing_stale(probe_files, kname, join_type):
    """the same HashJoinExec and scan collected over a large build side (its table pushed), a small one (its IN list pushed), the large
    one again and the small one again: every run publishes what its own build side gives and nothing of the run before"""
    from datafusion_amd import physical_plan as P
    from tests import plan_oracle
    typ = K.DYNAMIC_KEY_TYPES[kname]
    probe, path, probe_host = probe_files[kname]
    sides = {w: K.dynamic_build(w, typ) for w in ("two_clusters", "far_apart")}
    devs = {w: _dev(b) for w, b in sides.items()}
    refs = {w: _reference_of(b, probe) for w, b in sides.items()}
    j, scan, o = _plans(devs["two_clusters"], sides["two_clusters"], path, probe_host, [("o_k", "l_k")], join_type, False)
    for run, which in enumerate(("two_clusters", "far_apart", "two_clusters", "far_apart")):
        j.left, o.left = P.MemoryExec(devs[which], "build"), P.MemoryExec(sides[which], "build")
        assert_tables_equal(_plain(P.collect(j).to_arrow()), _plain(plan_oracle.collect(o)), ordered=False)
        bounds, values, kept, _ = refs[which]
        assert scan.dynamic_bounds == {"l_k": bounds} and scan.metrics["row_groups_read"] == len(kept), (run, which, scan.metrics)
        if which == "two_clusters":
            assert scan.dynamic_in_lists == {} and scan.dynamic_membership == {"l_k": None}, (run, scan.dynamic_in_lists)
        else:
            assert scan.dynamic_in_lists == {"l_k": values} and scan.dynamic_membership == {}, (run, scan.dynamic_membership)
        _check_published(scan, join_type, None, refs[which], (run, which))
