"""tests/agg_distinct_ref.py — the reference of COUNT(DISTINCT x) / SUM(DISTINCT x) — held to hand-worked answers and, on every case
table, to the oracle through the two-level spelling the reference's SingleDistinctToGroupBy rewrite produces: a `Single` aggregate
over (keys, x) without aggregates, then COUNT(x) / SUM(x) by keys (x FILTER (WHERE p) is CASE WHEN p THEN x END).  Then nine wrong
implementations, each of which must differ from the reference on those tables.  (String arguments are not the oracle's: the hand
table and the GPU tests cover them.)"""
import pytest

from tests import agg_distinct_ref as R

ORACLE_COUNT_TYPES = ("i32", "i64", "u8", "u32", "u64", "d32", "dec", "f64")
CASES = R.case_tables()


def _aggs_for(types=ORACLE_COUNT_TYPES):
    aggs = []
    for t in types:
        aggs += [("count_distinct", t, f"cd_{t}", None), ("count_distinct", t, f"cdp_{t}", "p")]
        if t in R.SUM_BITS:
            aggs += [("sum_distinct", t, f"sd_{t}", None), ("sum_distinct", t, f"sdp_{t}", "p")]
    return aggs


def _oracle_two_level(table, keys, agg):
    """one DISTINCT aggregate through GROUP BY (keys, x) with aggr=[], then COUNT(x) / SUM(x) by keys"""
    import pyarrow as pa
    from oracle import oracle
    func, arg, name, flt = agg
    t = R.to_arrow(table, names=list(keys) + [arg] + ([flt] if flt else []))
    x = ("col", arg) if flt is None else ("case", ("col", flt), ("col", arg), None)
    level1 = oracle.aggregate(t, [(("col", k), k) for k in keys] + [(x, "x")], [], "Single")
    level2 = oracle.aggregate(level1, [(("col", k), k) for k in keys], [({"count_distinct": "count", "sum_distinct": "sum"}[func], ("col", "x"), name)], "Single")
    assert level2.schema.field(name).type == (pa.int64() if func == "count_distinct" else
                                              {"dec": pa.decimal128(38, R.DEC[1]), "u32": pa.uint64(), "u64": pa.uint64()}.get(arg, pa.int64()))
    return [R.from_arrow_value(v, R.TYPES[arg]) for v in level2.column(name).to_pylist()]


@pytest.mark.parametrize("case", sorted(CASES))
def test_reference_agrees_with_the_oracle_through_the_two_level_spelling(case):
    table, keys = CASES[case]
    types = [t for t in ORACLE_COUNT_TYPES if t in table]
    aggs = _aggs_for(types)
    got = R.aggregate(table, keys, aggs, R.TYPES)
    if not keys and not table["k"]:
        # (the two-level spelling has no row to group: the one row over no rows is COUNT's 0 and SUM's NULL by definition)
        assert got == [{a[2]: (0 if a[0] == "count_distinct" else None) for a in aggs}]
        return
    for agg in aggs:
        want = _oracle_two_level(table, keys, agg)
        assert [r[agg[2]] for r in got] == want, (case, agg)
    if keys:     # the groups themselves, in first-seen order
        from oracle import oracle
        first = oracle.aggregate(R.to_arrow(table, names=keys), [(("col", k), k) for k in keys], [], "Single").to_pylist()
        assert [{k: r[k] for k in keys} for r in got] == first


def test_known_answers():
    t = R.hand_table()
    aggs = [("count_distinct", "i64", "ci", None), ("sum_distinct", "i64", "si", None), ("count_distinct", "f64", "cf", None), ("count_distinct", "dec", "cdec", None),
            ("sum_distinct", "dec", "sdec", None), ("count_distinct", "u64", "cu", None), ("sum_distinct", "u64", "su", None),
            ("count_distinct", "i64", "cip", "p"), ("sum_distinct", "i64", "sip", "p"), ("sum_distinct", "u64", "sup", "p"), ("count_distinct", "f64", "cfp", "p")]
    assert R.aggregate(t, ["k"], aggs, R.TYPES) == [
        {"k": 1, "ci": 2, "si": 10 + 2**32, "cf": 3, "cdec": 2, "sdec": 6 + 2**64, "cu": 3, "su": 2**63, "cip": 1, "sip": 5, "sup": 2**63 - 1, "cfp": 3},
        {"k": 2, "ci": 2, "si": 12, "cf": 2, "cdec": 2, "sdec": 3 + 2**64 + 10**37, "cu": 1, "su": 2**64 - 1, "cip": 1, "sip": 7, "sup": 2**64 - 1, "cfp": 1},
        {"k": 3, "ci": 0, "si": None, "cf": 1, "cdec": 0, "sdec": None, "cu": 0, "su": None, "cip": 0, "sip": None, "sup": None, "cfp": 0}]
    # without GROUP BY: one row; over no rows: one row of 0 / NULL
    (whole,) = R.aggregate(t, [], aggs[:3], R.TYPES)
    assert whole == {"ci": 3, "si": 17 + 2**32, "cf": 5}
    assert R.aggregate(R.make_table(0), [], aggs[:2], R.TYPES) == [{"ci": 0, "si": None}] and R.aggregate(R.make_table(0), ["k"], aggs[:2], R.TYPES) == []
    # wrapping like SUM's result type: signed 64 bits, unsigned 64 bits, signed 128 bits
    assert R.wrap(2**63, "i64") == -2**63 and R.wrap(2**64 + 5, "u64") == 5 and R.wrap(2**127, "dec") == -2**127 and R.wrap(-1, "u32") == 2**64 - 1
    s = {"k": [1, 1, 1], "i64": [2**63 - 1, 1, 1], "str": ["a", "", "a"]}
    assert R.aggregate(s, ["k"], [("sum_distinct", "i64", "s", None), ("count_distinct", "str", "c", None)], R.TYPES) == [{"k": 1, "s": -2**63, "c": 2}]


def test_the_tables_hold_the_rows_the_tests_need():
    table, keys = CASES["seven_groups"]
    n = len(table["k"])
    assert any(v is None for v in table["i64"]) and 0.05 < sum(v is None for v in table["i64"]) / n < 0.2            # about 10 % NULLs
    assert {True, False, None} == set(table["p"])
    rows = R.aggregate(table, keys, [("count_distinct", "i64", "c", None), ("count_distinct", "i64", "cp", "p"), ("sum_distinct", "i64", "sp", "p")], R.TYPES)
    assert len(rows) == 7 and any(r["c"] > 0 and r["cp"] == 0 and r["sp"] is None for r in rows)                       # a group without a passing row
    pairs = [(table["k"][i], R.bits(table["f64"][i])) for i in range(n)]
    assert any(pairs[i] in pairs[:i - 1] and pairs[i] != pairs[i - 1] for i in range(2, n))                            # duplicates that are not adjacent
    for t in R.EDGES:
        assert {R.bits(v) for v in table[t] if v is not None} == {R.bits(v) for v in R.EDGES[t]}, t                    # every edge value occurs


# ---------------------------------------------------------------------- wrong implementations
MISTAKES = {
    "a_null_counted_as_a_value": "cd_i64",
    "one_global_set_instead_of_one_per_group": "cd_i64",
    "only_adjacent_duplicates_removed": "cd_i64",
    "negative_zero_merged_with_positive_zero": "cd_f64",
    "decimal128_compared_on_its_low_64_bits": "cd_dec",
    "the_set_forgotten_between_two_updates": "cd_i64",
    "a_filter_ignored": "cdp_i64",
    "sum_over_all_rows_instead_of_the_distinct_ones": "sd_i64",
    "a_group_without_a_passing_row_dropped": None,
}


def _wrong(table, keys, aggs, mistake, split=None):
    """R.aggregate with one of the mistakes an implementation of DISTINCT aggregates can make.  `split`: the table arrives as two
    updates, rows [0, split) and [split, n)."""
    n = len(table["k"])
    groups = {}
    for i in range(n):
        if mistake == "a_group_without_a_passing_row_dropped" and table["p"][i] is not True:
            continue
        groups.setdefault(tuple(R.bits(table[k][i]) for k in keys), []).append(i)
    if not keys and not groups:
        groups[()] = []

    def ident(v, arg):
        if mistake == "negative_zero_merged_with_positive_zero" and isinstance(v, float) and v == 0.0:
            return R.bits(0.0)
        if mistake == "decimal128_compared_on_its_low_64_bits" and R.TYPES[arg] == "dec":
            return v & (2**64 - 1)
        return R.bits(v)

    out, global_seen = [], {}
    for rows in groups.values():
        row = {k: table[k][rows[0]] for k in keys}
        for func, arg, name, flt in aggs:
            if mistake == "a_filter_ignored":
                flt = None
            vals = []
            for i in rows:
                v = table[arg][i]
                if flt is not None and table[flt][i] is not True:
                    continue
                if v is None and mistake != "a_null_counted_as_a_value":
                    continue
                vals.append((i, v))
            if mistake == "only_adjacent_duplicates_removed":
                kept = [v for j, (i, v) in enumerate(vals) if j == 0 or ident(v, arg) != ident(vals[j - 1][1], arg)]
            elif mistake == "the_set_forgotten_between_two_updates":
                halves = [[v for i, v in vals if i < split], [v for i, v in vals if i >= split]]
                kept = [v for h in halves for v in {ident(v, arg): v for v in h}.values()]
            elif mistake == "one_global_set_instead_of_one_per_group":
                seen = global_seen.setdefault(name, set())
                kept = []
                for _, v in vals:
                    if ident(v, arg) not in seen:
                        seen.add(ident(v, arg))
                        kept.append(v)
            elif mistake == "sum_over_all_rows_instead_of_the_distinct_ones" and func == "sum_distinct":
                kept = [v for _, v in vals]
            else:
                uniq = {}
                for _, v in vals:
                    uniq.setdefault(ident(v, arg), v)
                kept = list(uniq.values())
            if func == "count_distinct":
                row[name] = len(kept)
            else:
                row[name] = R.wrap(sum(v for v in kept if v is not None), R.TYPES[arg]) if kept else None
        out.append(row)
    return out


@pytest.mark.parametrize("case", ["hand", "seven_groups", "two_keys"])
@pytest.mark.parametrize("mistake", sorted(MISTAKES))
def test_wrong_implementations_differ_from_the_reference(mistake, case):
    table, keys = CASES[case]
    aggs = [a for a in _aggs_for(("i64", "f64", "dec")) if a[1] in table]
    split = len(table["k"]) // 2
    ref = R.aggregate(table, keys, aggs, R.TYPES)
    assert _wrong(table, keys, aggs, None, split) == ref                     # the restatement of the restatement is right
    assert R.aggregate(R.concat([{c: v[:split] for c, v in table.items()}, {c: v[split:] for c, v in table.items()}]), keys, aggs, R.TYPES) == ref
    bad = _wrong(table, keys, aggs, mistake, split)
    shows_in = MISTAKES[mistake]
    if shows_in is None:
        assert len(bad) < len(ref), (mistake, case)                          # whole groups are missing
        return
    assert len(bad) == len(ref) and any(b[shows_in] != r[shows_in] for b, r in zip(bad, ref)), (mistake, case)
