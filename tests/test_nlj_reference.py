"""tests/nlj_ref.py — the nested-loop join reference of tests/test_gpu_nlj.py — held to hand-worked answers and to the oracle, and the
conditions of that GPU test checked where no GPU is needed: every case has the matched and unmatched rows it is named for, and a
list of wrong joins each differs from the reference on the tables the GPU test uses (so agreeing with it means something)."""
import pyarrow as pa
import pytest

from tests import nlj_cases as NC
from tests import nlj_ref as R

CASES = NC.all_cases()


_passing = NC.passing        # computed once per case and process, shared with tests/test_gpu_nlj.py


# ------------------------------------------------------------------------------------------------------------- hand-worked answers
# left bands [lo, hi): row 0 [0, 10), row 1 [5, 15), row 2 [100, 110) (never hit);  right x: 7, 12, NULL, 50
# x = 7 lies in bands 0 and 1, x = 12 in band 1, NULL and 50 in none.
L = pa.table({"lo": pa.array([0, 5, 100], type=pa.int64()), "hi": pa.array([10, 15, 110], type=pa.int64()), "n": pa.array(["a", "b", "c"])})
Rt = pa.table({"x": pa.array([7, 12, None, 50], type=pa.int64()), "m": pa.array([1.0, 2.0, 3.0, 4.0])})
BAND = (("bin", "and", ("bin", "<=", ("col", "f0"), ("col", "f2")), ("bin", "<", ("col", "f2"), ("col", "f1"))), [(0, "Left"), (1, "Left"), (0, "Right")])
N = None
HAND = {
    "Inner": [(0, 10, "a", 7, 1.0), (5, 15, "b", 7, 1.0), (5, 15, "b", 12, 2.0)],
    "Left": [(0, 10, "a", 7, 1.0), (5, 15, "b", 7, 1.0), (5, 15, "b", 12, 2.0), (100, 110, "c", N, N)],
    "Right": [(0, 10, "a", 7, 1.0), (5, 15, "b", 7, 1.0), (5, 15, "b", 12, 2.0), (N, N, N, N, 3.0), (N, N, N, 50, 4.0)],
    "Full": [(0, 10, "a", 7, 1.0), (5, 15, "b", 7, 1.0), (5, 15, "b", 12, 2.0), (N, N, N, N, 3.0), (N, N, N, 50, 4.0), (100, 110, "c", N, N)],
    "LeftSemi": [(0, 10, "a"), (5, 15, "b")],
    "LeftAnti": [(100, 110, "c")],
    "LeftMark": [(0, 10, "a", True), (5, 15, "b", True), (100, 110, "c", False)],
    "RightSemi": [(7, 1.0), (12, 2.0)],
    "RightAnti": [(N, 3.0), (50, 4.0)],
    "RightMark": [(7, 1.0, True), (12, 2.0, True), (N, 3.0, False), (50, 4.0, False)],
}


@pytest.mark.parametrize("join_type", R.ALL_TYPES)
def test_three_by_four_band_join_by_hand(join_type):
    out = R.nested_loop_join(L, Rt, join_type, BAND)
    rows = [tuple(c[i].as_py() for c in out.columns) for i in range(out.num_rows)]
    assert rows == HAND[join_type]
    if join_type.endswith("Mark"):
        assert out.column_names[-1] == "mark" and out.column("mark").null_count == 0


def test_pair_values_keep_null_apart_from_false_and_projections_pick_columns():
    vals = R.pair_values(L, Rt, BAND)
    assert [(l, r) for l, r, _ in vals] == [(l, r) for r in range(4) for l in range(3)]                # right-row-major
    assert [v for _, r, v in vals if r == 2] == [None, None, None] and [v for _, r, v in vals if r == 3] == [False, False, False]
    out = R.nested_loop_join(L, Rt, "Left", BAND, left_cols=["n", "lo"], right_cols=[])
    assert out.column_names == ["n", "lo"] and out.column("n").to_pylist() == ["a", "b", "b", "c"]
    assert R.nested_loop_join(L, Rt, "Inner", None).num_rows == 12                                      # no filter: the cross join


# --------------------------------------------------------------------------------------------------------------------- the oracle
def _oracle_join(c, join_type):
    """the same join as a hash join on an added constant key column with the same JoinFilter (filter columns keep their indices)"""
    from oracle import oracle
    key = lambda t: t.append_column("__k", pa.array([1] * t.num_rows, type=pa.int32()))
    flt = c.ref_filter if c.ref_filter is not None else (("lit", True, pa.bool_()), [])
    out = oracle.hash_join(key(c.left), key(c.right), [("__k", "__k")], join_type, join_filter=flt)
    return out.select([i for i, n in enumerate(out.column_names) if n != "__k"])


# every filter family and every join type; of the band shapes the ones up to a wave and one at the workgroup's size (the oracle
# materialises all |L| x |R| pairs once per join type, and the larger shapes add nothing the reference could get wrong).  The
# oracle's evaluator has no LIKE.
ORACLE_CASES = [c for c in CASES if c.name != "like_dictionary_65x64" and (c.left.num_rows * c.right.num_rows <= 65 * 257 or c.name == "band_256x256")]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=[c.name for c in ORACLE_CASES])
def test_the_reference_agrees_with_the_oracle(case):
    passing = list(_passing(case.name))
    for jt in R.ALL_TYPES:
        want, got = _oracle_join(case, jt), R.nested_loop_join(case.left, case.right, jt, case.ref_filter, passing=passing)
        if jt in R.PAIR_TYPES:
            assert got.column_names == want.column_names and R.multiset(got) == R.multiset(want), jt
        else:
            assert R.difference(got, want) is None, (jt, R.difference(got, want))


def test_like_reference_on_the_dictionary_case():
    """the one filter leaf the oracle lacks, by hand: LIKE '%green%' over the decoded strings, NULL for NULL"""
    c = NC.by_name("like_dictionary_65x64")
    names = c.left.column("name").combine_chunks().cast(pa.string()).to_pylist()
    got = R._like_values(c.left.column("name"), "%green%")
    assert got == [None if s is None else "green" in s for s in names] and None in got and True in got and False in got
    assert R._like_values(pa.array(["abc", "abd", "xabc", None]), "ab_") == [True, True, False, None]


# ------------------------------------------------------------------------------------------------------- conditions of the GPU test
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_every_case_has_the_rows_it_is_named_for(case):
    nl, nr = case.left.num_rows, case.right.num_rows
    passing = _passing(case.name)
    lh, rh = {l for l, _ in passing}, {r for _, r in passing}
    if case.kind == "empty":
        assert nl == 0 or nr == 0
    elif case.kind == "all_match":
        assert len(passing) == nl * nr > 0
    elif case.kind == "no_match":
        assert not passing and nl and nr
    elif case.kind == "one_sided":
        side = case.filter[1][0][1]
        mixed, n_mixed, full, n_full = (lh, nl, rh, nr) if side == "Left" else (rh, nr, lh, nl)
        assert 0 < len(mixed) < n_mixed and len(full) == n_full
    else:
        assert case.kind == "mixed"
        for hit, n in ((lh, nl), (rh, nr)):
            assert len(hit) >= 1
            assert n == 1 or len(hit) < n, "a side of two rows or more has an unmatched row"
    assert nl * nr <= 700 * 520


def test_the_chunked_cases_have_the_chunks_they_are_named_for():
    for name, chunks, last in (("band_700x1_three_chunks", 3, 100), ("band_515x63_ragged_chunks", 3, 115), ("band_700x3_seven_chunks", 7, 100)):
        c = NC.by_name(name)
        rows, nl = c.options["nlj__left_chunk_rows"], c.left.num_rows
        assert -(-nl // rows) == chunks >= 3 and nl - (chunks - 1) * rows == last and last % NC.TL != 0
    # the materialising path in pieces: a piece ends between two passing pairs of one right row
    c = NC.by_name("band_wide_materialised_pieces_65x63")
    piece, nl = c.options["nlj__chunk_pairs"], c.left.num_rows
    passing = _passing(c.name)
    assert nl * c.right.num_rows > 3 * piece
    assert any(r0 == r1 and (r0 * nl + l0) // piece != (r1 * nl + l1) // piece for (l0, r0), (l1, r1) in zip(passing, passing[1:]))


# ---------------------------------------------------------------------------------------------------------------- wrong joins
def _null_is_a_match(c, jt):
    passing = [(l, r) for l, r, v in NC.pair_values(c.name) if v is not False]
    return R.nested_loop_join(c.left, c.right, jt, passing=passing)


def _anti_is_some_pair_fails(c, jt):
    vals = NC.pair_values(c.name)
    side = 0 if jt == "LeftAnti" else 1
    rows = sorted({p[side] for p in vals if p[2] is not True})
    return R.materialise(c.left, c.right, rows if side == 0 else None, rows if side == 1 else None, None, jt)


def _visited_by_rejected_pairs(c, jt):
    nl, nr = c.left.num_rows, c.right.num_rows
    li, ri, marks = R.index_rows(nl, nr, list(_passing(c.name)), jt)
    if jt in ("Left", "Full"):            # every left row met some pair: none is reported unmatched
        keep = [k for k in range(len(li)) if ri[k] is not None]
        li, ri = [li[k] for k in keep], [ri[k] for k in keep]
    elif jt == "LeftSemi":
        li = list(range(nl))
    elif jt == "LeftAnti":
        li = []
    else:
        marks = [True] * nl
    return R.materialise(c.left, c.right, li, ri, marks, jt)


def _mark_is_null_for_unmatched(c, jt):
    li, ri, marks = R.index_rows(c.left.num_rows, c.right.num_rows, list(_passing(c.name)), jt)
    return R.materialise(c.left, c.right, li, ri, [True if m else None for m in marks], jt)


def _unmatched_once_per_chunk(c, jt):
    li, ri, _ = R.index_rows(c.left.num_rows, c.right.num_rows, list(_passing(c.name)), jt)
    extra = [k for k in range(len(li)) if ri[k] is None]           # the unmatched left rows, reported by a second chunk again
    return R.materialise(c.left, c.right, li + [li[k] for k in extra], ri + [None] * len(extra), None, jt)


def _left_major_pairs(c, jt):
    return R.nested_loop_join(c.left, c.right, jt, passing=sorted(_passing(c.name)))


WRONG = [("a NULL filter value taken as a match", _null_is_a_match, R.ALL_TYPES, ["nulls_65x257", "nulls_257x65"]),
         ("Anti as 'some pair fails'", _anti_is_some_pair_fails, ("LeftAnti", "RightAnti"), ["band_257x255", "nulls_65x257", "band_515x63_ragged_chunks"]),
         ("left visited marks set by rejected pairs", _visited_by_rejected_pairs, ("Left", "Full", "LeftSemi", "LeftAnti", "LeftMark"),
          ["band_257x255", "nulls_65x257", "band_700x3_seven_chunks"]),
         ("a Mark column that is NULL for unmatched rows", _mark_is_null_for_unmatched, ("LeftMark", "RightMark"), ["band_257x255", "nulls_257x65"]),
         ("unmatched rows of Full once per chunk", _unmatched_once_per_chunk, ("Left", "Full"), ["band_515x63_ragged_chunks", "band_700x3_seven_chunks"]),
         ("left-major pair order", _left_major_pairs, R.PAIR_TYPES, ["band_257x255", "band_wide_65x63", "nulls_65x257"])]


@pytest.mark.parametrize("what,wrong,types,names", WRONG, ids=[w[0] for w in WRONG])
def test_wrong_joins_differ_from_the_reference_on_the_gpu_tests_tables(what, wrong, types, names):
    for name in names:
        c = NC.by_name(name)
        for jt in types:
            want = R.nested_loop_join(c.left, c.right, jt, passing=list(_passing(name)))
            assert R.difference(wrong(c, jt), want) is not None, (what, name, jt)
