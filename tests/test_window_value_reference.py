"""tests/window_value_ref.py (percent_rank, cume_dist, ntile, first_value / last_value / nth_value) held to hand-worked answers, to
tests/window_ref.py where the two overlap, and to a list of plausible wrong implementations, each of which must change a result on the
reference table of tests/window_cases.py — so a device operator that agrees with the restatement there has made none of them."""
import pytest

from tests import window_cases as WC
from tests import window_ref as W
from tests import window_value_ref as V

PART, ORDER = ["p1", "p2"], ["o"]


@pytest.fixture(scope="module")
def table():
    cols, types = WC.reference_table()
    frames = WC.frames(cols, WC.PARTITION_LENGTHS, ORDER)       # (s, i, pe, e) per row, from the lengths the table was built with
    return cols, types, frames


def _peer_starts(frames):
    out = []
    for i, (s, _, pe, _) in enumerate(frames):
        out.append(s if i == s else (out[-1] if frames[i - 1][2] == pe else i))
    return out


def test_positions_are_the_frames_the_table_was_built_with(table):
    cols, _, frames = table
    n = len(cols["o"])
    assert n == sum(WC.PARTITION_LENGTHS)
    ps = _peer_starts(frames)
    assert V.positions(cols, PART, ORDER, n) == [(s, e, ps[i], pe) for i, (s, _, pe, e) in enumerate(frames)]
    assert V.positions(cols, [], [], n) == [(0, n - 1, 0, n - 1)] * n
    assert V.positions(cols, PART, [], n) == [(s, e, s, e) for s, _, _, e in frames]
    assert V.positions({}, [], [], 0) == []


def test_ntile_by_hand():
    six = {"p": [1] * 6, "x": list(range(6))}
    assert V.window(six, ["p"], [], [(("ntile", 4), None, "q", None)])["q"] == [1, 1, 2, 3, 3, 4]          # not 1,1,2,2,3,4
    ten = {"p": [1] * 10, "x": list(range(10))}
    assert V.window(ten, ["p"], [], [(("ntile", 4), None, "q", None)])["q"] == [1, 1, 1, 2, 2, 3, 3, 3, 4, 4]
    assert V.window(ten, ["p"], [], [(("ntile", 1), None, "q", None)])["q"] == [1] * 10
    assert V.window(ten, ["p"], [], [(("ntile", 10), None, "q", None)])["q"] == list(range(1, 11))
    assert V.window(ten, ["p"], [], [(("ntile", 2**40), None, "q", None)])["q"] == list(range(1, 11))    # k = min(n, rows)
    two = {"p": [1] * 6 + [2] * 10}
    assert V.window(two, ["p"], [], [(("ntile", 4), None, "q", None)])["q"] == [1, 1, 2, 3, 3, 4, 1, 1, 1, 2, 2, 3, 3, 3, 4, 4]


def test_hand_worked_answers_on_the_reference_table(table):
    cols, _, frames = table
    got = V.window(cols, PART, ORDER, [("percent_rank", None, "pr", None), ("cume_dist", None, "cd", None), (("ntile", 4), None, "q4", None),
                                       (("ntile", 2), None, "q2", None), ("first_value", "i64", "fv", None), ("last_value", "i64", "lv", "partition"),
                                       (("nth_value", 2), "i64", "n2", "rows_to_current"), (("nth_value", -1), "i64", "m1", "partition"),
                                       (("nth_value", 6), "i64", "n6", "partition"), (("nth_value", -2), "i64", "m2", "rows_to_current")])
    # partition 0: rows 0..4, the order key None, None, then values: rows 0 and 1 are one peer group
    assert cols["o"][:2] == [None, None] and cols["o"][2] == 0
    assert got["pr"][:2] == [0.0, 0.0] and got["pr"][2] == 2 / 4 and got["cd"][:2] == [2 / 5, 2 / 5]
    assert got["q4"][:5] == [1, 1, 2, 3, 4] and got["q2"][:5] == [1, 1, 1, 2, 2]
    assert got["fv"][:5] == [cols["i64"][0]] * 5 and got["lv"][:5] == [cols["i64"][4]] * 5
    assert got["n2"][:5] == [None] + [cols["i64"][1]] * 4                         # the frame of row 0 has one row
    assert got["m2"][:5] == [None] + cols["i64"][:4]                              # the row before the current one
    assert got["n6"][:5] == [None] * 5 and got["n6"][5:64] == [cols["i64"][10]] * 59
    # partition 3 is one row (row 128): everything about it is the row itself
    assert frames[128] == (128, 128, 128, 128)
    assert (got["pr"][128], got["cd"][128], got["q4"][128], got["fv"][128], got["lv"][128], got["m1"][128], got["n2"][128]) == (
        0.0, 1.0, 1, cols["i64"][128], cols["i64"][128], cols["i64"][128], None)
    # partition 2: rows 64..127, a whole 64-row word; quarters of 16 rows
    assert got["q4"][64:128] == [1] * 16 + [2] * 16 + [3] * 16 + [4] * 16
    assert got["pr"][127] == (_peer_starts(frames)[127] - 64) / 63 and got["cd"][127] == 1.0
    # partition 4 (rows 129..131) holds no argument value: every pick is NULL
    assert got["fv"][129:132] == got["lv"][129:132] == got["m1"][129:132] == [None] * 3
    # the last row of the table ends its partition
    n = len(cols["o"])
    assert got["cd"][n - 1] == 1.0 and got["lv"][n - 1] == cols["i64"][n - 1] and got["q2"][n - 28:] == [1] * 14 + [2] * 14


def test_the_restatement_agrees_with_window_ref_where_they_overlap(table):
    cols, types, _ = table
    old = W.window(cols, types, PART, ORDER, [("rank", None, "rk", None), ("count", None, "rows", "partition"), ("count", None, "upto", "range_to_current")])
    got = V.window(cols, PART, ORDER, [("percent_rank", None, "pr", None), ("cume_dist", None, "cd", None)])
    assert got["pr"] == [(rk - 1) / max(rows - 1, 1) for rk, rows in zip(old["rk"], old["rows"])]
    assert got["cd"] == [upto / rows for upto, rows in zip(old["upto"], old["rows"])]
    for arg in WC.ARGS:
        for frame in V.FRAMES:
            r = V.window(cols, PART, ORDER, [("first_value", arg, "f", frame), ("last_value", arg, "l", frame), (("nth_value", 1), arg, "n1", frame),
                                             (("nth_value", -1), arg, "m1", frame)])
            same = lambda a, b: list(map(repr, a)) == list(map(repr, b))     # (repr: a NaN equals itself, -0.0 is not 0.0)
            assert same(r["n1"], r["f"]) and same(r["m1"], r["l"]), (arg, frame)


def _column(cols, frames, pick):
    """a value function written as pick(s, i, pe, e) -> row or None"""
    out = []
    for s, i, pe, e in frames:
        p = pick(s, i, pe, e)
        out.append(None if p is None else cols["i64"][p])
    return out


def test_each_plausible_mistake_changes_a_result_on_the_reference_table(table):
    cols, _, frames = table
    ps = _peer_starts(frames)
    want = V.window(cols, PART, ORDER, [
        ("percent_rank", None, "pr", None), ("cume_dist", None, "cd", None), (("ntile", 7), None, "q7", None), (("ntile", 10), None, "q10", None),
        ("last_value", "i64", "lv", None), ("last_value", "i64", "lv_rows", "rows_to_current"), (("nth_value", 2), "i64", "n2", None),
        (("nth_value", -2), "i64", "m2", None)])
    # the restatement itself, written from the frames: what the mistakes below are mistakes OF
    assert want["pr"] == [(ps[i] - s) / max(e - s, 1) for i, (s, _, _, e) in enumerate(frames)]
    assert want["cd"] == [(pe - s + 1) / (e - s + 1) for s, _, pe, e in frames]
    assert want["q7"] == [(i - s) * min(7, e - s + 1) // (e - s + 1) + 1 for s, i, _, e in frames]
    assert want["lv"] == _column(cols, frames, lambda s, i, pe, e: pe)
    assert want["m2"] == _column(cols, frames, lambda s, i, pe, e: pe - 1 if pe - 1 >= s else None)

    def larger_first(n_buckets):
        out = []
        for s, i, _, e in frames:
            rows = e - s + 1
            k = min(n_buckets, rows)
            q, r = divmod(rows, k)
            j = i - s
            out.append(j // (q + 1) + 1 if j < r * (q + 1) else r + (j - r * (q + 1)) // q + 1)
        return out
    mistakes = {
        "percent_rank over rows instead of rows - 1": ("pr", [(ps[i] - s) / (e - s + 1) for i, (s, _, _, e) in enumerate(frames)]),
        "cume_dist up to the row instead of its last peer": ("cd", [(i - s + 1) / (e - s + 1) for s, i, _, e in frames]),
        "ntile with the larger buckets first": ("q7", larger_first(7)),
        "ntile without min(n, rows)": ("q10", [(i - s) * 10 // (e - s + 1) + 1 for s, i, _, e in frames]),
        "last_value under the default frame is the row's own value": ("lv", _column(cols, frames, lambda s, i, pe, e: i)),
        "a ROWS frame taken as the partition": ("lv_rows", _column(cols, frames, lambda s, i, pe, e: e)),
        "nth_value counting from 0": ("n2", _column(cols, frames, lambda s, i, pe, e: s + 2 if s + 2 <= pe else None)),
        "a negative n counted from the partition's end": ("m2", _column(cols, frames, lambda s, i, pe, e: e - 1 if e - 1 >= s else None)),
    }
    for what, (name, wrong) in mistakes.items():
        assert len(wrong) == len(want[name]) and wrong != want[name], what
    # (i64 has a value at the head of every partition that has one at all; i32 begins partitions 5 and 6 with a NULL)
    fv32 = V.window(cols, PART, ORDER, [("first_value", "i32", "fv", None)])["fv"]
    skipping = [next((cols["i32"][j] for j in range(s, pe + 1) if cols["i32"][j] is not None), None) for s, _, pe, _ in frames]
    assert fv32[132] is None and fv32[172] is None and skipping != fv32, "first_value skipping NULLs"
    # and on the small tables ntile(4) itself tells the two conventions apart
    six = {"p": [1] * 6}
    assert V.window(six, ["p"], [], [(("ntile", 4), None, "q", None)])["q"] != [1, 1, 2, 2, 3, 4]
