"""TEST INFRASTRUCTURE: key columns that are ascending but for one pair — the inputs on which a subtly wrong key statistic
(dfgpu_column_minmax / k_key_minmax: min, max, non-null count, strictly ascending, non-decreasing) would show.

The base key of n rows is k[i] = lo + step * i (step 3; 1 for UInt8, whose 256 values hold no more).  The order shapes over it:
  clean          the base key                                            ascending, non-decreasing
  equal_at(p)    k[p] = k[p-1]                                           non-decreasing only
  descent_at(p)  k[p] and k[p-1] swapped                                 neither
  runs           every key 1-5 times in a row                            non-decreasing only
  null_at(q)     a NULL at row q of clean                                neither
Every type's cases start at the type's minimum (`at_min`) and end at its maximum (`to_max`); UInt32 also crosses 2^31 (`cross`), where an
unsigned key read as a signed one turns an ascent into a descent.

k_key_minmax runs at most 512 workgroups of 256 threads, each thread taking 4 strided rows per trip of its loop: LARGE =
512 * 256 * 4 + 1025 rows is the smallest size at which a thread makes a second trip and the clamped tail loads are taken on that trip."""
import pyarrow as pa

from tests import edge_values as E

TYPES = {"int32": pa.int32(), "date32": pa.date32(), "uint8": pa.uint8(), "uint32": pa.uint32(), "int64": pa.int64()}
GRID, BLOCK, UNROLL = 512, 256, 4
LARGE = GRID * BLOCK * UNROLL + 1025
SMALL_SIZES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 4097]
SIZES = SMALL_SIZES + [LARGE]


def type_range(typ):
    return (0, 255) if typ == pa.uint8() else E.type_range(typ)


def step_of(typ) -> int:
    return 1 if typ == pa.uint8() else 3


def sizes_of(typ) -> list:
    """the sizes whose base key fits the type (UInt8: n <= 256)"""
    lo, hi = type_range(typ)
    return [n for n in SIZES if step_of(typ) * (n - 1) <= hi - lo and (typ != pa.uint8() or n <= 256)]


def positions(n: int) -> list:
    """where the one flaw sits: around the wave (64) and workgroup (256) edges, the middle, the last row; at LARGE also the last row of
    the first trip's first stride, the first row of its second stride, and the first row of the second trip"""
    ps = [1, 63, 64, 255, 256, 257, n // 2, n - 1]
    if n >= LARGE:
        ps += [GRID * BLOCK - 1, GRID * BLOCK, UNROLL * GRID * BLOCK]
    out = []
    for p in ps:
        if 1 <= p < n and p not in out:
            out.append(p)
    return out


def lows(typ, n: int) -> dict:
    """{name: lo}: the base key starting at the type's minimum, ending at its maximum, and (UInt32) crossing 2^31"""
    tmin, tmax = type_range(typ)
    out = {"at_min": tmin, "to_max": tmax - step_of(typ) * (n - 1)}
    if typ == pa.uint32():
        out["cross"] = 2**31 - 1 - 3 * (n // 8)
    return out


def clean(lo: int, n: int, step: int = 3) -> list:
    return [lo + step * i for i in range(n)]


def equal_at(keys: list, p: int) -> list:
    out = list(keys)
    out[p] = out[p - 1]
    return out


def descent_at(keys: list, p: int) -> list:
    out = list(keys)
    out[p], out[p - 1] = out[p - 1], out[p]
    return out


def null_at(keys: list, q: int) -> list:
    out = list(keys)
    out[q] = None
    return out


def runs(lo: int, n: int, step: int = 3) -> list:
    """every key 1-5 times in a row (the first one twice, so that two rows already hold a repeat)"""
    out, j = [], 0
    while len(out) < n:
        out += [lo + step * j] * (1 + (j * 7 + 1) % 5)
        j += 1
    return out[:n]


def column(values: list, typ) -> pa.Array:
    if typ == pa.date32():
        return pa.array(values, pa.int32()).cast(pa.date32())
    return pa.array(values, typ)


def order_cases(typ, n: int, rotate: bool = False) -> list:
    """[(id, values, (ascending, nondecreasing))] — every order shape over n rows of `typ`, each from every start of lows(); with
    `rotate` every shape takes ONE of the starts in turn (the large size: each start is still taken by every kind of shape)"""
    step = step_of(typ)
    starts = list(lows(typ, n).items())
    shapes = [("clean", None, list, (True, True))]
    if n >= 2:
        shapes.append(("runs", None, None, (False, True)))
    for p in positions(n):
        shapes.append((f"equal_at_{p}", p, lambda k, p=p: equal_at(k, p), (False, True)))
        shapes.append((f"descent_at_{p}", p, lambda k, p=p: descent_at(k, p), (False, False)))
    for q in ([0] + positions(n) if n < LARGE else [0, GRID * BLOCK, n // 2, n - 1]):
        shapes.append((f"null_at_{q}", q, lambda k, q=q: null_at(k, q), (False, False)))
    out = []
    base = {lname: clean(lo, n, step) for lname, lo in starts}
    for s, (name, _, make, want) in enumerate(shapes):
        mine = [starts[(s // 2) % len(starts)]] if rotate and name not in ("clean", "runs") else starts
        for lname, lo in mine:
            values = runs(lo, n, step) if make is None else make(base[lname])
            out.append((f"{name}-{lname}", values, want))
    return out


# ------------------------------------------------------------------------------- membership: key sets, build sides, probe sides
# A key set maps a slot number to a key: even slots are what build sides hold, odd slots lie between them (absent keys inside the
# build's range), negative slots below its minimum, slots from 2 * SLOTS on above its maximum.
KEY_SETS = ["int64", "int32", "date32", "uint32", "uint8", "i32_i64", "dec20_2", "f64", "utf8", "dict", "bool"]
INTEGER_SETS = ("int64", "int32", "date32", "uint32", "uint8")
WIDE_SETS = ("i32_i64", "dec20_2", "f64")
STRING_SETS = ("utf8", "dict", "bool")
PROBE_SIZES = [0, 1, 63, 64, 65, 1025, 4097]
BUILD_SIDES = ["empty", "one", "many", "many_valid"]
F64_SPECIAL = [0x0000000000000000, 0x8000000000000000, 0x7FF8000000000000, 0xFFF8000000000000]   # +0.0, -0.0, NaN, -NaN: slots 0-3


def slots_of(key_set: str) -> int:
    """how many even slots a build side draws from"""
    return {"uint8": 100, "bool": 1}.get(key_set, 3000)


def key_types(key_set: str) -> list:
    return {"int64": [pa.int64()], "int32": [pa.int32()], "date32": [pa.date32()], "uint32": [pa.uint32()], "uint8": [pa.uint8()],
            "i32_i64": [pa.int32(), pa.int64()], "dec20_2": [pa.decimal128(20, 2)], "f64": [pa.float64()], "utf8": [pa.string()],
            "dict": [pa.dictionary(pa.int32(), pa.string())], "bool": [pa.bool_()]}[key_set]


def key_of(key_set: str, slot: int) -> tuple:
    """the key (one raw value per column) of a slot: integers, day numbers, unscaled decimals, float bits, strings, bools"""
    if key_set == "int64":
        return (-5_000_000_000 + slot,)              # negative, beyond 32 bits
    if key_set == "int32":
        return (-1000 + slot,)
    if key_set == "date32":
        return (9000 + slot,)
    if key_set == "uint32":
        return (2**31 - 1000 + slot,)                # crosses 2^31
    if key_set == "uint8":
        return (8 + slot,)                           # slots -8 .. 247
    if key_set == "i32_i64":
        return (slot % 37 - 18, -(2**40) + slot // 37)
    if key_set == "dec20_2":
        return (3 * 10**18 + slot,)                  # unscaled, beyond 64 bits
    if key_set == "f64":
        return (F64_SPECIAL[slot] if 0 <= slot < 4 else E.f64_bits(slot * 0.25),)
    if key_set in ("utf8", "dict"):
        return (f"key{slot + 10:06d}",)
    return (slot % 2 == 0,)                          # bool: True is the build's key, False the absent one


def _array(raw: list, typ, reverse_dictionary=False) -> pa.Array:
    """raw values (None = NULL) of one key column as an Arrow array, bit-exact"""
    if pa.types.is_float64(typ) or pa.types.is_decimal128(typ):
        return E.from_raw([0 if v is None else v for v in raw], typ, [v is None for v in raw])
    if pa.types.is_dictionary(typ):
        values = sorted({v for v in raw if v is not None}, reverse=reverse_dictionary)
        at = {v: i for i, v in enumerate(values)}
        return pa.DictionaryArray.from_arrays(pa.array([None if v is None else at[v] for v in raw], pa.int32()), pa.array(values, pa.string()))
    return column(raw, typ)


def key_table(key_set: str, slots: list, nulls: list, prefix: str, row_name: str, reverse_dictionary=False) -> pa.Table:
    """rows of the given slots; nulls[r] = None, or the key column that is NULL in row r; plus the row number as a payload column"""
    types = key_types(key_set)
    cols = [[] for _ in types]
    for s, nul in zip(slots, nulls):
        key = key_of(key_set, s)
        for c in range(len(types)):
            cols[c].append(None if nul == c else key[c])
    data = {f"{prefix}{c}": _array(cols[c], t, reverse_dictionary) for c, t in enumerate(types)}
    data[row_name] = pa.array(list(range(len(slots))), pa.int64())
    return pa.table(data)


def build_side(key_set: str, which: str, unique: bool, rng) -> pa.Table:
    """`empty`, `one` row, or `many`: 3 000 rows (as many as the key set has slots for when fewer) with duplicate keys — `unique`: every
    key once, in no order — and NULL keys among them; `many_valid`: the same without a NULL key"""
    ncols = len(key_types(key_set))
    if which == "empty":
        slots = []
    elif which == "one":
        slots = [0]
    else:
        m = slots_of(key_set)
        if unique:
            slots = [2 * int(s) for s in rng.permutation(m)]
        else:
            slots = [2 * int(s) for s in rng.integers(0, max(1, m // 3), 3000)] + [2 * (m - 1), 0]
    nulls = [int(rng.integers(0, ncols)) if which == "many" and rng.random() < 0.03 else None for _ in slots]
    if which == "many":     # (at least one NULL key, whatever the draws gave)
        slots, nulls = slots + [0], nulls + [0]
    return key_table(key_set, slots, nulls, "k", "b_row")


def probe_side(key_set: str, n: int, rng) -> pa.Table:
    """n rows: about half on even slots (keys a `many` build side may hold), the others on odd slots, just below the lowest and just
    above the highest slot; 5 % of the rows have a NULL key component.  Dictionary keys use another dictionary than the build side."""
    m, ncols = slots_of(key_set), len(key_types(key_set))
    slots = []
    for _ in range(n):
        u = rng.random()
        if key_set == "bool":
            slots.append(int(u < 0.5))
        elif u < 0.47:
            slots.append(2 * int(rng.integers(0, max(1, m // 3))))    # (the third of the slots a build side with duplicates draws from)
        elif u < 0.90:
            slots.append(2 * int(rng.integers(0, m)) + 1)
        elif u < 0.95:
            slots.append(-1 - int(rng.integers(0, 4)))
        else:
            slots.append(2 * m + int(rng.integers(0, 4)))
    nulls = [int(rng.integers(0, ncols)) if rng.random() < 0.05 else None for _ in slots]
    return key_table(key_set, slots, nulls, "j", "p_row", reverse_dictionary=True)


def key_names(key_set: str):
    n = len(key_types(key_set))
    return [f"k{c}" for c in range(n)], [f"j{c}" for c in range(n)]


# ------------------------------------------------------------------------------------------ the dynamic filter through the node
ROW_GROUP = 1000
PROBE_ROWS = 12 * ROW_GROUP
NULL_GROUP = 5
DYNAMIC_KEY_TYPES = {"int64": pa.int64(), "int32": pa.int32()}


def dynamic_probe(key_type) -> pa.Table:
    """12 000 rows = 12 row groups of 1 000: `l_k` nullable and ascending with every key three times (a NULL every 97th row), row
    group 5 NULL throughout (no min / max in its statistics); a payload and a string column"""
    keys = [None if (i // ROW_GROUP == NULL_GROUP or i % 97 == 13) else i // 3 for i in range(PROBE_ROWS)]
    return pa.table({"l_k": column(keys, key_type), "l_pay": pa.array([i * 7 % 50 for i in range(PROBE_ROWS)], pa.int32()),
                     "l_tag": pa.array([["a", "bb", "ccc"][i % 3] for i in range(PROBE_ROWS)], pa.string())})


def write_dynamic_probe(table: pa.Table, path: str) -> str:
    import pyarrow.parquet as pq
    pq.write_table(table, path, row_group_size=ROW_GROUP, compression="snappy")
    return path


DYNAMIC_BUILDS = ["clustered", "far_apart", "two_clusters", "empty", "all_null", "below", "clustered_join_filter"]


def dynamic_build(which: str, key_type) -> pa.Table:
    keys = {"clustered": list(range(2100, 2500)),                              # the bounds prune
            "far_apart": [10, 2500, 3990, 10, None],                           # the IN list prunes between the bounds
            "two_clusters": list(range(300, 450)) + list(range(3500, 3650)),   # beyond 150 distinct keys: the Map strategy
            "empty": [], "all_null": [None] * 5,
            "below": list(range(-100, 0)),                                     # below every probe key
            "clustered_join_filter": list(range(2100, 2500))}[which]
    return pa.table({"o_k": column(keys, key_type), "o_pay": pa.array([i * 11 % 50 for i in range(len(keys))], pa.int32())})
