"""The definition of bit_and / bit_or / bit_xor and bool_and / bool_or (functions-aggregate bit_and_or_xor.rs, bool_and_or.rs) in
plain numpy, and the inputs the tests feed both to it and to the device.

Per group the non-NULL values are reduced with the operation at the argument's width; a group without a non-NULL value gives None.
A partial state is such a result (None = nothing seen yet) and states merge with the same operation — XOR with XOR.

AND and OR are idempotent: a row that is lost, or read twice, changes nothing unless the row is a WITNESS — the only row of its group
that clears a bit (AND) or sets it (OR).  `family` builds such rows at the places where an accumulation goes wrong: rows 0, 63, 64,
65 and the last row of the table (the edges of a wave's 64-row words) and the first and last row of every group (of every run, where
the groups are runs).  XOR needs no witness: any row lost or read twice changes its group's result."""
import numpy as np
import pyarrow as pa

BIT_FUNCS = ("bit_and", "bit_or", "bit_xor")
BOOL_FUNCS = ("bool_and", "bool_or")
FUNCS = BIT_FUNCS + BOOL_FUNCS
INT_TYPES = {"int32": pa.int32(), "int64": pa.int64(), "uint8": pa.uint8(), "uint32": pa.uint32(), "uint64": pa.uint64()}
NULL_FRACTIONS = (0.0, 0.1)
WORD_EDGE_ROWS = (0, 63, 64, 65)

_UFUNC = {"bit_and": np.bitwise_and, "bit_or": np.bitwise_or, "bit_xor": np.bitwise_xor, "bool_and": np.logical_and, "bool_or": np.logical_or}


def np_dtype(typ):
    return np.dtype(bool) if pa.types.is_boolean(typ) else np.dtype(typ.to_pandas_dtype())


def width(typ):
    return 1 if pa.types.is_boolean(typ) else typ.bit_width


def edge_values(typ):
    """0, all ones, the sign bit alone (= INT_MIN for a signed type), the largest positive value"""
    if pa.types.is_boolean(typ):
        return [False, True]
    w = typ.bit_width
    if pa.types.is_signed_integer(typ):
        return [0, -1, -2**(w - 1), 2**(w - 1) - 1]
    return [0, 2**w - 1, 2**(w - 1), 2**(w - 1) - 1]


def from_pattern(bits, typ):
    """unsigned bit patterns (uint64, below 2^width) -> values of the type"""
    dt = np_dtype(typ)
    if dt == bool:
        return (np.asarray(bits, np.uint64) & np.uint64(1)).astype(bool)
    return np.asarray(bits, np.uint64).astype(np.dtype(f"uint{dt.itemsize * 8}")).view(dt)


def reduce_groups(func, gids, values, valid, typ):
    """{group: result as a Python int / bool, None where the group has no non-NULL value}"""
    gids = np.asarray(gids)
    values = np.asarray(values, np_dtype(typ))
    out = {int(g): None for g in np.unique(gids)}
    keep = np.ones(len(gids), bool) if valid is None else np.asarray(valid, bool)
    g, v = gids[keep], values[keep]
    if len(g) == 0:
        return out
    order = np.argsort(g, kind="stable")
    g, v = g[order], v[order]
    starts = np.flatnonzero(np.r_[True, g[1:] != g[:-1]])
    red = _UFUNC[func].reduceat(v, starts)
    assert red.dtype == np_dtype(typ), (red.dtype, typ)             # the reduction stays at the argument's width
    for gg, r in zip(g[starts], red):
        out[int(gg)] = r.item()
    return out


def merge(func, a, b):
    """two partial states (None = nothing seen) -> one"""
    if a is None or b is None:
        return b if a is None else a
    if func in BOOL_FUNCS:
        return (a and b) if func == "bool_and" else (a or b)
    return a & b if func == "bit_and" else a | b if func == "bit_or" else a ^ b          # Python ints: two's complement of any width


def witness_rows(gids):
    """{group: its witness rows, ascending}: the group's first and last row, and rows 0 / 63 / 64 / 65 / n - 1 of the table"""
    gids = np.asarray(gids)
    n = len(gids)
    rows = dict()
    uniq, first = np.unique(gids, return_index=True)
    _, last_rev = np.unique(gids[::-1], return_index=True)
    for g, f, l in zip(uniq, first, n - 1 - last_rev):
        rows[int(g)] = {int(f), int(l)}
    for r in WORD_EDGE_ROWS + (n - 1,):
        if 0 <= r < n:
            rows[int(gids[r])].add(int(r))
    return {g: sorted(rs) for g, rs in rows.items()}


def all_null_group(gids):
    """the group `family` leaves without a value when it makes NULLs: the largest group number (None where there is one group only)"""
    return int(np.max(gids)) if len(gids) and np.min(gids) != np.max(gids) else None


def family(func, typ, gids, null_frac, seed=0):
    """-> (values, valid or None, {row: group} of the witnesses).  bit_and / bool_and: every other row of a group has the witnesses'
    bits set, a witness all bits but its own; bit_or / bool_or: the mirror image; bit_xor: random values, the type's edge values among
    them.  A Boolean has one bit: one witness per group (the candidates taken in turn from group to group), none in every third group,
    so both results occur.  NULLs (about null_frac of the rows that are no witness, and the whole last group) keep a value under them
    that would change the result if it were read: 0 for AND, all ones for OR, a random one for XOR."""
    gids = np.asarray(gids)
    n, w = len(gids), width(typ)
    rng = np.random.default_rng([seed, w, FUNCS.index(func)])
    full = np.uint64(2**w - 1)
    rand = rng.integers(0, 2**64, n, dtype=np.uint64) & full
    bits = rand.copy()
    witnesses = {}
    is_and = func in ("bit_and", "bool_and")
    dead = all_null_group(gids) if null_frac > 0 else None
    if func != "bit_xor":
        uniq, inv = np.unique(gids, return_inverse=True)
        group_mask = np.zeros(len(uniq), np.uint64)
        chosen = []
        for gi, (g, rows) in enumerate(sorted(witness_rows(gids).items())):
            if g == dead:
                continue
            if w == 1:
                rows = [] if g % 3 == 2 else [rows[(g // 3) % len(rows)]]
            rows = rows[:w]
            wbits = [(g + j) % w for j in range(len(rows))]
            group_mask[gi] = 1 if w == 1 else sum(1 << b for b in wbits)      # (a Boolean group without a witness is all true / all false)
            chosen += [(r, b, g) for r, b in zip(rows, wbits)]
        row_mask = group_mask[inv]
        bits = (rand | row_mask) if is_and else (rand & (full ^ row_mask))
        for r, b, g in chosen:
            bits[r] = (full ^ np.uint64(1 << b)) if is_and else np.uint64(1 << b)
            witnesses[r] = g
    else:
        edges = np.array([v & (2**w - 1) for v in edge_values(typ)], np.uint64)
        at = rng.permutation(n)[:min(n, 4 * len(edges))]
        bits[at] = edges[np.arange(len(at)) % len(edges)]
    valid = None
    if null_frac > 0:
        valid = rng.random(n) >= null_frac
        valid[list(witnesses)] = True
        if dead is not None:
            valid[gids == dead] = False
        if func != "bit_xor":
            bits[~valid] = np.uint64(0) if is_and else full
    return from_pattern(bits, typ), valid, witnesses


def to_arrow(values, valid, typ):
    """the values as an Arrow array; what lies under a NULL stays in the data buffer"""
    return pa.array(np.asarray(values, np_dtype(typ)), typ, mask=None if valid is None else ~np.asarray(valid, bool))
