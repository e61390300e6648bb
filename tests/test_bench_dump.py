"""bench.py --dump-outputs, the parts that need no GPU: the fixed row sample of a large output (chosen by a hash of its key, so the
same rows whatever order the output comes in), the canonical row order, decimals' 128-bit words, and the host conversion of a small
result to float64 arrays."""
import datetime
import decimal

import numpy as np
import pyarrow as pa
import torch

import bench
from datafusion_amd import table as T


def test_the_sample_does_not_depend_on_row_order():
    rng = np.random.default_rng(7)
    key = torch.from_numpy(rng.integers(1, 6_000_000, size=200_000))
    perm = torch.from_numpy(rng.permutation(key.numel()))
    a = bench.sample_rows(key, 37, 5, chunk=4096)
    b = bench.sample_rows(key[perm], 37, 5, chunk=4096)
    assert torch.equal(torch.sort(key[a]).values, torch.sort(key[perm][b]).values)
    assert 200_000 / 37 * 0.8 < a.numel() < 200_000 / 37 * 1.2
    assert torch.equal(a, torch.sort(a).values) and bench.sample_rows(key, 1, 0).numel() == key.numel()


def test_canonical_order_sorts_by_every_column_first_most_significant():
    rng = np.random.default_rng(1)
    cols = [torch.from_numpy(rng.integers(0, 4, size=5000).astype(np.float64)) for _ in range(3)]
    order = bench.canonical_order(cols)
    rows = list(zip(*(c[order].tolist() for c in cols)))
    assert rows == sorted(zip(*(c.tolist() for c in cols)))


def test_decimal128_words_become_their_values():
    vals = [0, 1, -1, 12345, -9876543210, 2 ** 63 + 5, -(2 ** 70)]
    words = torch.tensor([[v & (2 ** 64 - 1), (v >> 64) & (2 ** 64 - 1)] for v in vals], dtype=torch.uint64).view(torch.int64)
    assert bench._as_f64(T.DECIMAL128, words).tolist() == [float(v) for v in vals]
    assert bench._as_f64(T.UINT32, torch.tensor([-1, 7], dtype=torch.int32)).tolist() == [2.0 ** 32 - 1, 7.0]


def test_host_arrays_of_a_small_result():
    tab = pa.table({"flag": pa.array(["A", "NO", None]).dictionary_encode(),
                    "price": pa.array([decimal.Decimal("1.25"), decimal.Decimal("-3.50"), None], pa.decimal128(15, 2)),
                    "day": pa.array([datetime.date(1970, 1, 2), datetime.date(1969, 12, 31), datetime.date(1995, 3, 15)]),
                    "n": pa.array([1, 2, 3], pa.int64())})
    out = bench.host_arrays(tab)
    assert all(a.dtype == np.float64 for a in out.values())
    assert out["flag"].shape == (3, 2) and out["flag"][0].tolist() == [65.0, 0.0] and out["flag"][1].tolist() == [78.0, 79.0] and np.isnan(out["flag"][2]).all()
    assert out["price"][:2].tolist() == [1.25, -3.5] and np.isnan(out["price"][2])
    assert out["day"].tolist() == [1.0, -1.0, float((datetime.date(1995, 3, 15) - datetime.date(1970, 1, 1)).days)]
    assert out["n"].tolist() == [1.0, 2.0, 3.0]
