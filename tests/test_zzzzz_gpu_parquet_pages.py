"""The Parquet page decoders of csrc/parquet.hip against hand-built pages (tests/parquet_page_cases.py): every case is decoded through
ParquetFile.read_row_group and through read_table, by the kernels that read the pages themselves (k_pq_levels / k_pq_decode_pages, the
default) and by the host-planned kernel (k_pq_decode, parquet.device_decode=0), and compared — validity, values, for Float64 the bits —
with the values the pages were BUILT from: never with the other path, and not with another reader's decode of the same bytes (that
pyarrow reads these files as the same values is tests/test_parquet_page_reference.py's business).  The profile says which half ran."""
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from tests.parquet_page_cases import NAMES, case, column_values

pytestmark = pytest.mark.gpu

MODES = [(n, m) for n in NAMES for m in ("device", "host") + (("snappy_on_the_device",) if "snappy" in n else ())]
KERNELS = {"parquet_decode_pages", "parquet_levels", "parquet_decode", "parquet_decompress_pages"}


def _decode(path, how):
    """-> (arrow table, the names under which kernels were profiled)"""
    from datafusion_amd import ops
    from datafusion_amd import parquet as P
    P.CACHE.clear()          # (decode, do not serve the chunk from the device cache)
    ops.profile_enable(True)
    ops.profile_reset()
    try:
        if how == "read_row_group":
            f = P.ParquetFile(path)
            try:
                got = f.read_row_group(0).to_arrow()
            finally:
                f.close()
        else:
            got = P.read_table(path).to_arrow()
        return got, set(ops.profile_stats())
    finally:
        ops.profile_enable(False)
        P.CACHE.clear()


@pytest.mark.parametrize("name,mode", MODES, ids=[f"{n}-{m}" for n, m in MODES])
def test_pages_decode_to_the_values_they_were_built_from(tmp_path, name, mode):
    from datafusion_amd import ops
    c = case(name)
    path = str(tmp_path / "case.parquet")
    with open(path, "wb") as f:
        f.write(c.data)
    if mode == "host":
        ops.set_options(parquet__device_decode="0")
    elif mode == "snappy_on_the_device":
        ops.set_options(parquet__snappy="device")
    want_type = pq.read_schema(path).field("c").type
    for how in ("read_row_group", "read_table"):
        got, ran = _decode(path, how)
        assert got.column_names == ["c"] and got.num_rows == len(c.values), (how, got.schema)
        t = got.schema.field("c").type
        if c.kind == "dict_utf8":
            assert pa.types.is_dictionary(t), (how, t)
        elif c.kind == "utf8":
            assert pa.types.is_string(t) or pa.types.is_large_string(t), (how, t)
        else:
            assert t == want_type, (how, t, want_type)
        values = column_values(got.column("c"))
        wrong = [i for i, (a, b) in enumerate(zip(values, c.values)) if a != b]
        assert not wrong, (how, len(wrong), [(i, values[i], c.values[i]) for i in wrong[:5]])
        assert got.column("c").null_count == c.counts["nulls"], how
        # which half ran
        ran &= KERNELS
        if c.kind in ("bool", "utf8"):
            assert not ran, (how, ran)                    # planned and decoded on the host (bits / offsets), no page kernel
        elif mode == "host":
            assert ran == {"parquet_decode"}, (how, ran)
        else:
            want = {"parquet_decode_pages"} | ({"parquet_levels"} if c.optional else set()) | ({"parquet_decompress_pages"} if mode == "snappy_on_the_device" else set())
            assert ran == want, (how, ran, want)
