"""The hand-built pages of tests/parquet_page_cases.py, without a GPU: pyarrow's reader — an independent production decoder — must read
every file of the spec-level writer (tests/parquet_pages.py) back as exactly the values it was built from, and the library's host half
(dfgpu_parquet_inspect_chunk: page headers, decompression, levels, run headers) must count in it what the case put there."""
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from tests.parquet_page_cases import NAMES, case, column_values

COUNTED = ("values", "nulls", "dictionary_values", "n_dictionary_pages", "n_data_pages_v1", "n_data_pages_v2", "n_plain_pages", "n_dictionary_encoded_pages",
           "n_runs_rle", "n_runs_bitpacked")


@pytest.mark.parametrize("name", NAMES)
def test_pyarrow_reads_the_values_the_case_was_built_from(name):
    c = case(name)
    got = pq.read_table(pa.BufferReader(c.data))
    assert got.column_names == ["c"] and got.num_rows == len(c.values)
    assert column_values(got.column("c")) == c.values


@pytest.mark.parametrize("name", NAMES)
def test_host_half_counts_what_the_case_holds(tmp_path, name):
    from datafusion_amd.parquet import ParquetFile
    c = case(name)
    path = str(tmp_path / "case.parquet")
    with open(path, "wb") as f:
        f.write(c.data)
    f = ParquetFile(path)
    try:
        info = f.inspect_chunk(0, "c")
    finally:
        f.close()
    assert {k: info[k] for k in COUNTED} == c.counts
    assert info["n_pages"] == c.counts["n_dictionary_pages"] + c.counts["n_data_pages_v1"] + c.counts["n_data_pages_v2"]
    if c.codec == "none":
        assert info["compressed_bytes"] == info["uncompressed_bytes"]


def test_run_counts_of_the_run_stream_cases():
    """the counts the cases carry follow their run lists; these two are spelled out: 300 x [packed 8, RLE 3], and packed 4096 / RLE 500 / packed 77"""
    b1, b2 = case("B1_600_run_headers").counts, case("B2_packed_run_longer_than_the_window").counts
    assert (b1["n_runs_rle"], b1["n_runs_bitpacked"]) == (300, 300) and (b2["n_runs_rle"], b2["n_runs_bitpacked"]) == (1, 2)


def test_delta_cases_hold_the_miniblock_widths_they_are_named_for():
    assert case("D_widths_int64_ascending").widths == list(range(65)) + [0, 0, 0]
    assert case("D_widths_int64_descending").widths == list(range(64, -1, -1)) + [0, 0, 0]
    assert case("D_widths_int32_ascending").widths == list(range(33)) + [0, 0, 0]
    assert case("D_widths_int32_descending").widths == list(range(32, -1, -1)) + [0, 0, 0]
    assert len(case("D_400_miniblocks").widths) == 400
    last = case("D_shape_4096_64_count_three_blocks_one_miniblock_one").widths[3 * 64:]
    assert len(last) == 64 and last[0] > 0 and last[1] > 0 and last[2:] == [0] * 62      # one full miniblock, one value of the next, 62 unused
