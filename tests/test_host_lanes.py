"""The lane-level helpers that the rows kernels share (lewton_amd/csrc/lw_lanes.hpp), on the CPU: tests/san/lanes_host.cpp compiles
the header for the host under ASan/UBSan and holds each helper against the plainest restatement of what it promises -- bit lists
against a loop over single bits, the levels against the contract's recurrence (and the plan's scratch figure, by exact-size
buffers), the mask writer and the groups of the runs of four against "every byte / element once, nothing else".  The chunk load of
four floats stayed one copy per kernel file; tests/san/chunk_host.cpp holds both copies to one matrix of lengths and alignments."""
import os

import pytest

import host_harness as H


@pytest.fixture(scope="module")
def lanes(tmp_path_factory):
    return H.build(tmp_path_factory, "lanes_host", [os.path.join(H.SAN, "lanes_host.cpp")])


def test_count_first_and_last_over_every_range_of_three_192_bit_lists(lanes):
    """3 lists x 2 index types x 2 values of inv x every 0 <= lo < hi <= 192"""
    assert H.run(lanes, "bits") == ["OK bits %d" % (3 * 2 * 2 * (192 * 193 // 2))]


def test_levels_fold_in_the_order_of_normalising_rows(lanes):
    """1, 2, 64, 65, 4096 and 4097 doubles of mixed magnitude, scratch of exactly ceil(len / 64) + ceil(len / 4096) entries"""
    assert H.run(lanes, "levels") == ["OK levels 6"]


def test_the_mask_writer_writes_every_byte_of_its_span_once_and_nothing_else(lanes):
    """4 alignments of the line x 2 starts x 14 lengths x (n == 0, n < fill_end, n == fill_end)"""
    assert H.run(lanes, "mask") == ["OK mask %d" % (4 * 2 * 14 * 3)]


def test_every_element_of_a_line_lies_in_exactly_one_group_of_a_run(lanes):
    """2 line counts x 9 spans x 4 alignments of the destination x 2 of the source"""
    assert H.run(lanes, "runs") == ["OK runs %d" % (2 * 9 * 4 * 2)]


@pytest.fixture(scope="module")
def chunk(tmp_path_factory):
    return H.build(tmp_path_factory, "chunk_host", [os.path.join(H.SAN, "chunk_host.cpp")])


def test_both_chunk_loads_give_the_elements_and_read_nothing_at_or_beyond_n(chunk):
    """the two copies the kernels keep (k_norm_sum's, k_vad*'s): 4 alignments x 8 lengths x 2 chunks x 64 lanes"""
    assert H.run(chunk) == ["OK chunk %d" % (4 * 8 * 2 * 64)]
