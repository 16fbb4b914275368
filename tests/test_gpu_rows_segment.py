"""Segments of a frame mask and segment rows on the GPU (-m gpu): Segments.run (lw_segment_rows / k_segment_count, k_segment),
Segments.jobs and CutRows.run (lw_cut_rows / k_cut) against the numpy models of their contracts, and the chain from samples through
fbank, the energy VAD, the segments and the cut waveform to Whisper features per segment against the seven models composed.

The cases are in tests/rows_segment_gpu_cases.py and run ONCE, with pytest, in a process of their own that imports torch first
(tests/test_gpu_rows.py says why).  Each test below stands for one group of cases of that run (a function of the cases file with
all its parameters): every case of the group must have passed, and at least one must exist.  No case may skip."""
import pytest

import gpu_child

pytestmark = pytest.mark.gpu

CASES = "rows_segment_gpu_cases.py"
GROUPS = ["test_k_segment_is_the_model", "test_lengths_at_the_tile_seams", "test_runs_and_gaps_across_every_seam",
          "test_bytes_2_and_255_count_as_set_and_trivial_lines", "test_rows_and_channels_do_not_leak",
          "test_run_and_jobs_and_more_segments_than_seg_capacity", "test_calls_queued_back_to_back_on_one_stream_and_on_a_side_stream",
          "test_refusals_are_value_errors", "test_smoothed_mask_into_select_frames_is_the_two_models_composed",
          "test_k_cut_is_the_model_at_every_source_residue_and_length", "test_k_cut_long_jobs_repeated_and_overlapping",
          "test_cut_calls_queued_back_to_back_on_a_side_stream", "test_handle_lifecycle",
          "test_fbank_to_vad_to_segments_to_cut_waveform_to_whisper_features_is_the_models_composed"]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    return gpu_child.run_cases(tmp_path_factory, CASES, "rows_segment_gpu")


def test_every_group_of_the_cases_file_is_listed(child):
    assert sorted(child) == sorted(GROUPS)


@pytest.mark.parametrize("group", GROUPS)
def test_rows_segment(child, group):
    gpu_child.check_group(child, group)
