"""CPU: the numpy restatement of the reference's chunk labelling (tests/chunk_label_ref.py) equals, exactly, what the reference's
own get_labeledSTFT gave for the edge cases of tests/golden/chunk_labels.json (tools/gen_golden_chunk_labels.py), and the host
arithmetic of fs_eend_amd.device_data agrees with it."""
import numpy as np
import pytest

import chunk_label_ref as R
from fs_eend_amd import device_data as D

CASES = R.load_golden()


def test_golden_holds_the_required_cases():
    by = {c["name"]: c for c in CASES}
    assert by["covers_whole_chunk"]["T"].shape == (250, 1) and by["covers_whole_chunk"]["T"].sum() == 0
    assert by["starts_before_ends_inside"]["T"][:, 0].tolist() == [1] * 100 + [0] * 150
    assert by["starts_inside_runs_past"]["T"][:, 0].tolist() == [0] * 200 + [1] * 50
    assert by["entirely_inside"]["T"][:, 0].tolist() == [0] * 50 + [1] * 100 + [0] * 100
    assert by["start_frame_equals_end"]["T"][:, 0].sum() == 0 and by["start_frame_equals_end"]["T"][:20, 1].all()
    assert by["end_frame_equals_start"]["T"][:, 0].sum() == 0 and by["end_frame_equals_start"]["T"][200:, 1].all()
    t = by["rint_ties"]["T"]
    assert t[:, 0].argmax() == 12 and t[:, 1].argmax() == 14 and t[:, 2].tolist() == [0, 0] + [1] * 12 + [0] * 36      # 12.5 -> 12, 13.5 -> 14, 14.5 -> 14
    assert by["more_speakers_than_recorded"]["T"].shape == (250, 4) and by["more_speakers_than_recorded"]["T"][:, 2:].sum() == 0
    assert by["speaker_out_of_range"]["T"][:, 1:].sum() == 0 and by["speaker_out_of_range"]["T"][:, 0].sum() == 80
    assert by["file_ends_inside_odd"]["T"].shape == (151, 3) and by["file_ends_inside_even"]["T"].shape == (150, 3)
    assert by["starts_at_file_end"]["T"].shape == (0, 2)
    assert by["overlap_same_speaker"]["T"][:, 0].tolist() == [0] * 20 + [1] * 170 + [0] * 60


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_equals_reference(case):
    got = R.chunk_labels(case["segments"], case["utt2spk"], case["file_len"], case["start"], case["end"], case["n_speakers"])
    assert got.dtype == np.int32 and got.shape == case["T"].shape
    assert np.array_equal(got, case["T"])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_arithmetic_agrees(case):
    """device_data's chunk length, frame count, speaker order and segment frames are the restatement's."""
    n = R.chunk_length(case["file_len"], case["start"], case["end"])
    assert D.chunk_samples(case["file_len"], case["start"], case["end"])[1] == n
    assert D.chunk_frames(n) == R.frame_count(n) == case["T"].shape[0]
    c = D.DeviceCorpus("cuda:0")
    c.add("rec", np.zeros(case["file_len"], dtype=np.float32), case["segments"], case["utt2spk"])
    assert c.speakers["rec"] == R.speakers_of(case["segments"], case["utt2spk"])
    want = [(R.segment_frames(st), R.segment_frames(et), c.speakers["rec"].index(case["utt2spk"][u])) for u, st, et in case["segments"]]
    assert c._segrows == want
    assert c.reco2dur["rec"] == case["file_len"] / 8000


def test_frame_count_and_clipping():
    assert [R.frame_count(n) for n in (0, 1, 79, 80, 81, 160, 12013)] == [0, 1, 1, 1, 2, 2, 151]
    assert R.chunk_length(250 * 80 + 13, 100, 400) == 12013 and R.chunk_length(20000, 250, 500) == 0
    assert R.chunk_length(20000, 300, 500) == 0                      # a chunk past the end is empty, never negative
    assert D.chunk_samples(20000, 300, 500) == (20000, 0)
    with pytest.raises(IndexError):
        R.chunk_labels([("a", 0.0, 1.0), ("b", 0.5, 1.0)], {"a": "A", "b": "B"}, 8000, 0, 100, n_speakers=1)
