"""Independent numpy restatement of how the reference labels a training chunk (LS-EEND/datasets/feature.py:255-322
get_labeledSTFT with the file access of datasets/kaldi_data.py:68-90): the chunk's sample count as soundfile clips it, its STFT
frame count (feature.py:166-191) and the label rule, frame by frame.  tests/golden/chunk_labels.json (made by
tools/gen_golden_chunk_labels.py from the reference's own function) pins it; the device path is compared with it."""
import json
import os

import numpy as np


def chunk_length(file_len, start, end, frame_shift=80):
    """Samples sf.read(start=start * shift, stop=end * shift) returns from a file of file_len samples."""
    a = min(start * frame_shift, file_len)
    b = min(end * frame_shift, file_len)
    return max(b - a, 0)


def frame_count(n_samples, frame_shift=80):
    """Rows of stft(): librosa's centred 1 + n // hop frames, the last one dropped when n is a multiple of the hop."""
    n = 1 + n_samples // frame_shift
    return n - 1 if n_samples % frame_shift == 0 else n


def segment_frames(seconds, rate=8000, frame_shift=80):
    return int(np.rint(np.float64(seconds) * rate / frame_shift))        # half to even


def speakers_of(segments, utt2spk):
    return sorted(set(utt2spk[utt] for utt, _, _ in segments))


def chunk_labels(segments, utt2spk, file_len, start, end, n_speakers=None, rate=8000, frame_shift=80):
    """(rows, n_speakers) int32 labels of chunk [start, end) (STFT frames) of a recording with `segments`
    [(utt, st_seconds, et_seconds)].  IndexError when n_speakers is smaller than the recording's speaker count."""
    rows = frame_count(chunk_length(file_len, start, end, frame_shift), frame_shift)
    spk = speakers_of(segments, utt2spk)
    S = len(spk) if n_speakers is None else n_speakers
    if S < len(spk):
        raise IndexError("n_speakers is smaller than the recording's speaker count")
    T = np.zeros((rows, S), dtype=np.int32)
    for utt, st, et in segments:
        col = spk.index(utt2spk[utt])
        sf, ef = segment_frames(st, rate, frame_shift), segment_frames(et, rate, frame_shift)
        starts_inside = start <= sf < end
        ends_inside = start < ef <= end
        if not (starts_inside or ends_inside):
            continue                                    # also a segment that covers the whole chunk
        for t in range(rows):
            f = start + t                                # the frame's index in the recording
            if (not starts_inside or f >= sf) and (not ends_inside or f < ef):
                T[t, col] = 1
    return T


def subsampled(T, subsampling):
    return np.ascontiguousarray(T[::subsampling]).astype(np.float32)


def load_golden():
    """The cases of tests/golden/chunk_labels.json, each with its expected (rows, speakers) int32 matrix as case["T"]."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chunk_labels.json")) as f:
        g = json.load(f)
    assert (g["rate"], g["frame_shift"], g["frame_size"]) == (8000, 80, 200)
    for c in g["cases"]:
        c["segments"] = [tuple(s) for s in c["segments"]]
        c["T"] = np.array([[int(ch) for ch in col] for col in c["labels"]], dtype=np.int32).reshape(c["shape"][1], c["shape"][0]).T
    return g["cases"]
