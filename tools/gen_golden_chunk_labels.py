#!/usr/bin/env python3
"""Regenerate tests/golden/chunk_labels.json: the label matrices the reference's own get_labeledSTFT
(LS-EEND/datasets/feature.py:255-322) gives for the chunk / segment edge cases listed below.

    python tools/gen_golden_chunk_labels.py /path/to/reference

The reference's feature.py is loaded from the given checkout with `librosa` and `soundfile` stubbed as empty modules (neither is
needed for labels), its `stft` replaced by a stand-in that returns an array with the right number of rows, and a stand-in Kaldi
object whose `load_wav` returns as many zero samples as soundfile would (clipped at the end of the file).  Everything else --
speaker order, rounding, the comparisons, the slice assignment -- is the reference's code."""
import importlib.util
import json
import os
import sys
import types

import numpy as np

RATE, SHIFT, SIZE = 8000, 80, 200
LONG = 160000                   # 20 s: 2000 frames

# name, segments [(utt, st, et)], utt2spk, file_len, start, end, n_speakers
CASES = [
    ("covers_whole_chunk", [("a1", 0.0, 100.0)], {"a1": "A"}, LONG, 1000, 1250, None),
    ("starts_before_ends_inside", [("a1", 9.0, 11.0)], {"a1": "A"}, LONG, 1000, 1250, None),
    ("starts_inside_runs_past", [("a1", 12.0, 20.0)], {"a1": "A"}, LONG, 1000, 1250, None),
    ("entirely_inside", [("a1", 10.5, 11.5)], {"a1": "A"}, LONG, 1000, 1250, None),
    ("start_frame_equals_end", [("a1", 12.5, 13.0), ("b1", 10.0, 10.2)], {"a1": "A", "b1": "B"}, LONG, 1000, 1250, None),
    ("end_frame_equals_start", [("a1", 9.0, 10.0), ("b1", 12.0, 12.5)], {"a1": "A", "b1": "B"}, LONG, 1000, 1250, None),
    ("rint_ties", [("a1", 0.125, 0.2), ("b1", 0.135, 0.3), ("c1", 0.02, 0.145)], {"a1": "A", "b1": "B", "c1": "C"}, LONG, 0, 50, None),
    ("overlap_same_speaker", [("a1", 10.2, 11.0), ("a2", 10.8, 11.9), ("b1", 9.5, 10.4)], {"a1": "A", "a2": "A", "b1": "B"},
     LONG, 1000, 1250, None),
    ("speaker_out_of_range", [("a1", 10.1, 10.9), ("b1", 2.0, 3.0), ("c1", 15.0, 16.0)], {"a1": "A", "b1": "B", "c1": "C"},
     LONG, 1000, 1250, None),
    ("more_speakers_than_recorded", [("a1", 10.1, 10.9), ("b1", 11.0, 13.0)], {"a1": "A", "b1": "B"}, LONG, 1000, 1250, 4),
    ("unsorted_speaker_ids", [("u1", 10.1, 10.9), ("u2", 11.0, 12.0), ("u3", 9.0, 10.05)], {"u1": "spk9", "u2": "spk10", "u3": "spk2"},
     LONG, 1000, 1250, None),
    ("file_ends_inside_odd", [("a1", 1.5, 2.0), ("b1", 0.5, 3.5), ("b2", 2.2, 2.4), ("c1", 2.45, 3.0)],
     {"a1": "A", "b1": "B", "b2": "B", "c1": "C"}, 250 * SHIFT + 13, 100, 400, None),
    ("file_ends_inside_even", [("a1", 1.5, 2.0), ("b1", 0.5, 3.5), ("b2", 2.2, 2.4), ("c1", 2.45, 3.0)],
     {"a1": "A", "b1": "B", "b2": "B", "c1": "C"}, 250 * SHIFT, 100, 400, None),
    ("starts_at_file_end", [("a1", 1.5, 2.0), ("b1", 2.6, 3.0)], {"a1": "A", "b1": "B"}, 250 * SHIFT, 250, 500, None),
]


def load_reference_feature(ref_root):
    for name in ("librosa", "soundfile"):
        sys.modules.setdefault(name, types.ModuleType(name))
    path = os.path.join(ref_root, "LS-EEND", "datasets", "feature.py")
    spec = importlib.util.spec_from_file_location("reference_feature", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    def stft_rows(data, frame_size, frame_shift):          # rows only: 1 + n // hop, the last dropped for a multiple of the hop
        n = 1 + len(data) // frame_shift
        return np.zeros((n - 1 if len(data) % frame_shift == 0 else n, 1), dtype=np.complex64)

    mod.stft = stft_rows
    return mod


class FakeKaldi:
    def __init__(self, segments, utt2spk, file_len):
        self.segments = {"rec": [{"utt": u, "st": st, "et": et} for u, st, et in segments]}
        self.utt2spk = dict(utt2spk)
        self.file_len = file_len

    def load_wav(self, rec, start=0, end=None):
        a = min(start, self.file_len)
        b = self.file_len if end is None else min(end, self.file_len)
        return np.zeros(max(b - a, 0), dtype=np.float32), RATE


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = load_reference_feature(sys.argv[1])
    out = []
    for name, segments, utt2spk, file_len, start, end, n_speakers in CASES:
        _, T = ref.get_labeledSTFT(FakeKaldi(segments, utt2spk, file_len), "rec", start, end, SIZE, SHIFT, n_speakers)
        out.append({"name": name, "segments": [list(s) for s in segments], "utt2spk": utt2spk, "file_len": file_len, "start": start,
                    "end": end, "n_speakers": n_speakers, "shape": list(T.shape),
                    "labels": ["".join(str(int(v)) for v in T[:, s]) for s in range(T.shape[1])]})      # one 0/1 string per speaker
    dst = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "chunk_labels.json")
    with open(dst, "w") as f:
        json.dump({"rate": RATE, "frame_shift": SHIFT, "frame_size": SIZE, "cases": out}, f, indent=1)
        f.write("\n")
    print(f"{len(out)} cases -> {dst}")


if __name__ == "__main__":
    main()
