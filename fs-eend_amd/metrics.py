"""Diarization error rate as the papers report it, scored on the device (csrc/der_collar.hip; no CPU fallback).

    collar_der / CollarDER     LS-EEND/metrics.py:41-108: pyannote.metrics DiarizationErrorRate(collar=50) over the label runs
                               and the thresholded, median-filtered predictions (the FS-EEND copy does the same)

A forgiveness collar around every reference boundary, hypothesis speakers mapped one-to-one onto reference speakers so that
their overlap is maximal, then miss / false alarm / confusion over speaker time.  `postproc.calc_diarization_error` is the
training-time frame counter (no collar, column i against column i) and stays what it was.

The contract, in reference frames (include/eend_hip.h eend_collar_der_u64 states it in full): `ref` (Tr, Cr) and `hyp` (Th, Ch)
are 0 / 1 activity, hypothesis frame k covers the reference frames [k * subsampling, (k + 1) * subsampling), T = max(Tr, Th *
subsampling) and a side is zero beyond its own end.  `collar` is pyannote's: the total width centred on a boundary, an even
number of frames.  Frame t is removed iff a reference speaker changes state at some b with t - collar/2 < b <= t + collar/2
(zeros outside [0, Tr), so a speaker active in the first or last frame has a boundary there); `skip_overlap` also removes the
frames with two or more reference speakers.  Over the kept frames the co-occurrence counts give the optimal mapping, and
total / missed detection / false alarm / confusion / correct follow.  All counters are exact integers and do not depend on how
ties between equally good mappings are broken.

One quirk of the reference's script is not reproduced: `reference[Segment(s, e)] = str(spkid)` lets a second speaker with an
identical run (s, e) overwrite the first; here both speakers count.
"""
import torch

from . import lib as _lib
from . import postproc as _post

CMAX = 16                                         # speakers per side (DER_CMAX of csrc/kernels.h)
MAX_FRAMES = 2 ** 31 - 2 ** 16                    # longest recording and longest batch, in rows
MAX_COLLAR = 4096                                 # twice DER_HMAX, the half collar eend_collar_der_limits reports
COUNTERS = ("total", "missed detection", "false alarm", "confusion", "correct", "frames kept", "frames removed", "min sum")
_U8, _I32, _I64 = torch.uint8, torch.int32, torch.int64


def limits():
    """(reference frames per tile of the kernel, largest half collar it takes)"""
    import ctypes
    tile, hmax = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().eend_collar_der_limits(ctypes.byref(tile), ctypes.byref(hmax)), "eend_collar_der_limits")
    return tile.value, hmax.value


def _check_numbers(collar, subsampling):
    if isinstance(collar, bool) or not isinstance(collar, int) or collar < 0 or collar % 2:
        raise ValueError(f"collar: expected an even, non-negative number of frames (pyannote's total width), got {collar!r}")
    if collar > MAX_COLLAR:
        raise ValueError(f"collar: at most {MAX_COLLAR} frames, got {collar}")
    if isinstance(subsampling, bool) or not isinstance(subsampling, int) or subsampling < 1:
        raise ValueError(f"subsampling: expected an integer >= 1, got {subsampling!r}")


def _check_args(refs, hyps, collar, subsampling):
    """Everything that can be refused from shapes and numbers alone: ValueError before anything touches the GPU."""
    _check_numbers(collar, subsampling)
    if len(refs) != len(hyps):
        raise ValueError(f"{len(refs)} references for {len(hyps)} hypotheses")
    if not refs:
        raise ValueError("no recording to score")
    if len(refs) > 65535:
        raise ValueError("more than 65535 recordings in one batch")
    rows = [0, 0]
    for side, (name, ts) in enumerate((("ref", refs), ("hyp", hyps))):
        for b, t in enumerate(ts):
            if t.dim() != 2:
                raise ValueError(f"{name}[{b}]: expected (frames, speakers), got shape {tuple(t.shape)}")
            if t.shape[1] > CMAX:
                raise ValueError(f"{name}[{b}]: {t.shape[1]} speakers, at most {CMAX} are scored")
            if t.shape[0] * (int(subsampling) if side else 1) > MAX_FRAMES:
                raise ValueError(f"{name}[{b}]: frame indices beyond 2^31 are out of scope")
            rows[side] += t.shape[0]
    if max(rows) > MAX_FRAMES:
        raise ValueError("row offsets beyond 2^31 are out of scope")


def _as_list(x):
    if isinstance(x, (list, tuple)):
        return [t if isinstance(t, torch.Tensor) else torch.as_tensor(t) for t in x]
    return [x if isinstance(x, torch.Tensor) else torch.as_tensor(x)]


def _pack_side(ts, device):
    """Tensors (T_b, C_b) of any dtype -> (uint8 (max(sum T_b, 1), C) of 0 / 1 with C = max(C_b, 1), int32 (B + 1,) offsets), on
    the device.  Narrower recordings get silent speakers, which change no counter."""
    C = max(1, max(t.shape[1] for t in ts))
    lens = [t.shape[0] for t in ts]
    off = [0]
    for n in lens:
        off.append(off[-1] + n)
    parts = [(t.to(device) != 0).to(_U8) for t in ts]
    if all(p.shape[1] == C for p in parts) and off[-1] > 0:
        rows = torch.cat(parts, 0).contiguous()
    else:
        rows = torch.zeros(max(off[-1], 1), C, dtype=_U8, device=device)
        for p, o in zip(parts, off):
            if p.numel():
                rows[o:o + p.shape[0], :p.shape[1]] = p
    return rows, torch.tensor(off, dtype=_I32).to(device)


def pack(refs, hyps, subsampling=10):
    """Lists of (Tr, Cr) and (Th, Ch) activity tensors (any dtype, non-zero = active; CPU tensors are moved to the GPU) -> the
    ragged batch `collar_der_packed` reads: (ref rows, ref offsets, hyp rows, hyp offsets)."""
    refs, hyps = _as_list(refs), _as_list(hyps)
    _check_args(refs, hyps, 0, subsampling)
    refs = [_post._to_device(t, "ref") for t in refs]
    hyps = [_post._to_device(t, "hyp") for t in hyps]
    dev = refs[0].device
    return _pack_side(refs, dev) + _pack_side(hyps, dev)


def collar_der_packed(batch, collar=50, subsampling=10, skip_overlap=False, out=None):
    """Score a packed batch (see `pack`): three launches on the current stream, no host sync, so the call can be
    captured in a graph.  `out` = (counters int64 (B, 8), cooc int64 (B, 16, 16), mapping int32 (B, 16)) to write into."""
    _check_numbers(collar, subsampling)
    ref, roff, hyp, hoff = batch
    for t, dt, name in ((ref, _U8, "ref rows"), (hyp, _U8, "hyp rows"), (roff, _I32, "ref offsets"), (hoff, _I32, "hyp offsets")):
        if not t.is_cuda or t.dtype != dt or not t.is_contiguous():
            raise _lib.EendHipError(f"{name}: expected a contiguous {dt} GPU tensor")
    B = roff.numel() - 1
    if B < 1 or hoff.numel() != B + 1 or ref.dim() != 2 or hyp.dim() != 2 or not ref.numel() or not hyp.numel():
        raise _lib.EendHipError("collar_der_packed: not a batch made by pack()")
    if out is None:
        out = (torch.empty(B, 8, dtype=_I64, device=ref.device), torch.empty(B, CMAX, CMAX, dtype=_I64, device=ref.device),
               torch.empty(B, CMAX, dtype=_I32, device=ref.device))
    counters, cooc, mapping = out
    if (counters.shape != (B, 8) or cooc.shape != (B, CMAX, CMAX) or mapping.shape != (B, CMAX) or counters.dtype != _I64
            or cooc.dtype != _I64 or mapping.dtype != _I32 or not all(t.is_cuda and t.is_contiguous() for t in out)):
        raise _lib.EendHipError("collar_der_packed: out = (int64 (B, 8), int64 (B, 16, 16), int32 (B, 16)) on the GPU")
    _lib.check(_lib.load().eend_collar_der_u64(ref.data_ptr(), roff.data_ptr(), ref.shape[1], hyp.data_ptr(), hoff.data_ptr(),
                                               hyp.shape[1], B, int(subsampling), int(collar) // 2, int(bool(skip_overlap)),
                                               counters.data_ptr(), cooc.data_ptr(), mapping.data_ptr(), _post._stream()),
               "eend_collar_der_u64")
    return out


def collar_der_counters(refs, hyps, collar=50, subsampling=10, skip_overlap=False):
    """Lists of activity tensors, or a single pair -> (counters int64 (B, 8), cooc int64 (B, 16, 16), mapping int32 (B, 16)),
    all still on the device, no host sync.  counters[b] = total, missed detection, false alarm, confusion, correct, frames kept,
    frames removed within [0, T), sum of min(nr, nh); cooc[b][i][j] = kept frames with reference i and hypothesis j both active;
    mapping[b][j] = the reference speaker of hypothesis j, -1 = unmapped."""
    refs, hyps = _as_list(refs), _as_list(hyps)
    _check_args(refs, hyps, collar, subsampling)
    return collar_der_packed(pack(refs, hyps, subsampling), collar, subsampling, skip_overlap)


def rate(total, errors):
    """errors / total; with nothing to score, 0.0 if nothing went wrong and 1.0 otherwise."""
    return errors / total if total else (0.0 if errors == 0 else 1.0)


def _detail(c, mapping):
    total, miss, fa, conf, correct, kept, removed = c[:7]
    return {"total": total, "correct": correct, "confusion": conf, "false alarm": fa, "missed detection": miss,
            "diarization error rate": rate(total, miss + fa + conf),
            "mapping": {j: i for j, i in enumerate(mapping) if i >= 0}, "frames kept": kept, "frames removed": removed}


def _details(refs, hyps, collar, subsampling, skip_overlap):
    counters, _, mapping = collar_der_counters(refs, hyps, collar, subsampling, skip_overlap)
    return [_detail(c, m) for c, m in zip(counters.cpu().tolist(), mapping.cpu().tolist())]


def collar_der(ref, hyp, collar=50, subsampling=10, skip_overlap=False):
    """One recording -> pyannote's detailed components ('total', 'correct', 'confusion', 'false alarm', 'missed detection',
    'diarization error rate'), plus 'mapping' {hyp: ref}, 'frames kept' and 'frames removed'."""
    return _details([ref], [hyp], collar, subsampling, skip_overlap)[0]


def score_predictions(ref, pred, threshold=0.5, median=11, sad=None, collar=50, subsampling=10, skip_overlap=False):
    """(Tr, Cr) labels and (Th, Ch) probabilities -> collar_der of postproc.activity(pred, threshold, median, sad): probabilities
    to DER without leaving the device."""
    _check_args(_as_list(ref), _as_list(pred), collar, subsampling)
    hyp = _post.activity(_post._to_device(pred, "pred"), threshold, median, sad)
    return collar_der(ref, hyp, collar, subsampling, skip_overlap)


class CollarDER:
    """pyannote's metric object in the reference's use: `metric(ref, hyp, detailed=True)` per recording, `abs(metric)` for the
    aggregate rate as gen_ref forms it (sum of errors / sum of total over the recordings scored so far)."""
    KEYS = ("total", "correct", "confusion", "false alarm", "missed detection")

    def __init__(self, collar=50, subsampling=10, skip_overlap=False):
        _check_numbers(collar, subsampling)
        self.collar, self.subsampling, self.skip_overlap = int(collar), int(subsampling), bool(skip_overlap)
        self.reset()

    def reset(self):
        self.sums = {k: 0 for k in self.KEYS}
        self.recordings = 0

    def _add(self, res):
        for k in self.KEYS:
            self.sums[k] += res[k]
        self.recordings += 1
        return res

    def __call__(self, ref, hyp, detailed=False):
        res = self._add(collar_der(ref, hyp, self.collar, self.subsampling, self.skip_overlap))
        return res if detailed else res["diarization error rate"]

    def score_batch(self, refs, hyps):
        """Many recordings in one launch -> their detailed results, in order; all are accumulated."""
        return [self._add(r) for r in _details(refs, hyps, self.collar, self.subsampling, self.skip_overlap)]

    def report(self):
        """The aggregate components, with 'diarization error rate' = abs(self) and the number of recordings."""
        s = dict(self.sums)
        s["diarization error rate"] = abs(self)
        s["recordings"] = self.recordings
        return s

    def __abs__(self):
        s = self.sums
        return rate(s["total"], s["missed detection"] + s["false alarm"] + s["confusion"])
