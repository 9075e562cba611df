"""Diarization error rate as the papers report it, scored on the device (csrc/der_collar.hip; no CPU fallback).

    collar_der / CollarDER     LS-EEND/metrics.py:41-108: pyannote.metrics DiarizationErrorRate(collar=50) over the label runs
                               and the thresholded, median-filtered predictions (the FS-EEND copy does the same)
    sweep_predictions / DerSweep   the same at every point of a threshold x median grid, from the posteriors, in one device pass
                               (csrc/der_sweep.hip): what --thredshold and --median of that script are tuned with

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
import ctypes
import math

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


def _pack_rows(ts, dtype, fill, device, convert):
    """Tensors (T_b, C_b) -> (rows (max(sum T_b, 1), C) of `dtype` with C = max(C_b, 1): recording b's rows, `convert`ed, from
    row off[b], `fill` in the columns a narrower recording lacks; int32 (B + 1,) offsets; off as a list), on the device."""
    C = max(1, max(t.shape[1] for t in ts))
    off = [0]
    for t in ts:
        off.append(off[-1] + t.shape[0])
    parts = [convert(t.to(device)) for t in ts]
    if all(p.shape[1] == C for p in parts) and off[-1] > 0:
        rows = torch.cat(parts, 0).contiguous()
    else:
        rows = torch.full((max(off[-1], 1), C), fill, dtype=dtype, device=device)
        for p, o in zip(parts, off):
            if p.numel():
                rows[o:o + p.shape[0], :p.shape[1]] = p
    return rows, torch.tensor(off, dtype=_I32).to(device), off


def _pack_side(ts, device):
    """Tensors (T_b, C_b) of any dtype -> (uint8 rows of 0 / 1, int32 offsets).  Narrower recordings get silent speakers, which
    change no counter."""
    return _pack_rows(ts, _U8, 0, device, lambda t: (t != 0).to(_U8))[:2]


def pack(refs, hyps, subsampling=10):
    """Lists of (Tr, Cr) and (Th, Ch) activity tensors (any dtype, non-zero = active; CPU tensors are moved to the GPU) -> the
    ragged batch `collar_der_packed` reads: (ref rows, ref offsets, hyp rows, hyp offsets)."""
    refs, hyps = _as_list(refs), _as_list(hyps)
    _check_args(refs, hyps, 0, subsampling)
    refs = [_post._to_device(t, "ref") for t in refs]
    hyps = [_post._to_device(t, "hyp") for t in hyps]
    dev = refs[0].device
    return _pack_side(refs, dev) + _pack_side(hyps, dev)


def _check_packed(ref, roff, rows, off, dtype, *, side, what):
    """The reference half and the `side` ("hyp" / "pred", rows of `dtype`) half of a packed batch -> B, or EendHipError: `what`
    if they are not a batch."""
    for t, dt, name in ((ref, _U8, "ref rows"), (rows, dtype, side + " rows"), (roff, _I32, "ref offsets"), (off, _I32, side + " offsets")):
        if not t.is_cuda or t.dtype != dt or not t.is_contiguous():
            raise _lib.EendHipError(f"{name}: expected a contiguous {dt} GPU tensor")
    B = roff.numel() - 1
    if B < 1 or off.numel() != B + 1 or ref.dim() != 2 or rows.dim() != 2 or not ref.numel() or not rows.numel():
        raise _lib.EendHipError(what)
    return B


_OUT = (((8,), _I64), ((CMAX, CMAX), _I64), ((CMAX,), _I32))   # counters, cooc, mapping behind the leading dimensions


def _check_out(out, lead, name, device):
    """`out` = (counters int64 (*lead, 8), cooc int64 (*lead, 16, 16), mapping int32 (*lead, 16)) on the GPU, lead = (B,) or
    (G, B); made here if None."""
    if out is None:
        return tuple(torch.empty(lead + s, dtype=dt, device=device) for s, dt in _OUT)
    counters, cooc, mapping = out
    for t, (s, dt) in zip(out, _OUT):
        if t.shape != lead + s or t.dtype != dt or not t.is_cuda or not t.is_contiguous():
            d = "G, B" if len(lead) == 2 else "B"
            raise _lib.EendHipError(f"{name}: out = (int64 ({d}, 8), int64 ({d}, 16, 16), int32 ({d}, 16)) on the GPU")
    return out


def collar_der_packed(batch, collar=50, subsampling=10, skip_overlap=False, out=None):
    """Score a packed batch (see `pack`): three launches on the current stream, no host sync, so the call can be
    captured in a graph.  `out` = (counters int64 (B, 8), cooc int64 (B, 16, 16), mapping int32 (B, 16)) to write into."""
    _check_numbers(collar, subsampling)
    ref, roff, hyp, hoff = batch
    B = _check_packed(ref, roff, hyp, hoff, _U8, side="hyp", what="collar_der_packed: not a batch made by pack()")
    out = counters, cooc, mapping = _check_out(out, (B,), "collar_der_packed", ref.device)
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


def _components(c):
    """The eight counters of a recording, or their sums -> pyannote's components."""
    total, miss, fa, conf, correct = c[:5]
    return {"total": total, "correct": correct, "confusion": conf, "false alarm": fa, "missed detection": miss,
            "diarization error rate": rate(total, miss + fa + conf)}


def _detail(c, mapping):
    return {**_components(c), "mapping": {j: i for j, i in enumerate(mapping) if i >= 0}, "frames kept": c[5], "frames removed": c[6]}


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


# ---- a threshold x median grid in one device pass (csrc/der_sweep.hip, eend_collar_der_sweep_u64)

MAX_THRESHOLDS, MAX_MEDIANS, MAX_POINTS, MAX_MEDIAN = 16, 4, 32, 127   # DER_SWEEP_* of csrc/kernels.h
_F32 = torch.float32


def sweep_limits():
    """(thresholds, medians and points per call, largest median) of the sweep kernel"""
    v = [ctypes.c_int() for _ in range(4)]
    _lib.check(_lib.load().eend_der_sweep_limits(*(ctypes.byref(x) for x in v)), "eend_der_sweep_limits")
    return tuple(x.value for x in v)


def _check_grid(thresholds, medians):
    """The grid as the kernel will see it -> (thresholds rounded to float32, medians) as lists, or None in place of a list for
    a device tensor, whose values the host does not read (its length is still checked).  ValueError for an empty grid, more
    than 16 thresholds, 4 medians or 32 points, a non-finite threshold, and a median that is not an odd integer in 1 .. 127."""
    out = []
    for name, x, dt in (("thresholds", thresholds, _F32), ("medians", medians, _I32)):
        if isinstance(x, torch.Tensor) and x.is_cuda:
            if x.dim() != 1 or x.dtype != dt or not x.is_contiguous():
                raise ValueError(f"{name}: a device tensor must be contiguous, one-dimensional and {dt}, got {x.dtype} {tuple(x.shape)}")
            out.append((None, x.numel()))
            continue
        if isinstance(x, torch.Tensor):
            x = x.tolist()
        x = list(x) if isinstance(x, (list, tuple)) else [x]
        if name == "medians":
            for k in x:
                if isinstance(k, bool) or not isinstance(k, int) or k < 1 or k > MAX_MEDIAN or k % 2 == 0:
                    raise ValueError(f"medians: expected odd integers in 1 .. {MAX_MEDIAN}, got {k!r}")
        else:
            for v in x:
                if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                    raise ValueError(f"thresholds: expected finite numbers, got {v!r}")
            x = torch.tensor(x, dtype=_F32).tolist() if x else x    # rounded once: the value every comparison uses
            if not all(math.isfinite(v) for v in x):
                raise ValueError("thresholds: beyond the range of float32")
        out.append((x, len(x)))
    (th, nth), (med, nmed) = out
    if nth < 1 or nmed < 1:
        raise ValueError("an empty grid: at least one threshold and one median")
    if nth > MAX_THRESHOLDS or nmed > MAX_MEDIANS or nth * nmed > MAX_POINTS:
        raise ValueError(f"a grid of {nth} x {nmed}: at most {MAX_THRESHOLDS} thresholds, {MAX_MEDIANS} medians and {MAX_POINTS} points")
    return th, med


def _check_sads(preds, sads):
    if sads is None:
        return None
    sads = list(sads) if isinstance(sads, (list, tuple)) else [sads]
    if len(sads) != len(preds) or any(s is None for s in sads):
        raise ValueError(f"sads: a mask for every recording or for none, got {sum(s is not None for s in sads)} for {len(preds)}")
    sads = [s if isinstance(s, torch.Tensor) else torch.as_tensor(s) for s in sads]
    for b, (s, p) in enumerate(zip(sads, preds)):
        if not (s.dim() == 1 or (s.dim() == 2 and s.shape[1] == 1)) or s.shape[0] != p.shape[0]:
            raise ValueError(f"sads[{b}]: expected one flag per frame, shape ({p.shape[0]},) or ({p.shape[0]}, 1), got {tuple(s.shape)}")
    return sads


def pack_references(refs):
    """A list of (Tr, Cr) activity tensors -> (uint8 rows, int32 offsets) on the device, the reference half of `pack`."""
    refs = _as_list(refs)
    _check_args(refs, refs, 0, 1)
    refs = [_post._to_device(t, "ref") for t in refs]
    return _pack_side(refs, refs[0].device)


def pack_predictions(preds, sads=None):
    """A list of (Th, Ch) posteriors (CPU tensors are moved to the GPU) and, for all of them or for none, speech-activity masks
    (Th,) or (Th, 1) (non-zero: speech) -> (float32 rows (max(sum Th, 1), C), int32 offsets (B + 1,), uint8 flags or None) on the
    device.  A recording narrower than the widest gets NaN columns: NaN is never active and never the largest."""
    preds = _as_list(preds)
    _check_args(preds, preds, 0, 1)
    sads = _check_sads(preds, sads)
    preds = [_post._to_device(t, "pred") for t in preds]
    dev = preds[0].device
    rows, offsets, off = _pack_rows(preds, _F32, float("nan"), dev, lambda t: t.to(_F32))
    flags = None
    if sads is not None:
        flags = torch.zeros(max(off[-1], 1), dtype=_U8, device=dev)
        for s, t, o in zip(sads, preds, off):
            if t.shape[0]:
                flags[o:o + t.shape[0]] = _post._sad_u8(s, t.shape[0], dev)
    return rows, offsets, flags


def collar_der_sweep_packed(ref_batch, pred_batch, thresholds, medians, collar=50, subsampling=10, skip_overlap=False, out=None,
                            totals=None):
    """Score every point of thresholds x medians on a packed batch (`pack_references`, `pack_predictions`) in one pass: three
    launches on the current stream and no host sync.  Point g = i_threshold * len(medians) + i_median.  `thresholds` / `medians`:
    sequences (checked, rounded to float32 and copied to the device here) or float32 / int32 device tensors (used as they are;
    a median that is not odd in 1 .. 127 marks its points with counters of -1).  `out` = (counters int64 (G, B, 8), cooc int64
    (G, B, 16, 16), mapping int32 (G, B, 16)) to write into; `totals` int64 (G, 8), not cleared: every (g, b)'s counters are added
    to row g.  With `out` and device-tensor grids nothing is allocated or copied, so the call can be captured in a graph."""
    _check_numbers(collar, subsampling)
    th, med = _check_grid(thresholds, medians)
    ref, roff = ref_batch[:2]
    rows, poff, flags = pred_batch
    B = _check_packed(ref, roff, rows, poff, _F32, side="pred",
                      what="collar_der_sweep_packed: not batches made by pack_references() and pack_predictions()")
    if flags is not None and (not flags.is_cuda or flags.dtype != _U8 or not flags.is_contiguous() or flags.numel() < rows.shape[0]):
        raise _lib.EendHipError("collar_der_sweep_packed: flags = one contiguous uint8 per posterior row on the GPU")
    dev = ref.device
    thresholds = thresholds if th is None else torch.tensor(th, dtype=_F32).to(dev)
    medians = medians if med is None else torch.tensor(med, dtype=_I32).to(dev)
    nth, nmed = thresholds.numel(), medians.numel()
    G = nth * nmed
    out = counters, cooc, mapping = _check_out(out, (G, B), "collar_der_sweep_packed", dev)
    if totals is not None and (totals.shape != (G, 8) or totals.dtype != _I64 or not totals.is_cuda or not totals.is_contiguous()):
        raise _lib.EendHipError("collar_der_sweep_packed: totals = int64 (G, 8) on the GPU")
    _lib.check(_lib.load().eend_collar_der_sweep_u64(
        ref.data_ptr(), roff.data_ptr(), ref.shape[1], rows.data_ptr(), poff.data_ptr(), rows.shape[1],
        flags.data_ptr() if flags is not None else None, B, thresholds.data_ptr(), nth, medians.data_ptr(), nmed, int(subsampling),
        int(collar) // 2, int(bool(skip_overlap)), counters.data_ptr(), cooc.data_ptr(), mapping.data_ptr(),
        totals.data_ptr() if totals is not None else None, _post._stream()), "eend_collar_der_sweep_u64")
    return out


def sweep_counters(refs, preds, thresholds, medians, sads=None, collar=50, subsampling=10, skip_overlap=False, totals=None):
    """Lists of (Tr, Cr) labels and (Th, Ch) posteriors, or a single pair -> (counters int64 (G, B, 8), cooc int64 (G, B, 16, 16),
    mapping int32 (G, B, 16)) of the grid, still on the device, no host sync: row g of each is what
    `collar_der_counters(refs, [postproc.activity(p, threshold, median, sad) ...])` returns at point g."""
    refs, preds = _as_list(refs), _as_list(preds)
    _check_args(refs, preds, collar, subsampling)
    _check_grid(thresholds, medians)
    _check_sads(preds, sads)
    return collar_der_sweep_packed(pack_references(refs), pack_predictions(preds, sads), thresholds, medians, collar, subsampling,
                                   skip_overlap, totals=totals)


def _grid_values(th, med, thresholds, medians):
    """The grid's values on the host: from the checked lists, or one copy each of a device tensor."""
    return (th if th is not None else thresholds.cpu().tolist()), (med if med is not None else medians.cpu().tolist())


class SweepResult:
    """What a grid gave.  `thresholds` (as rounded to float32) and `medians`; `table[g]`: the aggregate components of point g =
    i_threshold * len(medians) + i_median over the recordings (sums, and 'diarization error rate' = sum of errors / sum of total),
    with its 'threshold' and 'median'; `details[g][b]`: recording b at point g in `collar_der`'s form (None where there are
    only totals); `best` = (threshold, median, rate) of the lowest rate, the lowest g on ties."""

    def __init__(self, thresholds, medians, sums, details=None, recordings=0):
        self.thresholds, self.medians, self.details, self.recordings = list(thresholds), list(medians), details, recordings
        self.table = [{"threshold": self.thresholds[g // len(self.medians)], "median": self.medians[g % len(self.medians)],
                       **_components(c)} for g, c in enumerate(sums)]
        g = min(range(len(self.table)), key=lambda i: (self.table[i]["diarization error rate"], i))
        self.best = (self.table[g]["threshold"], self.table[g]["median"], self.table[g]["diarization error rate"])

    def rates(self):
        """[[rate at (threshold i, median j) for j] for i]"""
        n = len(self.medians)
        return [[self.table[i * n + j]["diarization error rate"] for j in range(n)] for i in range(len(self.thresholds))]


def sweep_predictions(refs, preds, thresholds=(0.3, 0.4, 0.5, 0.6, 0.7), medians=(1, 11), sads=None, collar=50, subsampling=10,
                      skip_overlap=False):
    """Labels and posteriors (lists or one pair) -> SweepResult over the grid: one device pass, one copy to the host."""
    th, med = _check_grid(thresholds, medians)
    counters, _, mapping = sweep_counters(refs, preds, thresholds, medians, sads, collar, subsampling, skip_overlap)
    both = torch.cat([counters, mapping.to(_I64)], dim=2).cpu().tolist()           # (G, B, 8 + 16): the one copy
    th, med = _grid_values(th, med, thresholds, medians)
    details = [[_detail(row[:8], row[8:]) for row in point] for point in both]
    sums = [[sum(row[k] for row in point) for k in range(8)] for point in both]
    return SweepResult(th, med, sums, details, len(both[0]))


class DerSweep:
    """`CollarDER` for a grid: `add` scores a batch at every point and accumulates on the device without a host sync, `report`
    makes one copy and returns the SweepResult of everything added so far (no per-recording details)."""

    def __init__(self, thresholds=(0.3, 0.4, 0.5, 0.6, 0.7), medians=(1, 11), collar=50, subsampling=10, skip_overlap=False):
        _check_numbers(collar, subsampling)
        th, med = _check_grid(thresholds, medians)
        if th is None or med is None:
            th, med = _grid_values(th, med, thresholds, medians)
            th, med = _check_grid(th, med)
        self.thresholds, self.medians = th, med
        self.collar, self.subsampling, self.skip_overlap = int(collar), int(subsampling), bool(skip_overlap)
        self.reset()

    def reset(self):
        self.totals = self._grid = None
        self.recordings = 0

    def add(self, refs, preds, sads=None):
        """Score a batch and add it to the totals; returns the batch's device tensors (counters, cooc, mapping)."""
        refs, preds = _as_list(refs), _as_list(preds)
        _check_args(refs, preds, self.collar, self.subsampling)
        _check_sads(preds, sads)
        ref_batch, pred_batch = pack_references(refs), pack_predictions(preds, sads)
        dev = ref_batch[0].device
        if self.totals is None:
            self.totals = torch.zeros(len(self.thresholds) * len(self.medians), 8, dtype=_I64, device=dev)
            self._grid = (torch.tensor(self.thresholds, dtype=_F32).to(dev), torch.tensor(self.medians, dtype=_I32).to(dev))
        self.recordings += len(refs)
        return collar_der_sweep_packed(ref_batch, pred_batch, self._grid[0], self._grid[1], self.collar, self.subsampling,
                                       self.skip_overlap, totals=self.totals)

    def report(self):
        n = len(self.thresholds) * len(self.medians)
        sums = self.totals.cpu().tolist() if self.totals is not None else [[0] * 8 for _ in range(n)]
        return SweepResult(self.thresholds, self.medians, sums, None, self.recordings)
