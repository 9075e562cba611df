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

Real corpora (AMI, DIHARD II / III) are scored inside the regions of a UEM file, also by the Jaccard error rate, and against
references that come as RTTM text:

    uem=                       on every scoring call: per recording None (all of [0, T)), a list of half-open (start, end) pairs
                               in reference frames, or an (n, 2) integer tensor.  A frame is scored iff it lies in an interval,
                               is clear of the collars of the *uncropped* reference and (skip_overlap) has < 2 reference
                               speakers; an interval's edge is not a boundary (include/eend_hip.h eend_collar_der_regions_u64)
    jaccard_error / JaccardER  per-speaker Jaccard error with its own min-cost pairing (eend_jer_assign_f64), over the same
                               kept frames; collar=0 is the usual DIHARD figure
    read_rttm / read_uem / pack_rttm   text -> frame tables on the host -> label rows rasterised on the device

These follow what pyannote's `uemify` and dscore's JER are documented to do, restated in integers in tests/der_region_ref.py
with scipy's linear_sum_assignment as the reference; neither tool is a dependency or was available to compare against, so no
equality with them is claimed.
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
_OUT_TIMES = _OUT + (((CMAX,), _I64), ((CMAX,), _I64))         # ... and ref_time, hyp_time of the entries with regions


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


def _check_out_times(out, lead, name, device):
    """As _check_out for the entries with regions: `out` may be None, the three tensors of _check_out (the two marginal times
    are made here) or all five (counters, cooc, mapping, ref_time int64 (*lead, 16), hyp_time int64 (*lead, 16))."""
    out = tuple(out) if out is not None else ()
    if len(out) not in (0, 3, 5):
        raise _lib.EendHipError(f"{name}: out = (counters, cooc, mapping) or (counters, cooc, mapping, ref_time, hyp_time)")
    first = _check_out(out[:3] if out else None, lead, name, device)
    times = out[3:] or tuple(torch.empty(lead + s, dtype=dt, device=device) for s, dt in _OUT_TIMES[3:])
    for t, (s, dt) in zip(times, _OUT_TIMES[3:]):
        if t.shape != lead + s or t.dtype != dt or not t.is_cuda or not t.is_contiguous():
            raise _lib.EendHipError(f"{name}: ref_time and hyp_time = int64 {lead + s} on the GPU")
    return tuple(first) + tuple(times)


# ---- scoring regions (UEM)

_I32_MAX = 2 ** 31 - 1


def _check_uem_one(u, name):
    """One recording's regions -> None, or the sorted, merged list of (start, end) pairs.  ValueError for a shape that is not
    (n, 2), a value that is not an integer, start < 0 and end <= start."""
    if u is None:
        return None
    if isinstance(u, torch.Tensor):
        if u.is_floating_point() or u.is_complex() or u.dtype == torch.bool:
            raise ValueError(f"{name}: expected integer frames, got {u.dtype}")
        if not (u.dim() == 2 and u.shape[1] == 2) and u.numel():
            raise ValueError(f"{name}: expected (n, 2) intervals, got shape {tuple(u.shape)}")
        u = u.cpu().tolist() if u.numel() else []
    if not isinstance(u, (list, tuple)):
        raise ValueError(f"{name}: expected None, (start, end) pairs or an (n, 2) integer tensor, got {u!r}")
    pairs = []
    for iv in list(u):
        iv = tuple(iv) if isinstance(iv, (list, tuple)) else (iv,)
        if len(iv) != 2:
            raise ValueError(f"{name}: expected (start, end) pairs, got {iv!r}")
        s, e = iv
        for v in (s, e):
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"{name}: expected integer frames, got {v!r}")
        if s < 0 or e <= s:
            raise ValueError(f"{name}: expected 0 <= start < end, got ({s}, {e})")
        pairs.append((s, min(e, _I32_MAX)))
    out = []
    for s, e in sorted(pairs):
        if out and s <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], e))
        elif s < _I32_MAX:
            out.append((s, e))
    return out


def _check_uems(uem, B, single=False):
    """The `uem=` of a call on B recordings -> None (no regions anywhere) or a list of B checked entries.  `single`: the call got
    one pair of tensors, not lists, and `uem` is that recording's."""
    if uem is None:
        return None
    if single:
        uem = [uem]
    if not isinstance(uem, (list, tuple)) or len(uem) != B:
        raise ValueError(f"uem: expected one entry per recording ({B}): None, (start, end) pairs or an (n, 2) integer tensor")
    out = [_check_uem_one(u, f"uem[{b}]") for b, u in enumerate(uem)]
    return None if all(u is None for u in out) else out


def pack_uem(uems, device=None):
    """Checked or raw per-recording regions (a list with None, pair lists or (n, 2) tensors) -> the device table the kernels read:
    (int32 (max(n_total, 1), 2) intervals, recording after recording; int32 (B + 1,) offsets).  None becomes the one interval
    [0, 2^31 - 1), which the kernels clip to [0, T)."""
    uems = [_check_uem_one(u, f"uem[{b}]") for b, u in enumerate(uems)]
    if device is None:
        if not torch.cuda.is_available():
            raise _lib.EendHipError("pack_uem: no GPU available (the HIP path has no CPU fallback)")
        device = torch.device("cuda", torch.cuda.current_device())
    rows, off = [], [0]
    for u in uems:
        rows += [(0, _I32_MAX)] if u is None else u
        off.append(len(rows))
    table = torch.tensor(rows or [(0, 0)], dtype=_I32).reshape(-1, 2)
    return table.to(device), torch.tensor(off, dtype=_I32).to(device)


def _check_uem_table(uem, B, name):
    if uem is None:
        return None, None
    table, off = uem
    for t, what in ((table, "intervals"), (off, "offsets")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != _I32 or not t.is_contiguous():
            raise _lib.EendHipError(f"{name}: uem {what}: expected a contiguous int32 GPU tensor (see pack_uem)")
    if table.dim() != 2 or table.shape[1] != 2 or off.numel() != B + 1:
        raise _lib.EendHipError(f"{name}: uem = (int32 (n, 2) intervals, int32 (B + 1,) offsets) as pack_uem makes them")
    return table, off


def collar_der_regions_packed(batch, uem=None, collar=50, subsampling=10, skip_overlap=False, out=None):
    """`collar_der_packed` through eend_collar_der_regions_u64: `uem` = the device table of `pack_uem` (None: no regions
    anywhere) -> (counters, cooc, mapping, ref_time int64 (B, 16), hyp_time int64 (B, 16)); the two marginal times are the kept
    frames in which a reference speaker, and the kept reference frames under which a hypothesis speaker, is active.  Three
    launches, no host sync, capturable; `out`: the first three or all five tensors to write into."""
    _check_numbers(collar, subsampling)
    ref, roff, hyp, hoff = batch
    B = _check_packed(ref, roff, hyp, hoff, _U8, side="hyp", what="collar_der_regions_packed: not a batch made by pack()")
    table, uoff = _check_uem_table(uem, B, "collar_der_regions_packed")
    out = counters, cooc, mapping, ref_time, hyp_time = _check_out_times(out, (B,), "collar_der_regions_packed", ref.device)
    _lib.check(_lib.load().eend_collar_der_regions_u64(
        ref.data_ptr(), roff.data_ptr(), ref.shape[1], hyp.data_ptr(), hoff.data_ptr(), hyp.shape[1], B, int(subsampling),
        int(collar) // 2, int(bool(skip_overlap)), table.data_ptr() if table is not None else None,
        uoff.data_ptr() if uoff is not None else None, counters.data_ptr(), cooc.data_ptr(), mapping.data_ptr(), ref_time.data_ptr(),
        hyp_time.data_ptr(), _post._stream()), "eend_collar_der_regions_u64")
    return out


def collar_der_packed(batch, collar=50, subsampling=10, skip_overlap=False, out=None, uem=None):
    """Score a packed batch (see `pack`): three launches on the current stream, no host sync, so the call can be
    captured in a graph.  `out` = (counters int64 (B, 8), cooc int64 (B, 16, 16), mapping int32 (B, 16)) to write into.
    `uem`: the device table of `pack_uem`; only the frames inside a recording's intervals are scored."""
    if uem is not None:
        return collar_der_regions_packed(batch, uem, collar, subsampling, skip_overlap, out)[:3]
    _check_numbers(collar, subsampling)
    ref, roff, hyp, hoff = batch
    B = _check_packed(ref, roff, hyp, hoff, _U8, side="hyp", what="collar_der_packed: not a batch made by pack()")
    out = counters, cooc, mapping = _check_out(out, (B,), "collar_der_packed", ref.device)
    _lib.check(_lib.load().eend_collar_der_u64(ref.data_ptr(), roff.data_ptr(), ref.shape[1], hyp.data_ptr(), hoff.data_ptr(),
                                               hyp.shape[1], B, int(subsampling), int(collar) // 2, int(bool(skip_overlap)),
                                               counters.data_ptr(), cooc.data_ptr(), mapping.data_ptr(), _post._stream()),
               "eend_collar_der_u64")
    return out


def collar_der_counters(refs, hyps, collar=50, subsampling=10, skip_overlap=False, uem=None):
    """Lists of activity tensors, or a single pair -> (counters int64 (B, 8), cooc int64 (B, 16, 16), mapping int32 (B, 16)),
    all still on the device, no host sync.  counters[b] = total, missed detection, false alarm, confusion, correct, frames kept,
    frames removed within [0, T), sum of min(nr, nh); cooc[b][i][j] = kept frames with reference i and hypothesis j both active;
    mapping[b][j] = the reference speaker of hypothesis j, -1 = unmapped.  `uem`: per recording None, (start, end) pairs or an
    (n, 2) integer tensor (for a single pair: that recording's), sorted and merged here."""
    single = not isinstance(refs, (list, tuple))
    refs, hyps = _as_list(refs), _as_list(hyps)
    _check_args(refs, hyps, collar, subsampling)
    uems = _check_uems(uem, len(refs), single)
    batch = pack(refs, hyps, subsampling)
    return collar_der_packed(batch, collar, subsampling, skip_overlap, uem=pack_uem(uems, batch[0].device) if uems else None)


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


def _details(refs, hyps, collar, subsampling, skip_overlap, uems=None):
    counters, _, mapping = collar_der_counters(refs, hyps, collar, subsampling, skip_overlap, uems)
    return [_detail(c, m) for c, m in zip(counters.cpu().tolist(), mapping.cpu().tolist())]


def collar_der(ref, hyp, collar=50, subsampling=10, skip_overlap=False, uem=None):
    """One recording -> pyannote's detailed components ('total', 'correct', 'confusion', 'false alarm', 'missed detection',
    'diarization error rate'), plus 'mapping' {hyp: ref}, 'frames kept' and 'frames removed'.  `uem`: the recording's scoring
    regions, (start, end) pairs or an (n, 2) integer tensor in reference frames."""
    return _details([ref], [hyp], collar, subsampling, skip_overlap, None if uem is None else [uem])[0]


def score_predictions(ref, pred, threshold=0.5, median=11, sad=None, collar=50, subsampling=10, skip_overlap=False, uem=None,
                      jaccard=False):
    """(Tr, Cr) labels and (Th, Ch) probabilities -> collar_der of postproc.activity(pred, threshold, median, sad): probabilities
    to DER without leaving the device.  `jaccard`: also 'jaccard error rate' and 'pairing' {ref: hyp} over the same kept frames."""
    _check_args(_as_list(ref), _as_list(pred), collar, subsampling)
    _check_uems(uem, 1, True)
    hyp = _post.activity(_post._to_device(pred, "pred"), threshold, median, sad)
    res = collar_der(ref, hyp, collar, subsampling, skip_overlap, uem)
    if jaccard:
        j = jaccard_error(ref, hyp, uem, collar, subsampling, skip_overlap)
        res["jaccard error rate"], res["pairing"] = j["jaccard error rate"], j["pairing"]
    return res


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

    def __call__(self, ref, hyp, detailed=False, uem=None):
        res = self._add(collar_der(ref, hyp, self.collar, self.subsampling, self.skip_overlap, uem))
        return res if detailed else res["diarization error rate"]

    def score_batch(self, refs, hyps, uems=None):
        """Many recordings in one launch -> their detailed results, in order; all are accumulated."""
        return [self._add(r) for r in _details(refs, hyps, self.collar, self.subsampling, self.skip_overlap, uems)]

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
                            totals=None, uem=None, times=False):
    """Score every point of thresholds x medians on a packed batch (`pack_references`, `pack_predictions`) in one pass: three
    launches on the current stream and no host sync.  Point g = i_threshold * len(medians) + i_median.  `thresholds` / `medians`:
    sequences (checked, rounded to float32 and copied to the device here) or float32 / int32 device tensors (used as they are;
    a median that is not odd in 1 .. 127 marks its points with counters of -1).  `out` = (counters int64 (G, B, 8), cooc int64
    (G, B, 16, 16), mapping int32 (G, B, 16)) to write into; `totals` int64 (G, 8), not cleared: every (g, b)'s counters are added
    to row g.  With `out` and device-tensor grids nothing is allocated or copied, so the call can be captured in a graph.
    `uem`: the device table of `pack_uem`; `times`: return (and take in `out`) ref_time and hyp_time int64 (G, B, 16) as well.
    Either goes through eend_collar_der_sweep_regions_u64."""
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
    regions = uem is not None or times
    table, uoff = _check_uem_table(uem, B, "collar_der_sweep_packed")
    out = (_check_out_times if regions else _check_out)(out, (G, B), "collar_der_sweep_packed", dev)
    counters, cooc, mapping = out[:3]
    if totals is not None and (totals.shape != (G, 8) or totals.dtype != _I64 or not totals.is_cuda or not totals.is_contiguous()):
        raise _lib.EendHipError("collar_der_sweep_packed: totals = int64 (G, 8) on the GPU")
    if regions:
        _lib.check(_lib.load().eend_collar_der_sweep_regions_u64(
            ref.data_ptr(), roff.data_ptr(), ref.shape[1], rows.data_ptr(), poff.data_ptr(), rows.shape[1],
            flags.data_ptr() if flags is not None else None, B, thresholds.data_ptr(), nth, medians.data_ptr(), nmed, int(subsampling),
            int(collar) // 2, int(bool(skip_overlap)), table.data_ptr() if table is not None else None,
            uoff.data_ptr() if uoff is not None else None, counters.data_ptr(), cooc.data_ptr(), mapping.data_ptr(),
            totals.data_ptr() if totals is not None else None, out[3].data_ptr(), out[4].data_ptr(), _post._stream()),
            "eend_collar_der_sweep_regions_u64")
        return out if times else out[:3]
    _lib.check(_lib.load().eend_collar_der_sweep_u64(
        ref.data_ptr(), roff.data_ptr(), ref.shape[1], rows.data_ptr(), poff.data_ptr(), rows.shape[1],
        flags.data_ptr() if flags is not None else None, B, thresholds.data_ptr(), nth, medians.data_ptr(), nmed, int(subsampling),
        int(collar) // 2, int(bool(skip_overlap)), counters.data_ptr(), cooc.data_ptr(), mapping.data_ptr(),
        totals.data_ptr() if totals is not None else None, _post._stream()), "eend_collar_der_sweep_u64")
    return out


def sweep_counters(refs, preds, thresholds, medians, sads=None, collar=50, subsampling=10, skip_overlap=False, totals=None, uem=None,
                   times=False):
    """Lists of (Tr, Cr) labels and (Th, Ch) posteriors, or a single pair -> (counters int64 (G, B, 8), cooc int64 (G, B, 16, 16),
    mapping int32 (G, B, 16)) of the grid, still on the device, no host sync: row g of each is what
    `collar_der_counters(refs, [postproc.activity(p, threshold, median, sad) ...], uem=uem)` returns at point g.  `uem` as for
    `collar_der_counters`; `times`: ref_time and hyp_time int64 (G, B, 16) as well."""
    single = not isinstance(refs, (list, tuple))
    refs, preds = _as_list(refs), _as_list(preds)
    _check_args(refs, preds, collar, subsampling)
    _check_grid(thresholds, medians)
    _check_sads(preds, sads)
    uems = _check_uems(uem, len(refs), single)
    ref_batch = pack_references(refs)
    return collar_der_sweep_packed(ref_batch, pack_predictions(preds, sads), thresholds, medians, collar, subsampling,
                                   skip_overlap, totals=totals, uem=pack_uem(uems, ref_batch[0].device) if uems else None, times=times)


def _grid_values(th, med, thresholds, medians):
    """The grid's values on the host: from the checked lists, or one copy each of a device tensor."""
    return (th if th is not None else thresholds.cpu().tolist()), (med if med is not None else medians.cpu().tolist())


class SweepResult:
    """What a grid gave.  `thresholds` (as rounded to float32) and `medians`; `table[g]`: the aggregate components of point g =
    i_threshold * len(medians) + i_median over the recordings (sums, and 'diarization error rate' = sum of errors / sum of total),
    with its 'threshold' and 'median'; `details[g][b]`: recording b at point g in `collar_der`'s form (None where there are
    only totals); `best` = (threshold, median, rate) of the lowest rate, the lowest g on ties.  `jaccard` (None unless asked
    for): per point the aggregate Jaccard error rate, also in `table[g]['jaccard error rate']`, and `jaccard_details[g][b]` in
    `jaccard_error`'s form."""

    def __init__(self, thresholds, medians, sums, details=None, recordings=0, jaccard_details=None):
        self.thresholds, self.medians, self.details, self.recordings = list(thresholds), list(medians), details, recordings
        self.jaccard_details, self.jaccard = jaccard_details, None
        self.table = [{"threshold": self.thresholds[g // len(self.medians)], "median": self.medians[g % len(self.medians)],
                       **_components(c)} for g, c in enumerate(sums)]
        if jaccard_details is not None:
            self.jaccard = [_jer_aggregate(point) for point in jaccard_details]
            for row, j in zip(self.table, self.jaccard):
                row["jaccard error rate"] = j
        g = min(range(len(self.table)), key=lambda i: (self.table[i]["diarization error rate"], i))
        self.best = (self.table[g]["threshold"], self.table[g]["median"], self.table[g]["diarization error rate"])

    def rates(self):
        """[[rate at (threshold i, median j) for j] for i]"""
        n = len(self.medians)
        return [[self.table[i * n + j]["diarization error rate"] for j in range(n)] for i in range(len(self.thresholds))]


def sweep_predictions(refs, preds, thresholds=(0.3, 0.4, 0.5, 0.6, 0.7), medians=(1, 11), sads=None, collar=50, subsampling=10,
                      skip_overlap=False, uem=None, jaccard=False):
    """Labels and posteriors (lists or one pair) -> SweepResult over the grid: one device pass, one copy to the host.  `uem` as
    for `collar_der_counters`; `jaccard`: the Jaccard error rate of every point as well (one more launch, on G * B matrices)."""
    th, med = _check_grid(thresholds, medians)
    out = sweep_counters(refs, preds, thresholds, medians, sads, collar, subsampling, skip_overlap, uem=uem, times=jaccard)
    counters, cooc, mapping = out[:3]
    parts = [counters, mapping.to(_I64)]
    if jaccard:
        G, B = counters.shape[:2]
        Cr, Ch = _widths(_as_list(refs), _as_list(preds))
        pairing, speakers = jer_assign(cooc.view(G * B, CMAX, CMAX), out[3].view(G * B, CMAX), out[4].view(G * B, CMAX), Cr, Ch)
        parts += [pairing.view(G, B, CMAX).to(_I64), speakers.view(G, B, 3 * CMAX), out[4]]
    both = torch.cat(parts, dim=2).cpu().tolist()                                  # (G, B, 8 + 16 [+ 16 + 48 + 16]): the one copy
    th, med = _grid_values(th, med, thresholds, medians)
    details = [[_detail(row[:8], row[8:24]) for row in point] for point in both]
    sums = [[sum(row[k] for row in point) for k in range(8)] for point in both]
    jd = [[_jer_detail(row[24:40], row[40:88], row[88:104]) for row in point] for point in both] if jaccard else None
    return SweepResult(th, med, sums, details, len(both[0]), jd)


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

    def add(self, refs, preds, sads=None, uem=None):
        """Score a batch and add it to the totals; returns the batch's device tensors (counters, cooc, mapping).  `uem` as for
        `collar_der_counters`."""
        single = not isinstance(refs, (list, tuple))
        refs, preds = _as_list(refs), _as_list(preds)
        _check_args(refs, preds, self.collar, self.subsampling)
        _check_sads(preds, sads)
        uems = _check_uems(uem, len(refs), single)
        ref_batch, pred_batch = pack_references(refs), pack_predictions(preds, sads)
        dev = ref_batch[0].device
        if self.totals is None:
            self.totals = torch.zeros(len(self.thresholds) * len(self.medians), 8, dtype=_I64, device=dev)
            self._grid = (torch.tensor(self.thresholds, dtype=_F32).to(dev), torch.tensor(self.medians, dtype=_I32).to(dev))
        self.recordings += len(refs)
        return collar_der_sweep_packed(ref_batch, pred_batch, self._grid[0], self._grid[1], self.collar, self.subsampling,
                                       self.skip_overlap, totals=self.totals, uem=pack_uem(uems, dev) if uems else None)

    def report(self):
        n = len(self.thresholds) * len(self.medians)
        sums = self.totals.cpu().tolist() if self.totals is not None else [[0] * 8 for _ in range(n)]
        return SweepResult(self.thresholds, self.medians, sums, None, self.recordings)


# ---- Jaccard error rate (csrc/der_collar.hip jer_assign_kernel, eend_jer_assign_f64)

def _widths(refs, hyps):
    return max(1, max(t.shape[1] for t in refs)), max(1, max(t.shape[1] for t in hyps))


def jer_assign(cooc, ref_time, hyp_time, Cr=CMAX, Ch=CMAX, out=None):
    """int64 (n, 16, 16), (n, 16), (n, 16) on the device, as the entries with regions write them -> (pairing int32 (n, 16),
    reference -> hypothesis, -1 = unpaired; speakers int64 (n, 16, 3) = ref_time, paired hyp_time or 0, intersection).  One
    launch, no host sync.  The pairing minimises the sum of 1 - intersection / union; it is not the mapping of the DER."""
    n = cooc.shape[0]
    for t, shape in ((cooc, (n, CMAX, CMAX)), (ref_time, (n, CMAX)), (hyp_time, (n, CMAX))):
        if not t.is_cuda or t.dtype != _I64 or not t.is_contiguous() or tuple(t.shape) != shape or n < 1:
            raise _lib.EendHipError("jer_assign: cooc (n, 16, 16), ref_time (n, 16), hyp_time (n, 16): contiguous int64 on the GPU")
    if out is None:
        out = (torch.empty(n, CMAX, dtype=_I32, device=cooc.device), torch.empty(n, CMAX, 3, dtype=_I64, device=cooc.device))
    pairing, speakers = out
    if (pairing.shape != (n, CMAX) or pairing.dtype != _I32 or speakers.shape != (n, CMAX, 3) or speakers.dtype != _I64
            or not pairing.is_cuda or not speakers.is_cuda or not pairing.is_contiguous() or not speakers.is_contiguous()):
        raise _lib.EendHipError("jer_assign: out = (int32 (n, 16), int64 (n, 16, 3)) on the GPU")
    _lib.check(_lib.load().eend_jer_assign_f64(cooc.data_ptr(), ref_time.data_ptr(), hyp_time.data_ptr(), int(Cr), int(Ch), n,
                                               pairing.data_ptr(), speakers.data_ptr(), _post._stream()), "eend_jer_assign_f64")
    return out


def jaccard_error_counters(refs, hyps=None, uem=None, collar=0, subsampling=10, skip_overlap=False, out=None):
    """Lists of activity tensors or one pair -- or, with hyps=None, a batch made by `pack` with `uem` the device table of
    `pack_uem` -- -> (pairing int32 (B, 16), speakers int64 (B, 16, 3), hyp_time int64 (B, 16)) on the device.  On a packed
    batch nothing is copied or synchronised (four launches), so the call can be captured in a graph; `out` = (the five tensors
    of collar_der_regions_packed, (pairing, speakers)) to write into."""
    if hyps is None:
        batch, table = refs, uem
    else:
        single = not isinstance(refs, (list, tuple))
        refs, hyps = _as_list(refs), _as_list(hyps)
        _check_args(refs, hyps, collar, subsampling)
        uems = _check_uems(uem, len(refs), single)
        batch = pack(refs, hyps, subsampling)
        table = pack_uem(uems, batch[0].device) if uems else None
    der_out, jer_out = out if out is not None else (None, None)
    _, cooc, _, ref_time, hyp_time = collar_der_regions_packed(batch, table, collar, subsampling, skip_overlap, der_out)
    pairing, speakers = jer_assign(cooc, ref_time, hyp_time, batch[0].shape[1], batch[2].shape[1], jer_out)
    return pairing, speakers, hyp_time


def _jer_detail(pairing, speakers, hyp_time):
    """One recording's rows from the device (lists; speakers flat, 3 per speaker) -> the dict of `jaccard_error`."""
    per = {}
    for i in range(CMAX):
        rt, ht, inter = speakers[3 * i:3 * i + 3]
        if rt > 0:
            union = rt + ht - inter
            per[i] = {"ref time": rt, "hyp time": ht, "intersection": inter, "jaccard error rate": (union - inter) / union}
    if per:
        jer = sum(v["jaccard error rate"] for v in per.values()) / len(per)
    else:
        jer = 0.0 if not any(hyp_time) else 1.0
    return {"jaccard error rate": jer, "speakers": per, "pairing": {i: j for i, j in enumerate(pairing) if j >= 0 and i in per},
            "spurious": not per and any(hyp_time)}


def _jer_aggregate(details):
    """Sum of the per-speaker errors over the number of reference speakers; with none, 0.0 unless some hypothesis spoke."""
    n = sum(len(d["speakers"]) for d in details)
    errors = sum(v["jaccard error rate"] for d in details for v in d["speakers"].values())
    return errors / n if n else (1.0 if any(d["spurious"] for d in details) else 0.0)


def _jer_details(refs, hyps, uems, collar, subsampling, skip_overlap):
    pairing, speakers, hyp_time = jaccard_error_counters(_as_list(refs), _as_list(hyps), uems, collar, subsampling, skip_overlap)
    rows = torch.cat([pairing.to(_I64), speakers.view(-1, 3 * CMAX), hyp_time], dim=1).cpu().tolist()
    return [_jer_detail(r[:16], r[16:64], r[64:80]) for r in rows]


def jaccard_error(ref, hyp, uem=None, collar=0, subsampling=10, skip_overlap=False):
    """One recording -> {'jaccard error rate': the mean over the reference speakers with kept time of (union - intersection) /
    union (1.0 for a speaker left unpaired; with no reference speaker 0.0, or 1.0 if a hypothesis speaker has kept time),
    'speakers': {ref: {'ref time', 'hyp time', 'intersection', 'jaccard error rate'}} in kept frames, 'pairing': {ref: hyp},
    'spurious': hypothesis activity without any reference speaker}.  All counts are over the frames `collar_der` keeps with
    the same arguments; collar=0 gives the usual DIHARD figure."""
    return _jer_details([ref], [hyp], None if uem is None else [uem], collar, subsampling, skip_overlap)[0]


class JaccardER:
    """`CollarDER` for the Jaccard error rate: `metric(ref, hyp, detailed=True, uem=...)` per recording, `abs(metric)` = the sum
    of the per-speaker errors over the number of reference speakers of the recordings scored so far."""

    def __init__(self, collar=0, subsampling=10, skip_overlap=False):
        _check_numbers(collar, subsampling)
        self.collar, self.subsampling, self.skip_overlap = int(collar), int(subsampling), bool(skip_overlap)
        self.reset()

    def reset(self):
        self.errors, self.speakers, self.recordings, self.spurious = 0.0, 0, 0, 0

    def _add(self, res):
        self.errors += sum(v["jaccard error rate"] for v in res["speakers"].values())
        self.speakers += len(res["speakers"])
        self.spurious += int(res["spurious"])
        self.recordings += 1
        return res

    def __call__(self, ref, hyp, detailed=False, uem=None):
        res = self._add(jaccard_error(ref, hyp, uem, self.collar, self.subsampling, self.skip_overlap))
        return res if detailed else res["jaccard error rate"]

    def score_batch(self, refs, hyps, uems=None):
        """Many recordings in one launch -> their detailed results, in order; all are accumulated."""
        return [self._add(r) for r in _jer_details(refs, hyps, uems, self.collar, self.subsampling, self.skip_overlap)]

    def report(self):
        return {"jaccard error rate": abs(self), "speakers": self.speakers, "recordings": self.recordings,
                "errors": self.errors}

    def __abs__(self):
        return self.errors / self.speakers if self.speakers else (1.0 if self.spurious else 0.0)


# ---- references as RTTM + UEM text (host parse; csrc/segraster.hip rasterises on the device)

def _lines(source):
    if isinstance(source, (str, bytes)) or hasattr(source, "__fspath__"):
        with open(source, "r") as f:
            return f.read().splitlines()
    return [ln.decode() if isinstance(ln, bytes) else ln for ln in source]


def _frame(t, frame_rate, where):
    """np.rint(t * frame_rate) on float64, the reference's rule (datasets/feature.py get_labeledSTFT): half to even."""
    f = round(t * frame_rate)                                     # Python's round on a float is rint: exact, half to even
    if f > MAX_FRAMES:
        raise ValueError(f"{where}: frame {f} is beyond {MAX_FRAMES}")
    return f


def _number(text, where):
    try:
        v = float(text)
    except ValueError:
        raise ValueError(f"{where}: {text!r} is not a number") from None
    if not math.isfinite(v):
        raise ValueError(f"{where}: {text!r} is not finite")
    return v


def read_rttm(source, frame_rate=100.0):
    """RTTM text (a path, an open file or an iterable of lines) -> {recording: {'speakers': [names in order of first
    appearance], 'segments': [(speaker index, start frame, end frame), ...] in file order}}.  SPEAKER records only, other
    types are skipped.  start -> rint(start * frame_rate), end -> rint((start + duration) * frame_rate): the label matrix the
    reference's datasets make of the same segments.  ValueError naming the line for a malformed line, a negative start or
    duration, a 17th speaker in a recording, and a frame beyond MAX_FRAMES."""
    out = {}
    for no, line in enumerate(_lines(source), 1):
        f = line.split()
        if not f or f[0].startswith(("#", ";")) or (f[0] != "SPEAKER" and f[0].isupper() and len(f) >= 8):
            continue
        where = f"RTTM line {no}"
        if f[0] != "SPEAKER" or len(f) < 8:
            raise ValueError(f"{where}: expected 'SPEAKER file chan start duration <NA> <NA> name ...', got {line!r}")
        start, dur = _number(f[3], where), _number(f[4], where)
        if start < 0 or dur < 0:
            raise ValueError(f"{where}: negative start or duration in {line!r}")
        rec = out.setdefault(f[1], {"speakers": [], "segments": []})
        if f[7] not in rec["speakers"]:
            if len(rec["speakers"]) == CMAX:
                raise ValueError(f"{where}: more than {CMAX} speakers in recording {f[1]!r}")
            rec["speakers"].append(f[7])
        rec["segments"].append((rec["speakers"].index(f[7]), _frame(start, frame_rate, where), _frame(start + dur, frame_rate, where)))
    return out


def read_uem(source, frame_rate=100.0):
    """UEM text ('file chan start end' per line) -> {recording: sorted, merged [(start frame, end frame), ...]}, frames by the
    rule of `read_rttm`; an interval that is empty after rounding is dropped.  ValueError naming the line for a malformed line,
    a negative time, end < start, and a frame beyond MAX_FRAMES."""
    out = {}
    for no, line in enumerate(_lines(source), 1):
        f = line.split()
        if not f or f[0].startswith(("#", ";")):
            continue
        where = f"UEM line {no}"
        if len(f) != 4:
            raise ValueError(f"{where}: expected 'file chan start end', got {line!r}")
        start, end = _number(f[2], where), _number(f[3], where)
        if start < 0 or end < 0:
            raise ValueError(f"{where}: negative time in {line!r}")
        if end < start:
            raise ValueError(f"{where}: end before start in {line!r}")
        s, e = _frame(start, frame_rate, where), _frame(end, frame_rate, where)
        out.setdefault(f[0], [])
        if s < e:
            out[f[0]].append((s, e))
    return {rec: _check_uem_one(ivs, rec) for rec, ivs in out.items()}


def segments_raster(tables, lengths, n_speakers=None, device=None):
    """Per recording a list of (speaker, start, end) and a length in frames -> (uint8 rows, int32 offsets) on the device, equal to
    `pack_references` of the label matrices, which are never built on the host: the segment table is copied and
    eend_segments_raster_u8 writes the rows (zeroed, then one store per segment and frame)."""
    if len(tables) != len(lengths) or not tables:
        raise ValueError(f"{len(tables)} segment tables for {len(lengths)} lengths")
    if len(tables) > 65535:
        raise ValueError("more than 65535 recordings in one batch")
    C = max([1] + [s[0] + 1 for t in tables for s in t]) if n_speakers is None else int(n_speakers)
    off, segs = [0], []
    for b, (t, n) in enumerate(zip(tables, lengths)):
        if isinstance(n, bool) or not isinstance(n, int) or n < 0:
            raise ValueError(f"lengths[{b}]: expected a number of frames >= 0, got {n!r}")
        off.append(off[-1] + n)
        for spk, s, e in t:
            if not 0 <= spk < C or C > CMAX:
                raise ValueError(f"recording {b}: speaker {spk} of {C}, at most {CMAX} are scored")
            if s < 0 or e > n:
                raise ValueError(f"recording {b}: segment ({s}, {e}) outside its {n} frames")
            if s < e:
                segs.append((b, spk, s, e))
    if off[-1] > MAX_FRAMES:
        raise ValueError("row offsets beyond 2^31 are out of scope")
    if device is None:
        if not torch.cuda.is_available():
            raise _lib.EendHipError("segments_raster: no GPU available (the HIP path has no CPU fallback)")
        device = torch.device("cuda", torch.cuda.current_device())
    rows = torch.empty(max(off[-1], 1), C, dtype=_U8, device=device)
    offsets = torch.tensor(off, dtype=_I32).to(device)
    seg = torch.tensor(segs or [(0, 0, 0, 0)], dtype=_I32).reshape(-1, 4).to(device)
    _lib.check(_lib.load().eend_segments_raster_u8(seg.data_ptr(), len(segs), offsets.data_ptr(), len(tables), C, rows.data_ptr(),
                                                   rows.shape[0], _post._stream()), "eend_segments_raster_u8")
    return rows, offsets


def rttm_lengths(recs, rttm, uem=None, lengths=None):
    """A recording's length in frames: the largest of its last segment end, its last UEM end and the caller's length."""
    out = []
    for b, rec in enumerate(recs):
        n = max([0] + [e for _, _, e in rttm.get(rec, {"segments": []})["segments"]])
        if uem is not None and uem.get(rec):
            n = max(n, uem[rec][-1][1])
        if lengths is not None:
            given = lengths[rec] if isinstance(lengths, dict) else lengths[b]
            n = max(n, int(given))
        out.append(n)
    return out


def pack_rttm(recs, rttm, uem=None, lengths=None):
    """Recording ids in batch order, `read_rttm`'s and (optionally) `read_uem`'s dicts, and optional lengths in frames (a list
    in that order, or a dict) -> ((uint8 rows, int32 offsets), the device UEM table or None): the reference half of a batch,
    rasterised on the device, and what `uem=` of the packed calls takes.  A recording absent from `rttm` has no segments; one
    absent from `uem` is scored everywhere."""
    recs = list(recs)
    lens = rttm_lengths(recs, rttm, uem, lengths)
    C = max([1] + [len(rttm[r]["speakers"]) for r in recs if r in rttm])
    ref = segments_raster([rttm.get(r, {"segments": []})["segments"] for r in recs], lens, C)
    table = pack_uem([uem.get(r) for r in recs], ref[0].device) if uem is not None else None
    return ref, table
