"""Host-side mirror of the reference's output post-processing, running on the HIP kernels of
csrc/postproc.hip (no CPU fallback: tensors must live on the GPU).

    make_rttm                  FS-EEND/train/utils/make_rttm.py:10-28 (LS-EEND copy identical)
    calc_diarization_error     FS-EEND/train/utils/loss.py:198-236   (LS-EEND train/utils/loss.py:215-257)
    report_diarization_error   FS-EEND/train/utils/loss.py:239-254
    sad_func                   LS-EEND/sad_post_process.py:23-33     (external speech-activity mask; also `sad=` of
                               activity / make_rttm, which the reference applies before its median filter)

Same names, arguments and return structure as the reference, so `dia_pred.py` / `streaming_infer_dia.py` /
the Lightning validation step can import them from the drop-in `train.utils` shims.
"""
from collections import defaultdict

import torch

from . import lib as _lib

_U8, _I32, _F32 = torch.uint8, torch.int32, torch.float32


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _gpu_f32(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.EendHipError(f"{name}: expected a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype != _F32:
        t = t.to(_F32)
    if t.dim() != 2 or t.stride(1) != 1:
        t = t.contiguous()
    return t


def _to_device(t, name):
    """Drop-in entry points accept what the reference's drivers pass -- CPU tensors (`pred.detach().cpu()`,
    FS streaming_infer_dia.py:95-99, train/oln_tfm_enc_dec.py:262) -- and move them to the current GPU; with no GPU
    there is nothing to run on, and that is an error (no CPU fallback)."""
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t)
    if t.is_cuda:
        return t
    if not torch.cuda.is_available():
        raise _lib.EendHipError(f"{name}: no GPU available (the HIP path has no CPU fallback)")
    return t.to(torch.device("cuda", torch.cuda.current_device()))


def _sad_u8(sad, T, device):
    """A speech-activity mask of shape (T,) or (T, 1), any dtype (non-zero: speech) -> contiguous uint8 (T,) on `device`."""
    if not isinstance(sad, torch.Tensor):
        sad = torch.as_tensor(sad)
    if sad.dim() == 2 and sad.shape[1] == 1:
        sad = sad[:, 0]
    if sad.dim() != 1 or sad.shape[0] != T:
        raise ValueError(f"sad: expected one flag per frame, shape ({T},) or ({T}, 1), got {tuple(sad.shape)}")
    return (sad.to(device) != 0).to(_U8).contiguous()


def sad_fuse(pred, sad, threshold=0.5):
    """(T, S) probabilities and a speech-activity mask -> float32 (T, S) of 0 / 1 (csrc/postproc.hip sad_fuse_kernel): the
    decisions pred > threshold where the mask says speech, none elsewhere, and in a speech frame with no decision the speaker
    with the largest probability (the lowest index on ties).  NaN is never active and never the largest."""
    L = _lib.load()
    pred = _gpu_f32(pred, "pred")
    T, S = pred.shape
    flags = _sad_u8(sad, T, pred.device)
    out = torch.empty(T, S, dtype=_F32, device=pred.device)
    if T and S:
        _lib.check(L.eend_sad_fuse_f32(pred.data_ptr(), pred.stride(0), T, S, float(threshold), flags.data_ptr(), out.data_ptr(),
                                       _stream()), "eend_sad_fuse_f32")
    return out


def sad_func(decision, sad, posterior, threshold=0.5):
    """Drop-in for LS-EEND/sad_post_process.py sad_func(decision, sad, posterior): float32 (T, C) on the posterior's device (a
    CPU posterior is moved to the GPU, and so is the result).  `decision` is accepted for signature compatibility only: it is
    recomputed on the device as posterior > threshold, which is what the reference's caller passes (:69)."""
    posterior = _to_device(posterior, "posterior")
    if decision is not None and tuple(decision.shape) != tuple(posterior.shape):
        raise ValueError(f"decision {tuple(decision.shape)} and posterior {tuple(posterior.shape)} differ in shape")
    return sad_fuse(posterior, sad, threshold)


def activity(pred, threshold=0.5, median=11, sad=None):
    """(T, S) probabilities -> uint8 (T, S): threshold, then median filter along time (make_rttm.py:12-15).  With `sad` ((T,)
    or (T, 1), non-zero: speech) the thresholded decisions are fused with that mask first (sad_fuse), as the reference does."""
    L = _lib.load()
    pred = _gpu_f32(pred, "pred")
    T, S = pred.shape
    if sad is not None:
        pred, threshold = sad_fuse(pred, sad, threshold), 0.5
    out = torch.empty(T, S, dtype=_U8, device=pred.device)
    _lib.check(L.eend_activity_median_u8(pred.data_ptr(), pred.stride(0), T, S, float(threshold), int(median) if median > 1 else 1,
                                         out.data_ptr(), _stream()), "eend_activity_median_u8")
    return out


def segments(act):
    """uint8 (T, S) -> list over speakers of [(start_frame, end_frame), ...] (make_rttm.py:18-21)."""
    L = _lib.load()
    T, S = act.shape
    cap = T + 2                                   # a track of T frames has at most T + 1 change points
    changes = torch.empty(S, cap, dtype=_I32, device=act.device)
    counts = torch.empty(S, dtype=_I32, device=act.device)
    _lib.check(L.eend_activity_segments_i32(act.data_ptr(), T, S, changes.data_ptr(), counts.data_ptr(), cap, _stream()),
               "eend_activity_segments_i32")
    n = counts.cpu().tolist()
    ch = changes[:, : max(n) if n else 0].cpu().tolist() if n and max(n) > 0 else [[] for _ in range(S)]
    return [list(zip(ch[s][0:n[s]:2], ch[s][1:n[s]:2])) for s in range(S)]


RTTM_FMT = "SPEAKER {:s} 1 {:7.2f} {:7.2f} <NA> <NA> {:s} <NA>"


def rttm_lines(rec, segs, frame_shift=80, subsampling=10, sampling_rate=8000):
    """segs: per speaker track, [(start_frame, end_frame), ...] in frame order -> make_rttm's dict {str(spkid): [line, ...]}
    (speakers without segments are absent).  Shared by make_rttm and the live tracker (live_rttm.py)."""
    rttm = defaultdict(list)
    for spkid, ss in enumerate(segs):
        if not ss:
            continue
        # the reference formats 0-dim torch tensors computed as int64 * int / int -> float32; the same
        # arithmetic on the whole vector of change points gives the same float32 values
        se = torch.tensor(ss, dtype=torch.int64)
        st = (se[:, 0] * frame_shift * subsampling / sampling_rate).tolist()
        du = ((se[:, 1] - se[:, 0]) * frame_shift * subsampling / sampling_rate).tolist()
        name = rec + "_" + str(spkid)
        rttm[str(spkid)] = [RTTM_FMT.format(rec, a, b, name) for a, b in zip(st, du)]
    return rttm


def make_rttm(rec, pred, frame_shift=80, threshold=0.5, median=11, subsampling=10, sampling_rate=8000, sad=None):
    pred = _to_device(pred, "pred")
    return rttm_lines(rec, segments(activity(pred, threshold, median, sad)), frame_shift, subsampling, sampling_rate)


def der_counters(pred, label, label_delay=0):
    """Device-side counters (uint64 tensor of 8, still on the GPU; no host sync)."""
    L = _lib.load()
    pred, label = _gpu_f32(pred, "pred"), _gpu_f32(label, "label")
    if pred.shape != label.shape:
        raise _lib.EendHipError("calc_diarization_error: pred and label shapes differ")
    T, C = pred.shape
    out = torch.empty(8, dtype=torch.int64, device=pred.device)
    _lib.check(L.eend_der_counters_u64(pred.data_ptr(), pred.stride(0), label.data_ptr(), label.stride(0), T, C, int(label_delay),
                                       out.data_ptr(), _stream()), "eend_der_counters_u64")
    return out


def calc_diarization_error(pred, label, label_delay=0):
    pred, label = _to_device(pred, "pred"), _to_device(label, "label")
    T, C = pred.shape
    v = der_counters(pred, label, label_delay).cpu().tolist()
    res = {}
    (res["speech_scored"], res["speech_miss"], res["speech_falarm"], res["speaker_scored"], res["speaker_miss"],
     res["speaker_falarm"], res["speaker_error"]) = v[:7]
    # the reference divides two tensors: int64 / python int -> float32
    res["correct"] = float(torch.tensor(v[7]) / C)
    res["diarization_error"] = res["speaker_miss"] + res["speaker_falarm"] + res["speaker_error"]
    res["frames"] = T - label_delay
    if res["speaker_error"] < 0:
        raise Exception("spk error")
    return res


def report_diarization_error(ys, labels, label_delay=0):
    stats_batch = defaultdict(list)
    for y, t in zip(ys, labels):
        for k, v in calc_diarization_error(y, t, label_delay).items():
            stats_batch[k].append(float(v))
    return stats_batch
