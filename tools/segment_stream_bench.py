"""Live RTTM segments (live_rttm.py) measured three ways, printing one JSON line:

  session : per-frame wall time of FsMultiStreamSession (C = 6) and LsMultiStreamSession (C = 10) with and without the
            SegmentSession wrapper at S = 1, 8, 64, all slots pushing every frame; the two are timed alternately on the same
            box, --rounds times, and the median of each is kept.  With --sad a third session, SegmentSession(sad=True)
            with one speech-activity flag per pushed frame (runs of 0 and 1), joins the alternation.
  poll    : SegmentSession.poll at S = 64 with a poll every 100 frames: ms per poll (host wall, the sync included) and per frame.
  hour    : one hour (36 000 rows, 11 tracks) of one stream fed to a tracker in one call, end included, against
            postproc.make_rttm on the same logits (device-event time of each; make_rttm's includes its two host reads).

    python tools/segment_stream_bench.py [--slots 1,8,64] [--steps 200] [--warmup 20] [--rounds 3] [--skip-session] [--sad]

Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this tool."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS_CFG = dict(n_units=256, n_heads=4, enc_n_layers=4, dec_n_layers=2, dropout=0.1, has_mask=True,
              max_seqlen=500, dec_dim_feedforward=2048, mask_delay=0)          # = bench.py FS_CFG
LS_CFG = dict(n_units=256, n_heads=4, enc_n_layers=4, dec_n_layers=2, dropout=0.1, max_seqlen=1000,
              recurrent_chunk_size=500, feed_forward_expansion_factor=4, dec_dim_feedforward=2048,
              conv_expansion_factor=2, conv_kernel_size=16, half_step_residual=True, conv_delay=9)   # = bench.py LS_CFG


def timed(fn, n, torch):
    """ms per call from events around n calls (wall time of the stream, host-side gaps included)"""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def models(torch, dev):
    from fs_eend_amd.fs_model import OnlineTransformerDADiarization
    from fs_eend_amd.fs_stream import StreamingTransformerEDADiarization, copy_params_from_masked_to_streaming
    from fs_eend_amd.ls_model import OnlineConformerRetentionDADiarization
    torch.manual_seed(0)
    fm = OnlineTransformerDADiarization(n_speakers=None, in_size=345, **FS_CFG).eval().to(dev)
    sm = StreamingTransformerEDADiarization(in_size=345, **FS_CFG).eval().to(dev)
    copy_params_from_masked_to_streaming(fm, sm)
    lm = OnlineConformerRetentionDADiarization(n_speakers=None, in_size=345, **LS_CFG).eval().to(dev)
    return sm, lm


def sessions(args, torch, dev, sm, lm):
    from fs_eend_amd.fs_multistream import FsMultiStreamSession
    from fs_eend_amd.live_rttm import SegmentSession
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    out = []
    g = torch.Generator().manual_seed(1)
    for name, mk, C in (("FS", lambda S: FsMultiStreamSession(sm, S, 6), 6), ("LS", lambda S: LsMultiStreamSession(lm, S, 10), 10)):
        for S in [int(s) for s in args.slots.split(",")]:
            x = (torch.randn(S, 345, generator=g) * 2 - 3).to(dev)
            push = {s: x[s] for s in range(S)}
            bare, wrapped = mk(S), SegmentSession(mk(S))
            masked = SegmentSession(mk(S), sad=True) if args.sad else None
            flags = [{s: ((i + 3 * s) // 7) & 1 for s in range(S)} for i in range(14)]    # runs of 7 frames, staggered by slot
            for ses in (bare, wrapped, masked):
                if ses is None:
                    continue
                for _ in range(S):
                    ses.open()
                for i in range(args.warmup + 20):                          # past the look-ahead, graph captured, warm
                    ses.step(push=push, **({"sad": flags[i % 14]} if ses is masked else {}))
            t_bare, t_wrap, t_sad = [], [], []
            for _ in range(args.rounds):
                t_bare.append(timed(lambda i: bare.step(push=push), args.steps, torch))
                t_wrap.append(timed(lambda i: wrapped.step(push=push), args.steps, torch))
                wrapped.poll()
                if masked is not None:
                    t_sad.append(timed(lambda i: masked.step(push=push, sad=flags[i % 14]), args.steps, torch))
                    masked.poll()
            b, w = statistics.median(t_bare), statistics.median(t_wrap)
            out.append(dict(model=name, slots=S, C=C, steps=args.steps, rounds=args.rounds, bare_ms_per_frame=b,
                            segments_ms_per_frame=w, added=(w - b) / b, bare_all=t_bare, segments_all=t_wrap))
            if masked is not None:
                m = statistics.median(t_sad)
                out[-1].update(sad_ms_per_frame=m, sad_added=(m - b) / b, sad_over_segments=(m - w) / w, sad_all=t_sad)
            print(json.dumps(out[-1]), file=sys.stderr, flush=True)
            if S == 64 and name == "FS":
                out.append(poll_cost(args, torch, wrapped, push))
                print(json.dumps(out[-1]), file=sys.stderr, flush=True)
            del bare, wrapped, masked
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
    return out


def poll_cost(args, torch, ses, push):
    ses.poll()
    polls, t_poll = 0, 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(1, 501):
        ses.step(push=push)
        if i % 100 == 0:
            torch.cuda.synchronize()
            a = time.perf_counter()
            ses.poll()
            t_poll += time.perf_counter() - a
            polls += 1
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    return dict(what="poll", slots=ses.S, every=100, polls=polls, ms_per_poll=t_poll / polls * 1e3,
                ms_per_frame_amortised=t_poll / 500 * 1e3, frames_ms_total=total * 1e3, ring_bytes=ses.tracker.box.numel() * 4)


def hour(args, torch, dev):
    from fs_eend_amd import postproc
    from fs_eend_amd.live_rttm import SegmentTracker
    T, C = 36000, 12
    g = torch.Generator().manual_seed(2)
    x = torch.randn(T + 40, C, generator=g)
    L = ((torch.nn.functional.avg_pool1d(x.t().unsqueeze(0), 41, 1).squeeze(0).t() * 8) + 0.8 * torch.randn(T, C, generator=g)).to(dev)
    P = torch.sigmoid(L[:, 1:]).contiguous()
    tr = SegmentTracker(1, C - 1, device=dev, capacity=8192)
    inc, bat, full = [], [], []
    for _ in range(5):
        tr.reset(0)
        inc.append(timed(lambda i: tr.feed({0: L}, end=[0]), 1, torch))
        t0 = time.perf_counter()
        lines = tr.rttm(0, "r")
        full.append(inc[-1] + (time.perf_counter() - t0) * 1e3)
        bat.append(timed(lambda i: postproc.make_rttm("r", P), 1, torch))
    assert lines == postproc.make_rttm("r", P)
    n = sum(len(v) for v in lines.values())
    return dict(what="hour", rows=T, tracks=C - 1, segments=n, one_call_ms=min(inc), with_poll_and_lines_ms=min(full),
                make_rttm_ms=min(bat), ratio=min(inc) / min(bat))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="1,8,64")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-session", action="store_true")
    ap.add_argument("--sad", action="store_true", help="also time SegmentSession(sad=True) with a flag per pushed frame")
    ap.add_argument("--skip-hour", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("segment_stream_bench needs a GPU")
    dev = torch.device("cuda:0")
    r = dict(tool="segment_stream_bench", device=torch.cuda.get_device_name(0))
    if not args.skip_session:
        sm, lm = models(torch, dev)
        r["session"] = sessions(args, torch, dev, sm, lm)
    if not args.skip_hour:
        r["hour"] = hour(args, torch, dev)
        print(json.dumps(r["hour"]), file=sys.stderr, flush=True)
    r["timing"] = "events around the timed calls (host gaps included); session: median of alternating rounds; hour: best of 5"
    print(json.dumps(r))


if __name__ == "__main__":
    main()
