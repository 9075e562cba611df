"""The incremental audio front-end (audio_stream.py) measured three ways, printing one JSON line:

  front-end : AudioFrontEnd.feed for S slots x 800-sample (100 ms) chunks from the host, one model frame per slot per call,
              both transforms: device-event time and host time per call over --calls timed calls after --warmup.
  session   : AudioStreamSession at S = 64 (FS bench config with C = 6, LS bench config with C = 10) against the same session
              fed precomputed feature rows: ms per 100 ms of audio for all slots, and the front-end's share.
  hour      : one hour of audio fed to one slot in one call (end of stream included) against feature.extract_fbank_wave.

    python tools/audio_stream_bench.py [--slots 1,8,64] [--calls 200] [--warmup 20] [--steps 100] [--skip-session]

Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this tool (e.g. --skip-session)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS_CFG = dict(n_units=256, n_heads=4, enc_n_layers=4, dec_n_layers=2, dropout=0.1, has_mask=True,
              max_seqlen=500, dec_dim_feedforward=2048, mask_delay=0)          # = bench.py FS_CFG
LS_CFG = dict(n_units=256, n_heads=4, enc_n_layers=4, dec_n_layers=2, dropout=0.1, max_seqlen=1000,
              recurrent_chunk_size=500, feed_forward_expansion_factor=4, dec_dim_feedforward=2048,
              conv_expansion_factor=2, conv_kernel_size=16, half_step_residual=True, conv_delay=9)   # = bench.py LS_CFG
CHUNK = 800


def timed(fn, n, torch):
    """(ms per call from events around n calls -- wall time of the stream, host-side gaps included; host ms per call to enqueue)"""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    host = (time.perf_counter() - t0) / n * 1e3
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n, host


def front_end(args, torch, dev):
    from fs_eend_amd.audio_stream import AudioFrontEnd
    out = []
    n = args.warmup + args.calls
    g = torch.Generator().manual_seed(0)
    for S in [int(s) for s in args.slots.split(",")]:
        y = torch.randn(S, n * CHUNK + 100, generator=g) * 0.1
        for tr in ("logmel23", "logmel23_cummn"):
            fe = AudioFrontEnd(S, tr, device=dev)
            for s in range(S):
                fe.reset(s)
            fe.feed({s: y[s, :100] for s in range(S)})                   # start mid-frame: 100-sample offset, as live audio
            feed = lambda i: fe.feed({s: y[s, 100 + i * CHUNK:100 + (i + 1) * CHUNK] for s in range(S)})
            for i in range(args.warmup):
                feed(i)
            dev_ms, host_ms = timed(lambda i: feed(args.warmup + i), args.calls, torch)
            out.append(dict(slots=S, transform=tr, chunk=CHUNK, calls=args.calls, device_event_ms_per_feed=dev_ms,
                            host_ms_per_feed=host_ms))
            print(json.dumps(out[-1]), file=sys.stderr, flush=True)
    return out


def session(args, torch, dev):
    from fs_eend_amd.audio_stream import AudioStreamSession
    from fs_eend_amd.fs_model import OnlineTransformerDADiarization
    from fs_eend_amd.fs_multistream import FsMultiStreamSession
    from fs_eend_amd.fs_stream import StreamingTransformerEDADiarization, copy_params_from_masked_to_streaming
    from fs_eend_amd.ls_model import OnlineConformerRetentionDADiarization
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    from fs_eend_amd import feature
    torch.manual_seed(0)
    fm = OnlineTransformerDADiarization(n_speakers=None, in_size=345, **FS_CFG).eval().to(dev)
    sm = StreamingTransformerEDADiarization(in_size=345, **FS_CFG).eval().to(dev)
    copy_params_from_masked_to_streaming(fm, sm)
    lm = OnlineConformerRetentionDADiarization(n_speakers=None, in_size=345, **LS_CFG).eval().to(dev)
    S, K, W = 64, args.steps, args.warmup
    g = torch.Generator().manual_seed(1)
    y = torch.randn(S, (K + W + 20) * CHUNK, generator=g) * 0.1
    out = []
    for name, mk, C, tr in (("FS", lambda: FsMultiStreamSession(sm, S, 6), 6, "logmel23"),
                            ("LS", lambda: LsMultiStreamSession(lm, S, 10), 10, "logmel23_cummn")):
        ases = AudioStreamSession(mk())
        for _ in range(S):
            ases.open()
        ases.push({s: y[s, :100] for s in range(S)})
        push = lambda i: ases.push({s: y[s, 100 + i * CHUNK:100 + (i + 1) * CHUNK] for s in range(S)})
        for i in range(W + 10):                                          # past the splice and look-ahead delays, then warm
            push(i)
        a_dev, a_host = timed(lambda i: push(W + 10 + i), K, torch)
        ses = mk()
        for _ in range(S):
            ses.open()
        x = torch.stack([feature.extract_fbank_wave(y[s, :(K + W) * CHUNK].to(dev), input_transform=tr) for s in range(S)], 1)
        step = lambda i: ses.step(push={s: x[i, s] for s in range(S)})
        for i in range(W + 10):
            step(i)
        f_dev, f_host = timed(lambda i: step((W + 10 + i) % x.shape[0]), K, torch)
        out.append(dict(model=name, slots=S, C=C, transform=tr, steps=K, audio_ms_per_100ms=a_dev, features_ms_per_100ms=f_dev,
                        front_end_share=(a_dev - f_dev) / a_dev, audio_enqueue_ms=a_host, features_enqueue_ms=f_host))
        print(json.dumps(out[-1]), file=sys.stderr, flush=True)
        del ases, ses
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    return out


def hour(args, torch, dev):
    from fs_eend_amd.audio_stream import AudioFrontEnd
    from fs_eend_amd import feature
    n = 8000 * 3600
    y = (torch.randn(n, generator=torch.Generator().manual_seed(2)) * 0.1).to(dev)
    out = []
    for tr in ("logmel23", "logmel23_cummn"):
        fe = AudioFrontEnd(1, tr, device=dev)
        inc, bat = [], []
        for _ in range(3):
            fe.reset(0)
            inc.append(timed(lambda i: fe.feed({0: y}, end=[0]), 1, torch)[0])
            bat.append(timed(lambda i: feature.extract_fbank_wave(y, input_transform=tr), 1, torch)[0])
        inc, bat = min(inc), min(bat)
        out.append(dict(transform=tr, samples=n, one_call_ms=inc, batch_ms=bat, ratio=inc / bat))
        print(json.dumps(out[-1]), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="1,8,64")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--skip-session", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("audio_stream_bench needs a GPU")
    dev = torch.device("cuda:0")
    r = dict(tool="audio_stream_bench", device=torch.cuda.get_device_name(0), front_end=front_end(args, torch, dev))
    if not args.skip_session:
        r["session"] = session(args, torch, dev)
    r["hour"] = hour(args, torch, dev)
    r["timing"] = "events around the timed calls (host gaps included); host clock = enqueue time; hour: best of 3 single calls"
    print(json.dumps(r))


if __name__ == "__main__":
    main()
