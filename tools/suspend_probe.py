"""Suspend / resume of a stream slot: the one-launch block copy (MultiStreamSession.snapshot / resume over ops.copy_blocks) against
the same transfer written as torch slice copies -- the form available without the kernel, and the baseline -- in the same
process, alternating.  Bench configs (bench.py FS_CFG / LS_CFG): an FS session of 2 slots at C = 6 with one slot taken to
t = 36000 by seek (its cache rows keep what they hold; only the byte count matters to a copy), and an LS slot at C = 10.

    python tools/suspend_probe.py [--pos 36000,600] [--reps 5] [--out profiles/suspend_probe.json]

Per case: bytes moved, and for snapshot and resume with the blob on the device and on the host (pinned) the median / min / max
wall time of `reps` synchronised calls and GB/s = bytes / median.  A device-to-device copy reads and writes every byte, so its
share of the HBM copy rate is 2 x bytes / time over 6.3 TB/s.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.fs_multistream_bench import C as C_FS, FS_CFG, HBM_BPS, cap_for  # noqa: E402
from tools.ls_multistream_bench import C as C_LS, LS_CFG  # noqa: E402


def timed(torch, fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def report(ts, nbytes, d2d):
    med = sorted(ts)[len(ts) // 2]
    r = dict(ms=round(med * 1e3, 4), ms_min_max=[round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)], gb_per_s=round(nbytes / med / 1e9, 1))
    if d2d:
        r["share_of_hbm_copy_rate"] = round(2 * nbytes / med / HBM_BPS, 3)
    return r


def slices(ses, s, n_enc, n_dec):
    """The slot's state as torch slices (views): what the torch form copies one by one."""
    C = ses.C
    if ses.kind == "fs":
        out = [t[s:s + 1, :, :n_enc] for kv in ses.enc_kv for t in kv]
        out += [t[s * C:(s + 1) * C, :, :n_dec] for kv in ses.dec_kv for t in kv]
        return out + [ses.win16[s]]
    out = [t[s] for pair in zip(ses.enc_kv, ses.caches) for t in pair]
    return out + [t[s * C:(s + 1) * C] for t in ses.dec_kv] + [ses.win32[s]]


def probe(torch, ses, s, reps):
    """Slot s of ses, open at its position: snapshot and resume both ways, kernel and torch slices alternating."""
    f = ses.table.export(s)
    n_enc, n_dec = f["n_enc"], f["n_dec"]
    views = slices(ses, s, n_enc, n_dec)
    nbytes = sum(v.numel() * v.element_size() for v in views)
    snap = ses.snapshot(s)
    assert snap.nbytes == nbytes, (snap.nbytes, nbytes)            # no padding at these shapes: the blob is the state
    host = snap.to("cpu")
    parts = [v.clone() for v in views]
    pinned = [torch.empty(p.shape, dtype=p.dtype, pin_memory=True).copy_(p) for p in parts]
    free = next(i for i in range(ses.S) if ses.state(i) == "free")
    back = slices(ses, free, n_enc, n_dec)

    def resume(sn):
        ses.close(ses.resume(sn))

    def slices_to_host():
        out = [torch.empty(v.shape, dtype=v.dtype, pin_memory=True) for v in views]
        for o, v in zip(out, views):
            o.copy_(v, non_blocking=True)
        torch.cuda.synchronize()

    forms = {
        "snapshot_device": (lambda: ses.snapshot(s), lambda: [v.clone() for v in views], True),
        "snapshot_host": (lambda: ses.snapshot(s).to("cpu"), slices_to_host, False),
        "resume_device": (lambda: resume(snap), lambda: [b.copy_(p) for b, p in zip(back, parts)], True),
        "resume_host": (lambda: resume(host), lambda: [b.copy_(p, non_blocking=True) for b, p in zip(back, pinned)], False),
    }
    out = dict(kind=ses.kind, slots=ses.S, C=ses.C, t=f["t"], n_enc=n_enc, n_dec=n_dec, bytes=nbytes, pieces=len(views))
    for name, (kernel, torch_form, d2d) in forms.items():
        rounds = {"copy_blocks": [], "torch_slices": []}
        for i in range(reps + 1):                                  # alternating in one process; round 0 warms both forms up
            for form, fn in (("copy_blocks", kernel), ("torch_slices", torch_form)):
                ts = timed(torch, fn, 1, warm=2 if i == 0 else 0)
                if i:
                    rounds[form] += ts
        r = {form: report(ts, nbytes, d2d) for form, ts in rounds.items()}
        k, b = rounds["copy_blocks"], rounds["torch_slices"]
        r["speedup"] = round(sorted(b)[len(b) // 2] / sorted(k)[len(k) // 2], 2)
        r["slower_beyond_baseline_spread"] = min(k) > max(b)
        out[name] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pos", default="36000,600", help="FS stream positions (frames)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("suspend_probe needs a GPU")
    from fs_eend_amd import ops
    from fs_eend_amd.fs_model import OnlineTransformerDADiarization
    from fs_eend_amd.fs_multistream import FsMultiStreamSession
    from fs_eend_amd.fs_stream import StreamingTransformerEDADiarization, copy_params_from_masked_to_streaming
    from fs_eend_amd.ls_model import OnlineConformerRetentionDADiarization
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    out = dict(tool="suspend_probe", device=torch.cuda.get_device_name(0), reps=args.reps, tile_bytes=ops.copy_blocks_tile_bytes(),
               timing="host clock around one synchronised call, kernel and torch forms alternating in one process", results=[])
    fm = OnlineTransformerDADiarization(n_speakers=None, in_size=345, **FS_CFG).eval().to(dev)
    sm = StreamingTransformerEDADiarization(in_size=345, **FS_CFG).eval().to(dev)
    copy_params_from_masked_to_streaming(fm, sm)
    for t in (int(p) for p in args.pos.split(",") if p):
        ses = FsMultiStreamSession(sm, 2, C_FS, cap=cap_for(t), use_graph=False)
        s = ses.open()
        ses.seek(s, t)
        r = probe(torch, ses, s, args.reps)
        out["results"].append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
        ses = None
        torch.cuda.empty_cache()
    m = OnlineConformerRetentionDADiarization(n_speakers=None, in_size=345, **LS_CFG).eval().to(dev)
    ses = LsMultiStreamSession(m, 2, C_LS, use_graph=False)
    s = ses.open()
    g = torch.Generator().manual_seed(1)
    for x in (torch.randn(20, 345, generator=g) * 2 - 3).to(dev):
        ses.step({s: x})
    r = probe(torch, ses, s, args.reps)
    out["results"].append(r)
    print(json.dumps(r), file=sys.stderr, flush=True)
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
