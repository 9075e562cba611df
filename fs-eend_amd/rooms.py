"""Room impulse responses of shoebox rooms generated on the device by the image method (csrc/room.hip `eend_room_rir_f32`).

`simulate.simulate` convolves every speaker with a room impulse response from a resident pool.  The recipe behind the shipped
configs takes those responses from a corpus of simulated shoebox rooms; here they are drawn and generated where they are used, so
a fresh set of rooms costs a kernel launch and nothing has to be loaded:

    rows, groups = draw_rooms(seed, n_rooms=256, n_sources=4)          # host: rooms, one receiver and 4 sources each
    rirs = room_responses(rows, taps=4000, normalize="direct")         # device: a finalized "f32" SourcePool
    recipes = draw_recipes(seed, spk2utt, utts, rirs=rirs, noises=noises, n_mixtures=64, rir_groups=groups)
    corpus, stats = simulate(utts, rirs, noises, recipes)

A row is a dict {"name", "size" (Lx, Ly, Lz) m, "source", "receiver" (x, y, z) m, "beta" (one reflection coefficient, or six:
x0, x1, y0, y1, z0, z1), "c" m/s (343 when absent)}.  The arithmetic contract (images, interpolator, value and bits) is written
down at eend_room_rir_f32 in include/eend_hip.h and in DESIGN 10e; tests/room_ref.py restates it in float64.  `plan_rooms` does
everything the host decides, with every refusal, in numpy and without a device; the tables travel in one pinned block with one
asynchronous copy and the device runs one launch.

Out of scope: frequency-dependent walls, directivity, a high-pass, rates other than 8 kHz, rooms that are not shoeboxes,
equality with any external generator.
"""
import ctypes
import math

import numpy as np
import torch

from . import lib as _lib
from .simulate import MAX_TAPS, RATE, SourcePool

ROOM_WORDS = 20                     # csrc/kernels.h ROOM_WORDS: 17 doubles, K, the output offset, the row's tiles
MIN_SIZE, MIN_DISTANCE = 1.0, 0.01  # metres: the smallest room dimension and source-receiver distance a row may have
_limits = None


def limits():
    """eend_room_limits: dict(tile, window, max_rows, max_axis).  The layout constants live in csrc/kernels.h only."""
    global _limits
    if _limits is None:
        v = [ctypes.c_int() for _ in range(4)]
        _lib.check(_lib.load().eend_room_limits(*[ctypes.byref(x) for x in v]), "eend_room_limits")
        _limits = dict(zip(("tile", "window", "max_rows", "max_axis"), (x.value for x in v)))
    return _limits


def eyring_beta(L, rt60, c=343.0):
    """One reflection coefficient for all six walls of the room L = (Lx, Ly, Lz) from Eyring's formula for a target rt60 in
    seconds: alpha = 1 - exp(-24 ln 10 V / (c S rt60)), beta = sqrt(1 - alpha).  This sets coefficients; it promises no decay
    time.  The image model decays slower than the diffuse-field formula assumes: a 6 x 5 x 3 m room aimed at 0.3 s measures a
    Schroeder T30 near 0.48 s."""
    Lx, Ly, Lz = (float(v) for v in L)
    V, S = Lx * Ly * Lz, 2.0 * (Lx * Ly + Ly * Lz + Lx * Lz)
    alpha = 1.0 - math.exp(-24.0 * math.log(10.0) * V / (float(c) * S * float(rt60)))
    return math.sqrt(1.0 - alpha)


def draw_rooms(seed, n_rooms, n_sources, size=((3.0, 10.0), (3.0, 10.0), (2.5, 4.0)), rt60=(0.2, 0.8), c=343.0, min_distance=0.5,
               margin=0.3, prefix="room"):
    """Random shoebox rooms (host only, deterministic in the seed).  Per room, in this order: the three dimensions (uniform over
    the ranges of `size`), an rt60 (uniform over `rt60`; the walls get eyring_beta of it), one receiver, then `n_sources`
    source positions, every coordinate uniform between `margin` and the dimension less `margin`; a source closer than
    `min_distance` to the receiver is drawn again.  Every draw comes from numpy.random.Generator(PCG64(seed)).
    -> (rows, groups): rows as plan_rooms takes them, named "{prefix}_{room:05d}_{source:02d}", each with its "room"
    "{prefix}_{room:05d}" and "rt60"; groups {room: [its responses' names]} as simulate.draw_recipes(rir_groups=) takes it."""
    rng = np.random.Generator(np.random.PCG64(seed))
    if min(lo for lo, _ in size) <= 2.0 * margin or margin < 0:
        raise ValueError(f"margin {margin} leaves no space in a room of {min(lo for lo, _ in size)} m")
    rows, groups = [], {}
    for i in range(n_rooms):
        L = np.array([rng.uniform(lo, hi) for lo, hi in size])
        t60 = float(rng.uniform(*rt60))
        beta = eyring_beta(L, t60, c)
        rcv = rng.uniform(margin, L - margin)
        room = f"{prefix}_{i:05d}"
        groups[room] = []
        for j in range(n_sources):
            for _ in range(1000):
                src = rng.uniform(margin, L - margin)
                if np.linalg.norm(src - rcv) >= min_distance:
                    break
            else:
                raise ValueError(f"no source position {min_distance} m from the receiver fits a room of {L.tolist()} m")
            name = f"{room}_{j:02d}"
            rows.append({"name": name, "room": room, "size": tuple(L.tolist()), "source": tuple(src.tolist()),
                         "receiver": tuple(rcv.tolist()), "beta": beta, "c": float(c), "rt60": t60})
            groups[room].append(name)
    return rows, groups


def _tile_table(taps, work, tile):
    """Rows (row, first tap) covering taps[i] taps of every row in tiles of `tile`, the tiles with the most images first
    (`work`[i] scales row i's image count per squared tap: late tiles of small rooms lead, so the launch does not end on them)."""
    nt = -(-taps // tile)
    idx = np.repeat(np.arange(len(taps), dtype=np.int64), nt)
    first = (np.arange(int(nt.sum()), dtype=np.int64) - np.repeat(np.cumsum(nt) - nt, nt)) * tile
    order = np.argsort(-((first + tile).astype(np.float64) ** 2 * work[idx]), kind="stable")
    return np.stack([idx[order], first[order]], axis=1)


def plan_rooms(rows, taps, normalize=None):
    """Everything `room_responses` decides on the host, with every refusal (numpy only, no device touched).  rows: dicts as in
    the module docstring; taps: K for all rows or one K per row; normalize: None for g = 1 / (4 pi), "direct" for g = |s - r|
    (the direct path gets amplitude 1, which keeps 16-bit mixtures out of the noise floor), or explicit g, one number or one
    per row.  -> dict(rooms (R, 20), tiles (n, 2) int64 arrays as eend_room_rir_f32 takes them, names, taps (R,), offsets (R,),
    total, table {name: (first sample, K)})."""
    lim = limits()
    T, W = lim["tile"], lim["window"]
    rows = list(rows)
    R = len(rows)
    if R > lim["max_rows"]:
        raise ValueError(f"a call takes at most {lim['max_rows']} rows, got {R}")
    K = np.asarray(taps, dtype=np.int64).reshape(-1)
    if K.size == 1:
        K = np.repeat(K, R)
    if K.size != R:
        raise ValueError(f"taps names {K.size} rows, the call has {R}")
    explicit = None
    if normalize is not None and not isinstance(normalize, str):
        explicit = np.asarray(normalize, dtype=np.float64).reshape(-1)
        explicit = np.repeat(explicit, R) if explicit.size == 1 else explicit
        if explicit.size != R or not np.isfinite(explicit).all():
            raise ValueError(f"normalize names {explicit.size} finite scales, the call has {R} rows")
    elif normalize not in (None, "direct"):
        raise ValueError(f"normalize must be None, 'direct' or a scale, got {normalize!r}")
    names = [row["name"] for row in rows]
    if len(set(names)) != R:
        seen = set()
        twice = next(n for n in names if n in seen or seen.add(n))
        raise ValueError(f"response {twice!r} is named twice")

    def refuse(bad, why):
        """Raise for the first row that `bad` marks."""
        if bad.any():
            i = int(np.argmax(bad))
            raise ValueError(f"{names[i]}: {why(i)}")

    try:                                                            # the rows as arrays: (R, 3) lengths, (R, 6) walls, (R,) speeds
        L, s, r = (np.array([row[key] for row in rows], dtype=np.float64).reshape(R, 3) for key in ("size", "source", "receiver"))
        beta = np.array([(b,) * 6 if np.ndim(b) == 0 else tuple(b) for b in (row["beta"] for row in rows)], dtype=np.float64).reshape(R, 6)
        c = np.array([row.get("c", 343.0) for row in rows], dtype=np.float64).reshape(R)
    except ValueError as e:
        raise ValueError("size, source and receiver have three values, beta one or six, c one") from e
    finite = np.isfinite(L).all(1) & np.isfinite(s).all(1) & np.isfinite(r).all(1) & np.isfinite(beta).all(1) & np.isfinite(c)
    refuse(~finite, lambda i: "every value must be finite")
    refuse((L < MIN_SIZE).any(1), lambda i: f"a room dimension below {MIN_SIZE} m: {L[i].tolist()}")
    refuse(~((s > 0) & (s < L)).all(1), lambda i: f"the source {s[i].tolist()} is not strictly inside the room {L[i].tolist()}")
    refuse(~((r > 0) & (r < L)).all(1), lambda i: f"the receiver {r[i].tolist()} is not strictly inside the room {L[i].tolist()}")
    refuse(((beta < 0) | (beta > 1)).any(1), lambda i: f"a reflection coefficient outside [0, 1]: {beta[i].tolist()}")
    refuse(c <= 0, lambda i: f"the speed of sound must be positive, got {c[i]}")
    refuse((K < 1) | (K > MAX_TAPS), lambda i: f"{K[i]} taps, 1 .. {MAX_TAPS} are supported")
    p = s - r                                                       # the direct image's offset and distance, as the contract forms them
    d0 = np.sqrt(p[:, 0] * p[:, 0] + (p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2]))
    refuse(d0 < MIN_DISTANCE, lambda i: f"source and receiver are {d0[i]} m apart, less than 1 cm")
    q = RATE / np.where(c > 0, c, 1.0)
    deep = 2 * (2 * (np.floor((K - 1 + W // 2) / q / (2.0 * L.min(1) if R else 1.0)).astype(np.int64) + 1) + 1)
    refuse(deep > lim["max_axis"], lambda i: f"{K[i]} taps at c = {c[i]} in a room of {L[i].tolist()} m need {deep[i]} image-table entries "
                                             f"on an axis, at most {lim['max_axis']} are supported")
    g = explicit if explicit is not None else d0 if normalize == "direct" else np.full(R, 1.0 / (4.0 * np.pi))
    words = np.zeros((R, ROOM_WORDS), dtype=np.int64)
    words[:, :17] = np.concatenate([L, s, r, beta, q[:, None], g[:, None]], axis=1).view(np.int64)
    work = 1.0 / (q * q * L.prod(1))
    nt = -(-K // T) if R else K
    offsets = np.cumsum(K) - K
    words[:, 17], words[:, 18], words[:, 19] = K, offsets, nt
    tiles = _tile_table(K, work, T) if R else np.zeros((0, 2), dtype=np.int64)
    return {"rooms": words, "tiles": tiles, "names": names, "taps": K.copy(), "offsets": offsets, "total": int(K.sum()),
            "table": {n: (int(o), int(k)) for n, o, k in zip(names, offsets, K)}}


@torch.no_grad()
def room_responses(rows, taps, device=None, normalize=None):
    """The responses of `rows` (plan_rooms' arguments) generated on `device`.  -> a finalized "f32" SourcePool, as
    simulate.simulate takes it as `rirs`, whose waves are the responses by name, ragged when `taps` is.  One pinned descriptor
    block, one asynchronous copy, one launch; the samples never visit the host and the call does not wait for the device."""
    dev = torch.device(device) if device is not None else torch.device("cuda")
    if dev.type != "cuda":
        raise _lib.EendHipError("room_responses runs on the GPU (no CPU fallback)")
    p = plan_rooms(rows, taps, normalize)
    R, n_tiles = len(p["names"]), len(p["tiles"])
    with torch.cuda.device(dev):
        out = torch.empty(max(p["total"], 1), dtype=torch.float32, device=dev)
        if R:
            parts = (p["rooms"], p["tiles"])
            n_words = sum(a.size for a in parts)
            stage = torch.empty(n_words, dtype=torch.int64, pin_memory=True)      # a fresh pinned block per call (copied asynchronously)
            words = stage.numpy()
            words[:p["rooms"].size] = p["rooms"].reshape(-1)
            words[p["rooms"].size:] = p["tiles"].reshape(-1)
            dbuf = torch.empty(n_words, dtype=torch.int64, device=dev)
            dbuf.copy_(stage, non_blocking=True)
            base = dbuf.data_ptr()
            _lib.check(_lib.load().eend_room_rir_f32(base, R, base + 8 * p["rooms"].size, n_tiles, out.data_ptr(),
                                                     torch.cuda.current_stream(dev).cuda_stream), "eend_room_rir_f32")
    return SourcePool.from_device(out, p["table"], storage="f32")
