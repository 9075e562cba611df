"""Plain references and probe inputs for the feature front-end kernels (csrc/feature.hip behind eend_stft_logmel23_f32,
eend_feature_meannorm_f32, eend_splice_subsample_f32, eend_audio_feed_f32 and eend_chunk_batch_f32; no GPU needed, numpy only).

What the STFT tile body reads, from the code (stft_logmel_tile): of the dft table [200][288] it multiplies all 288 columns but keeps the
accumulators of "bins" n = 0..131 only, Re from column n and Im from column 144 + n; the power Re^2 + Im^2 of those 132 bins meets
melT rows 0..131, and of the 32 mel columns 0..22 are stored.  So
    read and used:     dft columns 0..131 and 144..275 (129..131 and 273..275 are zero in the production table), melT rows 0..131
                       (129..131 zero in production), melT columns 0..22;
    read and ignored:  dft columns 132..143 and 276..287, melT columns 23..31 (they pass through the MFMA and are dropped).
`ref_logmel` models exactly that in float64, so a probe may put values anywhere: those in the ignored columns must not show.

Two probe families make the f32 result independent of the summation order (`assert_exact` proves it from the operands: all integers,
every partial sum of every stage below 2^24 in magnitude), so the only device error left is log10f's:
    dense  integer samples |y| <= 4, dft entries in {-1, 0, 1} in every column, 0/1 mel columns with a few ones: every tap of every
           frame contributes to every output;
    pick   dft[k][n] = 1 for one tap k per bin n (imaginary half zero), melT one bin per mel column, samples distinct integers 1..1000
           within any 1000 consecutive positions: output (t, m) is log10(y[first + 80 t + k_m]^2) of exactly one sample, and a wrong
           tap, bin, frame or sample moves it by at least 2 log10(1000 / 999) = 8.69e-4 (PICK_STEP).

The mean normalisations carry their sums in float64 and round once: with `quantised` inputs (multiples of 2^-10, |v| <= 16) every fp64
sum is exact in any order and the device result is bit-defined; the incremental front-end adds its sum strictly in frame order, which
`ref_meannorm` (numpy's sequential cumsum) restates for any input.  `MUTATIONS` are one-step indexing mistakes of `ref_melpower`;
tests/test_feature_edges_ref.py shows on the CPU that each moves an output of the GPU cases far beyond the bar."""
import numpy as np

WIN, HOP, NCOL, IMOFF, KMEL, NMEL, MELP = 200, 80, 288, 144, 132, 23, 32          # csrc/feature.hip
FB, KC, RING, SPL_ROWS = 64, 20, 32, 16
NT2, PER = 1024, 4
SCAN = NT2 * PER                          # rows per pass of the mode-2 scan
LIMIT = 1 << 24
FLOOR = 1e-10
PICK_STEP = 2.0 * np.log10(1000.0 / 999.0)
USED_DFT = np.r_[0:KMEL, IMOFF:IMOFF + KMEL]
IGNORED_DFT = np.r_[KMEL:IMOFF, IMOFF + KMEL:NCOL]
N_FRAMES = (1, 15, 16, 17, 63, 64, 65, 128, 129)
FIRSTS = (-100, 28, 0, -199, -200, -5239, -5240)            # -5239: of 64 frames only the last tap of the last reaches sample 0


def stft_frames(n):
    """log-mel frames of a recording of n samples (the header's rule: 1 + n / 80, minus one when n % 80 == 0)"""
    return 1 + n // HOP - (n % HOP == 0)


def stft_grid(n_frames):
    """(blocks, frames per block, waves of 16 frames in the last block)"""
    nb = -(-n_frames // FB)
    return nb, FB, -(-(n_frames - (nb - 1) * FB) // 16)


# ------------------------------------------------------------------------------------------------ log-mel
MUTATIONS = ("drop_tap_19", "drop_tap_20", "drop_tap_99", "drop_tap_100", "drop_tap_199", "frame_64_one_hop_late", "im_pairing_off_by_one",
             "mel_row_132", "len_inclusive", "first_minus_99")


def ref_melpower(y, length, first, n_frames, dft, melT, mutation=None):
    """float64 [n_frames][23] mel power by the header's contract.  y: 1-D array whose element i is sample i (values at or beyond
    `length` are never used, whatever they are).  `mutation`: one of MUTATIONS, a one-step mistake of the tile body."""
    y, dft, melT = np.asarray(y, np.float64), np.asarray(dft, np.float64), np.asarray(melT, np.float64)
    assert dft.shape == (WIN, NCOL) and melT.shape == (KMEL, MELP)
    if mutation == "first_minus_99":
        first += 1
    t = np.arange(n_frames)[:, None]
    idx = first + HOP * t + np.arange(WIN)[None, :]
    if mutation == "frame_64_one_hop_late":
        idx = idx + HOP * (t >= FB)
    inside = (idx >= 0) & ((idx <= length) if mutation == "len_inclusive" else (idx < length))
    assert not inside.any() or idx[inside].max() < len(y), "the mutation needs the sample behind len"
    X = np.where(inside, y[np.clip(idx, 0, len(y) - 1)], 0.0)
    if mutation and mutation.startswith("drop_tap_"):
        X[:, int(mutation[9:])] = 0.0
    nb = KMEL + 1 if mutation == "mel_row_132" else KMEL
    im0 = IMOFF + (mutation == "im_pairing_off_by_one")
    re, im = X @ dft[:, :nb], X @ dft[:, im0:im0 + nb]
    P = re * re + im * im
    M = melT[:, :NMEL]
    if mutation == "mel_row_132":                     # whatever lies behind the table: taken as a row of ones
        M = np.vstack([M, np.ones((1, NMEL))])
    return P @ M


def ref_logmel(y, length, first, n_frames, dft, melT, mutation=None):
    """float64 [n_frames][23]: log10(max(mel power, 1e-10))"""
    return np.log10(np.maximum(ref_melpower(y, length, first, n_frames, dft, melT, mutation), FLOOR))


def header_tables():
    """(dft [200][288], melT [132][32]) float64 as include/eend_hip.h words them: periodic Hann of 200 taps, row k = w[k] cos(2 pi (k + 28)
    n / 256) in column n <= 128 and -w[k] sin(..) in column 144 + n; melT = the Slaney filterbank (float32 values) transposed."""
    from oracle import feature_ref as R
    k = np.arange(WIN, dtype=np.float64)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * k / WIN)
    ang = 2.0 * np.pi * np.outer(k + 28, np.arange(129)) / 256.0
    dft = np.zeros((WIN, NCOL))
    dft[:, :129] = w[:, None] * np.cos(ang)
    dft[:, IMOFF:IMOFF + 129] = -w[:, None] * np.sin(ang)
    melT = np.zeros((KMEL, MELP))
    melT[:129, :NMEL] = R.mel_filterbank(8000, 256, NMEL).astype(np.float64).T
    return dft, melT


def speechlike(n, seed, floor=0.01):
    """float32 waveform: three tones under a slow envelope plus white noise of rms `floor` (keeps every mel power far from zero)"""
    g = np.random.default_rng(seed)
    t = np.arange(n) / 8000.0
    env = 0.5 * (1 + np.sin(2 * np.pi * 0.7 * t + 1.0))
    y = env * (0.3 * np.sin(2 * np.pi * 180 * t) + 0.2 * np.sin(2 * np.pi * 1230 * t + 0.3) + 0.1 * np.sin(2 * np.pi * 3100 * t))
    return (y + floor * g.standard_normal(n)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ probes
def _ignored_fill(dft, melT, g):
    """non-zero values where the kernel must not look"""
    dft[:, IGNORED_DFT] = g.integers(1, 4, (WIN, len(IGNORED_DFT)))
    melT[:, NMEL:] = g.integers(1, 4, (KMEL, MELP - NMEL))


def dense_tables(seed=0, ones=6):
    """dft in {-1, 0, 1} (about half non-zero, every tap and every used column hit), melT 0/1 with `ones` bins per mel column, bins
    128..131 among them"""
    g = np.random.default_rng(1000 + seed)
    dft = g.integers(-1, 2, (WIN, NCOL)).astype(np.float64) * g.integers(0, 2, (WIN, NCOL))
    dft[np.arange(WIN), USED_DFT[np.arange(WIN) % len(USED_DFT)]] = 1.0          # no tap without a used column
    dft[g.integers(0, WIN, len(USED_DFT)), USED_DFT] = -1.0                       # no used column without a tap
    melT = np.zeros((KMEL, MELP))
    for m in range(NMEL):
        melT[g.choice(KMEL, ones, replace=False), m] = 1.0
    melT[[128, 129, 130, 131], [0, 7, 15, 22]] = 1.0
    _ignored_fill(dft, melT, g)
    return dft, melT


def dense_samples(n, seed=0):
    """integers in -4..4, zero excluded: a lost sample always shows"""
    g = np.random.default_rng(2000 + seed)
    return (g.integers(1, 5, n) * (2 * g.integers(0, 2, n) - 1)).astype(np.float64)


# taps at the ends of the 20-tap table slices and of the 4-tap MFMA steps, bins at the ends of the 16-column tiles and beyond 128
PICK_TAPS = ((0, 19, 20, 39, 40, 99, 100, 119, 120, 179, 180, 199, 3, 4, 59, 60, 79, 80, 139, 140, 159, 160, 198),
             (1, 2, 5, 18, 21, 23, 24, 41, 61, 81, 98, 101, 102, 103, 121, 141, 161, 181, 195, 196, 197, 16, 17))
PICK_BINS = ((0, 1, 15, 16, 17, 31, 32, 47, 48, 63, 64, 79, 80, 95, 96, 111, 112, 127, 128, 129, 130, 131, 5),
             (2, 14, 18, 30, 33, 46, 49, 62, 65, 78, 81, 94, 97, 110, 113, 126, 125, 124, 131, 130, 129, 128, 3))


def pick_tables(variant=0):
    """mel column m is bin PICK_BINS[variant][m], whose one tap is PICK_TAPS[variant][m]; every other bin has a tap of its own too"""
    g = np.random.default_rng(3000 + variant)
    dft, melT = np.zeros((WIN, NCOL)), np.zeros((KMEL, MELP))
    tap_of = g.integers(0, WIN, KMEL)
    tap_of[list(PICK_BINS[variant])] = PICK_TAPS[variant]
    dft[tap_of, np.arange(KMEL)] = 1.0
    melT[list(PICK_BINS[variant]), np.arange(NMEL)] = 1.0
    _ignored_fill(dft, melT, g)
    return dft, melT


def pick_samples(n, seed=0):
    """y[i] = 1 + perm[i % 1000]: any 1000 consecutive samples are distinct integers of 1..1000"""
    perm = np.random.default_rng(4000 + seed).permutation(1000)
    return (1 + perm[np.arange(n) % 1000]).astype(np.float64)


PROBES = ("dense", "pick0", "pick1")


def probe(name, n, seed=0):
    """-> (samples float64 [n] drawn with `seed`, dft, melT); the tables of a family are always the same"""
    if name == "dense":
        return (dense_samples(n, seed),) + dense_tables()
    return (pick_samples(n, seed),) + pick_tables(int(name[4:]))


def assert_exact(y, dft, melT, unit=1.0):
    """The exactness guard, from the operands alone: samples are integer multiples of `unit` (a power of two), table entries integers,
    and the largest magnitude any partial sum can reach -- |Re|, |Im| <= max|y| sum_k |dft[k][c]| for every one of the 288 columns,
    the power of the 132 bins, the mel sum of the 23 stored columns -- is below 2^24 in its unit, so every f32 product and sum of the
    tile body is exact in any order.  Returns the largest bound."""
    y, dft, melT = np.asarray(y, np.float64) / unit, np.asarray(dft, np.float64), np.asarray(melT, np.float64)
    for a in (y[np.isfinite(y)], dft, melT):
        assert np.array_equal(a, np.round(a)), "operand is not an integer"
    amp = np.abs(y[np.isfinite(y)]).max() * np.abs(dft).sum(0)
    power = amp[:KMEL] ** 2 + amp[IMOFF:IMOFF + KMEL] ** 2
    mel = power @ np.abs(melT[:, :NMEL])
    worst = max(amp.max(), power.max(), mel.max())
    assert worst < LIMIT, worst
    return worst


def stft_lengths(first, n_frames):
    """The `len` values of one (first, n_frames) launch: ending exactly at the last frame's last tap and one short of it, inside the
    first tap of the first frame of the last block (and of block 1), 1, and one hop short of the end; only those >= 1."""
    last = first + HOP * (n_frames - 1) + WIN - 1
    blocks = sorted({(n_frames - 1) // FB, min(1, (n_frames - 1) // FB)})
    cand = [last + 1, last, 1, last + 1 - HOP] + [first + HOP * FB * b + 1 for b in blocks]
    return sorted({c for c in cand if c >= 1})


# ------------------------------------------------------------------------------------------------ mean normalisation, splice
def quantised(T, F, seed):
    """float32 [T][F], multiples of 2^-10 with |v| <= 16: every float64 sum of up to 2^38 such values is exact in any order"""
    g = np.random.default_rng(5000 + seed)
    return (g.integers(-(1 << 14), (1 << 14) + 1, (T, F)) / 1024.0).astype(np.float32)


def ref_meannorm(Y, mode, sums=None):
    """float32 [T][F]: mode 1  Y - f32(sum64(Y) / T);  mode 2  Y[t] - f32(cumsum64(Y)[t] / (t + 1)), the cumsum sequential in float64
    (numpy accumulates in order), one rounding to f32, the subtraction in f32"""
    Y = np.asarray(Y, np.float32)
    T = Y.shape[0]
    if mode == 1:
        s = np.cumsum(Y.astype(np.float64), axis=0)[-1]
        return Y - (s / np.float64(T)).astype(np.float32)[None, :]
    assert mode == 2
    c = np.cumsum(Y.astype(np.float64), axis=0)
    return Y - (c / np.arange(1, T + 1, dtype=np.float64)[:, None]).astype(np.float32)


def pairwise_sum(v):
    """float64 column sums of v [T][F] by a binary tree (another order than cumsum's)"""
    v = np.asarray(v, np.float64)
    while v.shape[0] > 1:
        if v.shape[0] % 2:
            v = np.vstack([v, np.zeros((1, v.shape[1]))])
        v = v[0::2] + v[1::2]
    return v[0]


def ref_splice(Y, ctx, sub):
    """[ceil(T / sub)][F (2 ctx + 1)]: row j = frames j sub - ctx .. j sub + ctx of Y side by side, zero outside [0, T); bits kept"""
    Y = np.asarray(Y)
    T, F = Y.shape
    Yp = np.zeros((T + 2 * ctx, F), Y.dtype)
    Yp[ctx:ctx + T] = Y
    rows = range(0, T, sub)
    return np.stack([Yp[f:f + 2 * ctx + 1].reshape(-1) for f in rows]) if T else np.zeros((0, F * (2 * ctx + 1)), Y.dtype)


def splice_grid(T, F, ctx, sub):
    """(output elements, blocks of 256 threads)"""
    n = -(-T // sub) * F * (2 * ctx + 1)
    return n, -(-n // 256)


# ------------------------------------------------------------------------------------------------ the incremental front-end
def ready_frames(n, ended):
    """log-mel frames computable from n samples: frame f needs 80 f + 100 of them; at the end the batch count"""
    if ended:
        return stft_frames(n)
    return (n - 100) // HOP + 1 if n >= 100 else 0


def ready_rows(T, ended, ctx, sub):
    """model frames computable from T log-mel frames: row j needs frame sub j + ctx; at the end ceil(T / sub)"""
    if ended:
        return -(-T // sub)
    return (T - 1 - ctx) // sub + 1 if T > ctx else 0


def ref_stream(y, cuts, ctx, sub, mode, tables, logmel=None):
    """What the feeds of one stream must add up to.  y: its whole waveform; cuts: [(new samples, ended)] per call naming the stream;
    mode 0 / 2; tables (dft, melT).  `logmel`: the f32 log-mel rows to go on from (the batch kernel's, for a bit-for-bit comparison)
    instead of float64 `ref_logmel` rounded to f32.  -> (rows f32 [ceil(n_frames / sub)][23 (2 ctx + 1)], [rows each call returns])"""
    n = len(y)
    T = stft_frames(n)
    if logmel is None:
        logmel = ref_logmel(y, n, -100, T, *tables).astype(np.float32) if T else np.zeros((0, NMEL), np.float32)
    L = np.asarray(logmel, np.float32)
    assert L.shape == (T, NMEL)
    if mode == 2 and T:
        L = ref_meannorm(L, 2)
    counts, recv, done = [], 0, 0
    for m, ended in cuts:
        recv += m
        rows = ready_rows(ready_frames(recv, ended), ended, ctx, sub)
        counts.append(rows - done)
        done = rows
    assert recv == n
    return ref_splice(L, ctx, sub), counts


def stream_schedule(n_calls=330):
    """The calls of the four-slot walk of tests/test_feature_edges.py: [(call, {slot: new samples}, [slots ending], [slots reset before
    it])], and per slot the list of its streams' lengths.  Slot 0 gets one sample per call for 300 calls (its first frame becomes
    computable at 100 samples, its second at 180), then 500, 1, and its end in a call of its own with no samples.  Slot 1 gets 79 / 80 /
    81 in turn, pausing every third call, and ends in the call of its last samples.  Slot 2 gets 100 samples (one frame), then chunks
    that add exactly 64, 65 and 129 log-mel frames (one, two and three STFT tiles), 10 samples that add none, chunks that add 16, 17
    and 33 (one, two and three splice tiles with sub = 1), and ends with its last 37 samples.  Slot 3 holds a stream of 57 samples in
    all that ends without new samples, then after a reset a stream of NaN, then after another reset an ordinary one that leaves 2 ctx
    frames in the ring, the most there can be."""
    calls = []
    big = [100, HOP * 64, HOP * 65, HOP * 129, 10, HOP * 16, HOP * 17, HOP * 33, 37]
    s1 = [79, 80, 81] * 4
    k1 = k2 = 0
    for c in range(n_calls):
        feed, end, reset = {}, [], []
        if c < 300:
            feed[0] = 1
        elif c == 300:
            feed[0] = 500
        elif c == 301:
            feed[0] = 1
        elif c == 303:
            end.append(0)
        if c % 3 != 2 and k1 < len(s1):
            feed[1] = s1[k1]
            k1 += 1
            if k1 == len(s1):
                end.append(1)
        if c % 11 == 4 and k2 < len(big):
            feed[2] = big[k2]
            k2 += 1
            if k2 == len(big):
                end.append(2)
        if c == 5:
            feed[3] = 40
        elif c == 8:
            feed[3] = 17
        elif c == 9:
            end.append(3)
        elif c == 20:
            reset.append(3)
            feed[3] = 700
        elif c == 23:
            feed[3] = 0
            end.append(3)
        elif c == 40:
            reset.append(3)
            feed[3] = 333
        elif c in (41, 60):
            feed[3] = 1001
        elif c == 61:
            feed[3] = 1465                    # 3800 samples, 47 frames: 47 = 15 mod 16 = 7 mod 10, the fullest ring of (15, 16) and (7, 10)
        elif c == 62:
            feed[3] = 95
            end.append(3)
        if feed or end:
            calls.append((c, feed, end, reset))
    assert k1 == len(s1) and k2 == len(big)
    return calls


STREAM_PAIRS = ((15, 16), (15, 1), (0, 16), (0, 1), (7, 10))

# ------------------------------------------------------------------------------------------------ shapes of the GPU tests
# rows around the wave (64), the block stride (1024) and the scan pass (4096) of colnorm_column, and two passes and one row more
NORM_T = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 8193)
NORM_F = (1, 23, 40)
# (T, F, ctx, sub): 255 / 256 / 257 and 511 / 513 output elements (the 256-thread block edge), sub > T, ctx >= T, the identity, T = 1, and
# the largest context and subsampling of the incremental front-end
SPLICE_CASES = ((5, 17, 1, 1), (16, 16, 0, 1), (257, 1, 0, 1), (7, 73, 0, 1), (17, 19, 1, 2), (5, 23, 2, 7), (3, 23, 7, 1), (37, 5, 0, 1),
                (1, 23, 7, 10), (100, 23, 15, 16), (1000, 23, 15, 16), (33, 23, 15, 1))

# the corpus of the chunk-batch test: recording A of 4300 frames and 37 samples, B of 70 and C of 66 frames exactly; chunks (recording,
# start, end) in frames.  A: offset 0 and one frame; 63, 64, 65 frames; 4097 frames (a second scan pass of the column normalisation); one
# clipped at the end of A to 197 samples (len % 80 != 0, 3 frames).  B: one clipped at its end to 800 samples (len % 80 == 0, 10 frames).
# C: one ending exactly at the end of the corpus.  Between the chunks lie samples of no chunk: the poison.
CHUNK_LENS = {"A": 4300 * HOP + 37, "B": 70 * HOP, "C": 66 * HOP}
CHUNK_ROWS = (("A", 0, 1), ("A", 2, 65), ("A", 66, 130), ("A", 131, 196), ("A", 200, 4297), ("A", 4298, 4400), ("B", 60, 100), ("C", 1, 66))
CHUNK_FRAMES = (1, 63, 64, 65, 4097, 3, 10, 65)


def chunk_segments(S):
    """{recording: ([(utt, start seconds, end seconds)], {utt: speaker})} with S speakers in A (named so that they sort by index) and
    min(S, 3) in B and in C.  Around chunk (A, 66, 130): a segment starting exactly at its start, one ending exactly at its end, one ending
    exactly at its start and one starting exactly at its end (both outside it), one covering it whole (skipped), one wholly outside
    every chunk, two overlapping ones of one speaker, and segments of speaker S - 1."""
    spk = lambda s: "s%02d" % s
    a = [("u0", 66, 80, 0), ("u1", 100, 130, S - 1), ("u2", 50, 66, 0), ("u3", 130, 140, S - 1), ("u4", 0, 5000, min(1, S - 1)),
         ("u5", 5000, 6000, 0), ("u6", 70, 90, min(1, S - 1)), ("u7", 85, 120, min(1, S - 1)), ("u8", 300, 4100, S - 1),
         ("u9", 150, 250, min(2, S - 1))]
    a += [("f%02d" % s, 210 + 60 * s, 243 + 60 * s, s) for s in range(S)]
    b = [("b0", 5, 30, 0), ("b1", 62, 66, min(S, 3) - 1), ("b2", 0, 100, min(1, min(S, 3) - 1))] + [("g%d" % s, 20 * s + 3, 20 * s + 27, s) for s in range(min(S, 3))]
    out = {}
    for rec, rows in (("A", a), ("B", b), ("C", b)):
        out[rec] = ([(u, st / 100.0, et / 100.0) for u, st, et, _ in rows], {u: spk(s) for u, _, _, s in rows})
    return out


def chunk_cover():
    """bool per corpus sample: inside some chunk of CHUNK_ROWS"""
    at, cover = 0, np.zeros(sum(CHUNK_LENS.values()), bool)
    for rec, n in CHUNK_LENS.items():
        for r, st, ed in CHUNK_ROWS:
            if r == rec:
                cover[at + min(st * HOP, n):at + min(ed * HOP, n)] = True
        at += n
    return cover
