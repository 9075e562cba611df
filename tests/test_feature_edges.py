"""GPU: the five entries of the feature front-end (csrc/feature.hip: eend_stft_logmel23_f32, eend_feature_meannorm_f32,
eend_splice_subsample_f32, eend_audio_feed_f32, eend_chunk_batch_f32) at their tile, tap, scan and ring edges, against the plain
references of tests/feature_edge_ref.py.

The STFT tile body runs on probe tables for which every f32 sum is exact (E.assert_exact proves it from the operands), so what remains
is log10f's own error, compared with float64 under a bar 500 times below the smallest step of the pick probe: a wrong sample, tap, bin,
mel column or frame fails it (tests/test_feature_edges_ref.py shows that on the CPU).  The mean normalisations are bit for bit on
quantised inputs, the splice always; the incremental and the chunk-batch paths are bit for bit against the single-waveform entries, as
the header promises, and the incremental cumulative mean against the sequential float64 reference.

The direct C-ABI cases pre-fill each output with NaN between two NaN canary rows, keep NaN in the samples before index 0 and from
`len` on and in the rows behind T, and print the grid they exercised.  AudioFrontEnd and DeviceCorpus allocate their own outputs: there
the state rows of slots a call does not name are compared bitwise around every call, and the corpus pool is seeded with NaN buffers whose
tails must stay NaN."""
import functools

import numpy as np
import pytest
import torch

from tests import chunk_label_ref as C
from tests import feature_edge_ref as E

pytestmark = pytest.mark.gpu
F32, F64, I16, I32, I64 = torch.float32, torch.float64, torch.int16, torch.int32, torch.int64
NAN = float("nan")
EINVAL = -1
PRE = 6000                      # NaN samples in front of index 0 (first goes down to -5240)

# Bars of the float64 comparisons: twice the worst error measured on the MI355X (the measured figure stands beside each bar).
# "logmel probe abs": the sums are exact, so this is log10f's error alone; it must stay below E.PICK_STEP / 64 = 1.36e-5.
# "logmel real abs": the production tables on a speech-like wave, never above the 2e-4 of tests/test_feature_gpu.py.
# "meannorm abs": random f32 rows (normal, mean 5), never above 1e-6 max|Y|.  Measured 0 in all 78 cases, and that is no accident: float64
# sums of at most 8193 f32 values between 2^-2 and 2^4 need 43 of float64's 53 bits, so they are exact in any order and the device result
# is bit-defined for these rows too.  The bar is therefore 0.
BARS = {
    "logmel probe abs": 1.7e-6,            # measured 8.17e-7 (897 launches; |log10| <= 6.6, one ulp there is 4.8e-7)
    "logmel real abs": 2.1e-6,             # measured 1.03e-6 (81 launches; existing bar 2e-4)
    "meannorm abs": 0.0,                   # measured 0
}
WORST = {}
FLOOR_BITS = set()


def _bar(key, err):
    """print the measured error, remember the worst, assert the bar"""
    err = float(err)
    WORST[key] = max(WORST.get(key, 0.0), err)
    print(f"  {key}: error {err:.3e} (bar {BARS[key]:.1e}, worst so far {WORST[key]:.3e})")
    assert err <= BARS[key], (key, err)


def _rc(L, name, *args):
    """one C-ABI call on the current stream -> its return code"""
    a = [x.data_ptr() if isinstance(x, torch.Tensor) else x for x in args]
    return getattr(L, name)(*a, torch.cuda.current_stream().cuda_stream)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: I32, 8: I64, 2: I16}[t.element_size()])


def _same(got, want):
    """bit for bit up to the sign of zero; NaN must sit exactly where it is expected"""
    got = torch.as_tensor(got).detach().cpu().double()
    want = torch.as_tensor(np.asarray(want) if not isinstance(want, torch.Tensor) else want).detach().cpu().double()
    return got.shape == want.shape and torch.equal(got.isnan(), want.isnan()) and torch.equal(got.nan_to_num(0.0), want.nan_to_num(0.0))


def _framed(rows, width, dev):
    """a NaN output of `rows` rows between two NaN canary rows -> (whole buffer, the view to hand to the kernel)"""
    buf = torch.full((rows + 2, width), NAN, dtype=F32, device=dev)
    return buf, buf[1:1 + rows]


def _canaries_intact(buf):
    return bool(buf[0].isnan().all()) and bool(buf[-1].isnan().all())


def _dev(a, dev, dtype=F32):
    t = torch.from_numpy(np.ascontiguousarray(a))
    r = t.to(dtype)
    assert torch.equal(r.double(), t.double()), "not exact in the device type"
    return r.to(dev)


@functools.lru_cache(maxsize=None)
def _probe(name, n, seed=0):
    y, dft, melT = E.probe(name, n, seed)
    E.assert_exact(y, dft, melT)
    return y, dft, melT


def _tables(name, dev):
    """(dft, melT) float64 numpy and their f32 device copies; "prod": the production tables"""
    if name == "prod":
        from fs_eend_amd import feature
        d, m = feature._tables(dev)
        return d.cpu().double().numpy(), m.cpu().double().numpy(), d, m
    _, dft, melT = _probe(name, 16)
    return dft, melT, _dev(dft, dev), _dev(melT, dev)


def _samples(name, n, seed):
    """float64 samples, exact in f32: the probe's integers, or for "prod" a speech-like wave over a noise floor"""
    return E.speechlike(n, seed, floor=0.03).astype(np.float64) if name == "prod" else _probe(name, n, seed)[0]


def _padded(y, length, dev):
    """device buffer [PRE NaN | y[0 : length] | PRE NaN] -> (buffer, the view whose element 0 is sample 0)"""
    buf = torch.full((PRE + len(y) + PRE,), NAN, dtype=F32, device=dev)
    buf[PRE:PRE + length] = y[:length]
    return buf, buf[PRE:]


def _stft(L, yview, length, first, n_frames, dftd, meld, dev):
    buf, out = _framed(n_frames, E.NMEL, dev)
    assert _rc(L, "eend_stft_logmel23_f32", yview, length, first, n_frames, dftd, meld, out) == 0
    assert _canaries_intact(buf)
    return out


# ==================================================================================================== eend_stft_logmel23_f32
SPAN = 28 + E.HOP * 128 + E.WIN + 400


@pytest.mark.parametrize("n_frames", E.N_FRAMES)
@pytest.mark.parametrize("name", E.PROBES)
def test_stft_probe(hip_lib, dev, name, n_frames):
    """both probe families at every (first, len) edge: outputs whose reference power is zero (frames or picked taps wholly outside
    [0, len)) carry the one bit pattern of log10f(1e-10f); all others are log10 of an exactly known integer"""
    L = hip_lib
    nb, fpb, waves = E.stft_grid(n_frames)
    print(f"eend_stft_logmel23_f32 {name}: frames {n_frames} -> blocks {nb}, frames per block {fpb}, waves in the last block {waves}, table passes {E.WIN // E.KC}")
    y, dft, melT = _probe(name, SPAN)
    dftd, meld, yd = _dev(dft, dev), _dev(melT, dev), _dev(y, dev)
    worst, floors, cases = 0.0, 0, 0
    for first in E.FIRSTS:
        for length in E.stft_lengths(first, n_frames) + [SPAN]:
            _, yview = _padded(yd, length, dev)
            got = _stft(L, yview, length, first, n_frames, dftd, meld, dev).cpu()
            power = E.ref_melpower(y, length, first, n_frames, dft, melT)
            assert not got.isnan().any(), (first, length)
            zero = torch.from_numpy(power == 0)
            if zero.any():
                FLOOR_BITS.update(_bits(got)[zero].unique().tolist())
                assert (got[zero] + 10.0).abs().max() <= 2e-6
                floors += int(zero.sum())
            if (~zero).any():
                want = torch.from_numpy(np.log10(np.maximum(power, E.FLOOR)))
                worst = max(worst, float((got.double() - want)[~zero].abs().max()))
            cases += 1
    assert len(FLOOR_BITS) <= 1, FLOOR_BITS
    print(f"  {cases} launches, {floors} floor outputs with bits {sorted(FLOOR_BITS)}")
    assert BARS["logmel probe abs"] < E.PICK_STEP / 64
    _bar("logmel probe abs", worst)


@pytest.mark.parametrize("n_frames", E.N_FRAMES)
def test_stft_production_tables(hip_lib, dev, n_frames):
    """the production tables on a speech-like wave over a noise floor: every reference mel power >= 1e-6, so the log amplifies nothing"""
    L = hip_lib
    dft, melT, dftd, meld = _tables("prod", dev)
    y = _samples("prod", SPAN, 11)
    yd = torch.from_numpy(y).to(F32).to(dev)
    y = yd.cpu().double().numpy()
    worst = 0.0
    for first in (-100, 28, 0):
        last = first + E.HOP * (n_frames - 1) + E.WIN - 1
        for length in (last + 1, last, SPAN):
            _, yview = _padded(yd, length, dev)
            got = _stft(L, yview, length, first, n_frames, dftd, meld, dev).cpu().double()
            power = E.ref_melpower(y, length, first, n_frames, dft, melT)
            assert power.min() >= 1e-6, power.min()
            worst = max(worst, float((got - torch.from_numpy(np.log10(power))).abs().max()))
    assert BARS["logmel real abs"] <= 2e-4
    _bar("logmel real abs", worst)


@pytest.mark.parametrize("name", E.PROBES + ("prod",))
def test_stft_blocks_are_independent(hip_lib, dev, name):
    """a launch of B frames equals its blocks launched one at a time with `first` moved on, bit for bit"""
    L = hip_lib
    dft, melT, dftd, meld = _tables(name, dev)
    yd = torch.from_numpy(_samples(name, SPAN, 3)).to(F32).to(dev)
    for first, n_frames, length in ((-100, 129, SPAN), (28, 129, 9000), (-200, 65, 5200), (0, 128, 7001)):
        _, yview = _padded(yd, length, dev)
        whole = _stft(L, yview, length, first, n_frames, dftd, meld, dev)
        for b in range(-(-n_frames // E.FB)):
            k = min(E.FB, n_frames - E.FB * b)
            part = _stft(L, yview, length, first + E.HOP * E.FB * b, k, dftd, meld, dev)
            assert _same(part, whole[E.FB * b:E.FB * b + k]), (name, first, n_frames, b)
    print(f"eend_stft_logmel23_f32 {name}: blocks 3 / 3 / 2 / 2 against one-block launches")


# ==================================================================================================== eend_feature_meannorm_f32
@pytest.mark.parametrize("T", E.NORM_T)
def test_meannorm(hip_lib, dev, T):
    L = hip_lib
    for F in E.NORM_F:
        print(f"eend_feature_meannorm_f32: T {T} F {F} -> blocks {F} of {E.NT2} threads, mode 1 strides {-(-T // E.NT2)}, mode 2 scan passes {-(-T // E.SCAN)}")
        Yq = E.quantised(T, F, T + F)
        g = np.random.default_rng(T * 64 + F)
        Yr = (g.standard_normal((T, F)) + 5.0).astype(np.float32)
        assert BARS["meannorm abs"] <= 1e-6 * np.abs(Yr).max()
        for mode in (1, 2):
            for Y, exact in ((Yq, True), (Yr, False)):
                Yd = torch.full((T + 8, F), NAN, dtype=F32, device=dev)                 # NaN rows behind T
                Yd[:T] = torch.from_numpy(Y).to(dev)
                before = Yd.clone()
                buf, out = _framed(T, F, dev)
                assert _rc(L, "eend_feature_meannorm_f32", Yd, out, T, F, mode) == 0
                assert _canaries_intact(buf) and _same(Yd, before)
                want = E.ref_meannorm(Y, mode)
                if exact:
                    assert _same(out, want), (T, F, mode)
                else:
                    assert not out.isnan().any()
                    _bar("meannorm abs", (out.cpu().double() - torch.from_numpy(want).double()).abs().max())


# ==================================================================================================== eend_splice_subsample_f32
@pytest.mark.parametrize("T,F,ctx,sub", E.SPLICE_CASES)
def test_splice_subsample(hip_lib, dev, T, F, ctx, sub):
    L = hip_lib
    n, nb = E.splice_grid(T, F, ctx, sub)
    print(f"eend_splice_subsample_f32: T {T} F {F} ctx {ctx} sub {sub} -> {n} elements, blocks {nb} of 256 threads")
    Y = np.random.default_rng(T + 7 * F).standard_normal((T, F)).astype(np.float32)
    Yd = torch.full((T + 2 * ctx + sub + 4, F), NAN, dtype=F32, device=dev)             # NaN rows behind T: never read
    Yd[:T] = torch.from_numpy(Y).to(dev)
    rows, W = -(-T // sub), F * (2 * ctx + 1)
    buf, out = _framed(rows, W, dev)
    assert _rc(L, "eend_splice_subsample_f32", Yd, T, F, ctx, sub, out) == 0
    assert _canaries_intact(buf) and _same(out, E.ref_splice(Y, ctx, sub))


# ==================================================================================================== eend_audio_feed_f32 (AudioFrontEnd)
def _stream_lengths(schedule):
    """{slot: [length of each of its streams]}"""
    n = {s: [0] for s in range(4)}
    for _, feed, _, reset in schedule:
        for s in reset:
            n[s].append(0)
        for s, m in feed.items():
            n[s][-1] += m
    return n


@pytest.mark.parametrize("mode", ("logmel23", "logmel23_cummn"))
@pytest.mark.parametrize("tables", ("prod", "probe"))
@pytest.mark.parametrize("ctx,sub", E.STREAM_PAIRS)
def test_audio_feed_walk(hip_lib, dev, ctx, sub, tables, mode):
    """four slots on the schedule of E.stream_schedule (its docstring lists the cuts), the state rows NaN to begin with"""
    from fs_eend_amd.audio_stream import AudioFrontEnd
    L = hip_lib
    if tables == "probe":
        tables = "dense" if (ctx + sub) % 2 else "pick0"
    fe = AudioFrontEnd(4, mode, ctx, sub, device=dev)
    dft, melT, fe.dft, fe.melT = _tables(tables, dev)
    for t in (fe.tail, fe.ring, fe.sums):
        t.fill_(NAN)
    schedule = E.stream_schedule()
    lengths = _stream_lengths(schedule)
    waves = {s: [_samples(tables, max(n, 1), 10 * s + k)[:n] for k, n in enumerate(v)] for s, v in lengths.items()}
    waves[3][1] = np.full(lengths[3][1], NAN)                                           # the stream whose leftovers the next one must not see
    wd = {s: [torch.from_numpy(w).to(F32) for w in v] for s, v in waves.items()}
    cur, pos = {s: 0 for s in range(4)}, {s: 0 for s in range(4)}
    cuts = {s: [[] for _ in v] for s, v in lengths.items()}
    outs = {s: [[] for _ in v] for s, v in lengths.items()}
    changed, named_in = [], []
    for s in range(4):
        fe.reset(s)
    stft_tiles = splice_tiles = 0
    recv, frames = {s: 0 for s in range(4)}, {s: 0 for s in range(4)}
    for c, feed, end, reset in schedule:
        for s in reset:
            fe.reset(s)
            cur[s] += 1
            pos[s] = recv[s] = frames[s] = 0
        snap = [t.clone() for t in (fe.tail, fe.ring, fe.sums)]
        call = {}
        for s in sorted(feed, reverse=bool(c % 2)):
            w = wd[s][cur[s]][pos[s]:pos[s] + feed[s]]
            call[s] = w.to(dev) if (c + s) % 2 else w
            pos[s] += feed[s]
            cuts[s][cur[s]].append((feed[s], s in end))
        for s in end:
            if s not in feed:
                cuts[s][cur[s]].append((0, True))
        got = fe.feed(call, end=end)
        assert set(got) == set(feed) | set(end)
        for s, v in got.items():
            outs[s][cur[s]].append(v)
            recv[s] += feed.get(s, 0)
            new = E.ready_frames(recv[s], s in end) - frames[s]
            frames[s] += new
            stft_tiles = max(stft_tiles, -(-new // E.FB))
            splice_tiles = max(splice_tiles, -(-v.shape[0] // E.SPL_ROWS))
        # per slot: did any bit of its tail / ring / sums row change in this call?  (kept on the device, read once at the end)
        now = (fe.tail, fe.ring, fe.sums)
        diff = [(a.view(I32 if a.dtype == F32 else I64) != b.view(I32 if b.dtype == F32 else I64)).reshape(4, -1).any(1) for a, b in zip(now, snap)]
        changed.append(torch.stack(diff).any(0))
        named_in.append(set(got))
    changed = torch.stack(changed).cpu()
    assert changed[0, 0] and changed[:, 2].sum() >= 9                                   # the comparison sees a fed slot's rows move
    for i, named in enumerate(named_in):
        for s in range(4):
            assert s in named or not changed[i, s], f"call {schedule[i][0]} changed the state of slot {s}, which it does not name"
    print(f"eend_audio_feed_f32 {tables} {mode} ctx {ctx} sub {sub}: {len(schedule)} calls, up to {max(len(n) for n in named_in)} slots a call, "
          f"up to {stft_tiles} STFT tiles and {splice_tiles} splice tiles for a slot")
    for s in range(4):
        for k, n in enumerate(lengths[s]):
            T = int(E.stft_frames(n))
            W = E.NMEL * (2 * ctx + 1)
            got = torch.cat(outs[s][k]) if outs[s][k] else torch.zeros(0, W)
            if T == 0:
                assert got.shape[0] == 0
                continue
            yd = wd[s][k].to(dev)
            _, yview = _padded(yd, n, dev)
            lm = _stft(L, yview, n, -100, T, fe.dft, fe.melT, dev)
            want, counts = E.ref_stream(waves[s][k], cuts[s][k], ctx, sub, fe.mode, None, logmel=lm.cpu().numpy())
            assert [v.shape[0] for v in outs[s][k]] == counts, (s, k)
            assert _same(got, want), f"slot {s} stream {k}: the feeds do not add up to the whole waveform's rows"
            if fe.mode == 0:
                buf, spl = _framed(want.shape[0], W, dev)
                assert _rc(L, "eend_splice_subsample_f32", lm, T, E.NMEL, ctx, sub, spl) == 0
                assert _same(got, spl)
    # slot 3, reused after the NaN stream, against a slot of a front-end that never saw one: the same feeds, the same bits
    fresh = AudioFrontEnd(1, mode, ctx, sub, device=dev)
    fresh.dft, fresh.melT = fe.dft, fe.melT
    fresh.reset(0)
    at = 0
    for (m, ended), v in zip(cuts[3][2], outs[3][2]):
        assert _same(fresh.feed({0: wd[3][2][at:at + m]}, end=[0] if ended else [])[0], v)
        at += m
    assert at == lengths[3][2] and not torch.cat(outs[3][2]).isnan().any()


# ==================================================================================================== eend_chunk_batch_f32 (DeviceCorpus)
@functools.lru_cache(maxsize=None)
def _corpus_samples(probe):
    """float64 probe integers of the whole corpus and the cover mask"""
    total = sum(E.CHUNK_LENS.values())
    return _probe(probe, total, 77)[0], E.chunk_cover()


@functools.lru_cache(maxsize=None)
def _labels(S):
    """the header's label rule at full frame rate, per chunk (tests/chunk_label_ref.py)"""
    segs = E.chunk_segments(S)
    return [C.chunk_labels(*segs[rec], E.CHUNK_LENS[rec], st, ed, S) for rec, st, ed in E.CHUNK_ROWS]


def _build_corpus(dev, storage, probe, S):
    from fs_eend_amd.device_data import DeviceCorpus
    y, cover = _corpus_samples(probe)
    if storage == "f32":
        w = np.where(cover, y, np.nan).astype(np.float32)
    else:
        w = np.where(cover, y, np.where(np.arange(len(y)) % 2, 32767, -32768)).astype(np.int16)
    corpus = DeviceCorpus(dev, storage=storage)
    segs, at = E.chunk_segments(S), 0
    for rec, n in E.CHUNK_LENS.items():
        corpus.add(rec, torch.from_numpy(w[at:at + n].copy()), *segs[rec])
        at += n
    corpus.finalize()
    decoded = w.astype(np.float32) if storage == "f32" else (w.astype(np.float32) / np.float32(32768.0))
    return corpus, decoded


@pytest.mark.parametrize("ctx,sub", [(7, 10), (0, 1), (15, 16)])
@pytest.mark.parametrize("transform,mode", [("logmel23", 0), ("logmel23_mn", 1), ("logmel23_cummn", 2)])
def test_chunk_batch(hip_lib, dev, transform, mode, ctx, sub):
    from fs_eend_amd import device_data as DD
    L = hip_lib
    case = 3 * mode + [(7, 10), (0, 1), (15, 16)].index((ctx, sub))                     # deals probe family and S_max over the nine cases
    W = E.NMEL * (2 * ctx + 1)
    rows = list(E.CHUNK_ROWS)
    for si, storage in enumerate(("f32", "s16")):
        probe = ("dense", "pick0")[(case + si) % 2]
        S = (1, 5, 64)[(case + si) % 3]
        corpus, decoded = _build_corpus(dev, storage, probe, S)
        _, dftn, meln = _probe(probe, 16)
        corpus.dft, corpus.melT = _dev(dftn, dev), _dev(meln, dev)
        E.assert_exact(_corpus_samples(probe)[0] / 32768.0, dftn, meln, unit=2.0 ** -15)
        p, Ss, S_max, _ = corpus.plan(rows, ctx, sub, transform, n_speakers=S)
        assert S_max == S and p["frames"].tolist() == list(E.CHUNK_FRAMES)
        print(f"eend_chunk_batch_f32 {storage} {probe} mode {mode} ctx {ctx} sub {sub} S_max {S}: chunks {len(rows)}, STFT tiles {len(p['stft'])}, "
              f"colnorm grid {E.NMEL} x {len(rows)} with up to {-(-int(p['frames'].max()) // E.SCAN)} scan passes, splice tiles {len(p['splice'])}")
        # the pool seeded with NaN: outputs fully written, nothing behind them touched
        sizes = {"feats": p["o_rows"] * W, "labels": p["o_rows"] * S, "Y": p["y_rows"] * E.NMEL, "Yn": p["y_rows"] * E.NMEL if mode else 0}
        for k, n in sizes.items():
            corpus._pool[k] = torch.full((n + 512,), NAN, dtype=F32, device=dev)
        feats, labels, _ = corpus.batch(rows, ctx, sub, transform, n_speakers=S)
        for k, n in sizes.items():
            assert corpus._pool[k][n:].isnan().all() and not corpus._pool[k][:n].isnan().any(), k
        feats, labels = [f.clone() for f in feats], [l.clone() for l in labels]
        # features: the three single-waveform entries on corpus[off : off + len]
        at = dict(zip(E.CHUNK_LENS, np.cumsum([0] + list(E.CHUNK_LENS.values()))[:-1].tolist()))
        for b, (rec, st, ed) in enumerate(rows):
            a, n = DD.chunk_samples(E.CHUNK_LENS[rec], st, ed)
            T = int(p["frames"][b])
            piece = torch.from_numpy(decoded[at[rec] + a:at[rec] + a + n].copy()).to(dev)
            assert not piece.isnan().any()
            _, yview = _padded(piece, n, dev)
            lm = _stft(L, yview, n, -100, T, corpus.dft, corpus.melT, dev)
            if mode:
                nbuf, norm = _framed(T, E.NMEL, dev)
                assert _rc(L, "eend_feature_meannorm_f32", lm, norm, T, E.NMEL, mode) == 0
                lm = norm
            sbuf, spl = _framed(-(-T // sub), W, dev)
            assert _rc(L, "eend_splice_subsample_f32", lm, T, E.NMEL, ctx, sub, spl) == 0
            assert _same(feats[b], spl), f"chunk {b} {rows[b]}: features differ from the single-waveform entries"
            assert _same(labels[b], C.subsampled(_labels(S)[b], sub)), f"chunk {b} {rows[b]}: labels"
        # batch mates and position: the same chunks reversed, and a few of them alone
        for order in (list(range(len(rows)))[::-1], [4, 0, 6], [2]):
            f2, l2, _ = corpus.batch([rows[i] for i in order], ctx, sub, transform, n_speakers=S)
            for i, f, l in zip(order, f2, l2):
                assert _same(f, feats[i]) and _same(l, labels[i]), (order, i)


# ==================================================================================================== arguments
def test_einval_leaves_outputs_untouched(hip_lib, dev):
    """arguments the host refuses before any launch: -1 and every output still NaN"""
    L = hip_lib
    nan = lambda *s, dt=F32: torch.full(s, NAN, dtype=dt, device=dev)
    _, _, dftd, meld = _tables("dense", dev)
    y, out = torch.ones(400, device=dev), nan(4, 23)
    for args in ((None, 400, -100, 2, dftd, meld, out), (y, 400, -100, 2, None, meld, out), (y, 400, -100, 2, dftd, None, out),
                 (y, 400, -100, 2, dftd, meld, None), (y, 0, -100, 2, dftd, meld, out), (y, -1, -100, 2, dftd, meld, out),
                 (y, 400, -100, 0, dftd, meld, out), (y, 400, -100, -3, dftd, meld, out)):
        assert _rc(L, "eend_stft_logmel23_f32", *args) == EINVAL, args[1:4]
    Y = torch.ones(8, 23, device=dev)
    for args in ((Y, out, 4, 23, 0), (Y, out, 4, 23, 3), (Y, out, 0, 23, 1), (Y, out, 4, 0, 2), (None, out, 4, 23, 1), (Y, None, 4, 23, 1)):
        assert _rc(L, "eend_feature_meannorm_f32", *args) == EINVAL, args[2:]
    for args in ((Y, 4, 23, -1, 1, out), (Y, 4, 23, 0, 0, out), (Y, 0, 23, 0, 1, out), (Y, 4, 0, 0, 1, out), (None, 4, 23, 0, 1, out), (Y, 4, 23, 0, 1, None)):
        assert _rc(L, "eend_splice_subsample_f32", *args) == EINVAL, args[1:5]
    assert out.isnan().all()
    # feed: one well-formed descriptor (a slot receiving 180 samples: two frames), refused for its scalar arguments alone
    chunk = torch.ones(180, device=dev)
    desc = torch.tensor([[chunk.data_ptr(), 0, 180, 0, 2, 0, 0, 0, 0]], dtype=I64, device=dev)
    st, sp = torch.tensor([[0, 0, 2]], dtype=I64, device=dev), torch.tensor([[0, 0, 2, 0]], dtype=I64, device=dev)
    tail, ring, sums, Ys, fo = nan(2, 200), nan(2, 32, 23), nan(2, 23, dt=F64), nan(8, 23), nan(4, 23)
    good = dict(desc=desc, n_desc=1, st=st, n_stft=1, sp=sp, n_splice=1, tail=tail, ring=ring, sums=sums, Y=Ys, out=fo, mode=0, ctx=0, sub=1, dft=dftd, melT=meld)
    for bad in (dict(mode=1), dict(mode=3), dict(mode=-1), dict(ctx=16), dict(ctx=-1), dict(sub=0), dict(sub=17), dict(n_desc=-1), dict(n_desc=0),
                dict(n_stft=-1), dict(n_splice=-1), dict(dft=None), dict(melT=None), dict(st=None), dict(Y=None), dict(sp=None), dict(out=None),
                dict(desc=None), dict(tail=None), dict(ring=None), dict(sums=None)):
        a = {**good, **bad}
        assert _rc(L, "eend_audio_feed_f32", *a.values()) == EINVAL, bad
    for t in (tail, ring, sums, Ys, fo):
        assert t.isnan().all()
    # chunk batch: likewise
    corpus = torch.ones(400, device=dev)
    segs = torch.zeros(1, 3, dtype=I32, device=dev)
    cd = torch.tensor([[0, 180, 3, 0, 0, 3, 0, 1]], dtype=I64, device=dev)
    cs, cp = torch.tensor([[0, 0, 3]], dtype=I64, device=dev), torch.tensor([[0, 0, 3, 0]], dtype=I64, device=dev)
    Yc, Yn, feats, labels = nan(4, 23), nan(4, 23), nan(4, 23), nan(4, 64)
    good = dict(corpus=corpus, storage=0, segs=segs, desc=cd, n=1, st=cs, n_stft=1, sp=cp, n_splice=1, Y=Yc, Yn=Yn, feats=feats, labels=labels, S=2, mode=1,
                ctx=0, sub=1, dft=dftd, melT=meld)
    for bad in (dict(storage=2), dict(storage=-1), dict(mode=3), dict(mode=-1), dict(ctx=65), dict(ctx=-1), dict(sub=0), dict(sub=4097), dict(S=0), dict(S=65),
                dict(n=65536), dict(n=-1), dict(n=0), dict(n_stft=-1), dict(n_splice=-1), dict(dft=None), dict(melT=None), dict(corpus=None), dict(desc=None),
                dict(segs=None), dict(st=None), dict(Y=None), dict(Yn=None), dict(sp=None), dict(feats=None), dict(labels=None), dict(n_stft=0)):
        a = {**good, **bad}
        assert _rc(L, "eend_chunk_batch_f32", *a.values()) == EINVAL, bad
    for t in (Yc, Yn, feats, labels):
        assert t.isnan().all()
