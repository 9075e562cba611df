"""What the audio paths share on the host (`audio_stream`, `audio_ingest`, `device_data` and `feature` import it; it imports none
of them): the layout constants of csrc/feature.hip and csrc/resample.hip, the batch frame count, the free / open / ended slot
table that `audio_stream.FrontEndTable` and `audio_ingest.IngestTable` specialise, with the snapshot of one slot, and `Staging`,
the pinned block that carries a feed's words and CPU chunks to the device in one copy."""
import torch

from .multistream import SlotError

F32 = torch.float32
# csrc/feature.hip
HOP, WIN, NMEL = 80, 200, 23               # constexpr HOP, WIN, NMEL: frame f reads samples 80 f - 100 .. 80 f + 99
TAIL, RING = 200, 32                       # constexpr TAIL, RING: per-slot sample tail and log-mel ring
FB, SPL_ROWS, FEED_N, CHUNK_N = 64, 16, 9, 8   # constexpr FB, SPL_ROWS: log-mel frames per STFT tile, model frames per splice
#                                                tile; enum FEED_N, CHUNK_N: fields of a feed and of a chunk descriptor
# csrc/resample.hip
HIST, TILE, DESC_N = 256, 256, 8           # constexpr NT: history row and outputs per tile; enum ING_N: descriptor fields

FREE, OPEN, ENDED = "free", "open", "ended"


def stft_frames(n):
    """Log-mel frames of a whole recording of n samples (an int or a numpy array of them): 1 + n // 80, the excess last frame
    dropped ({LS,FS}-EEND/datasets/feature.py:166-191)."""
    return 1 + n // HOP - (n % HOP == 0)


class SlotTable:
    """Host bookkeeping of one stage of the audio path (pure Python, no device): per slot its state free / open / ended and the
    stage's counters.  reset(s) starts an empty stream in any slot; a slot fed its end accepts no more audio until the next
    reset.  A subclass names its counters, `counters` = {counter: the field of its plan record that becomes its next value}
    with "recv" among them, and gives `advance`."""

    counters = {}

    def __init__(self, slots: int, what: str):
        if slots <= 0:
            raise SlotError(f"{what} needs at least one slot")
        self.S = slots
        self.state = [FREE] * slots
        for k in self.counters:
            setattr(self, k, [0] * slots)

    def advance(self, s: int, recv1: int, ended: bool):
        """The plan record of slot s once it has received recv1 samples in all."""
        raise NotImplementedError

    def _check(self, s):
        if not isinstance(s, int) or not 0 <= s < self.S:
            raise SlotError(f"slot {s!r} out of range 0..{self.S - 1}")

    def _check_open(self, s):
        self._check(s)
        if self.state[s] == FREE:
            raise SlotError(f"slot {s} is not open (reset it first)")

    def reset(self, s):
        self._check(s)
        self.state[s] = OPEN
        for k in self.counters:
            getattr(self, k)[s] = 0

    def close(self, s):
        self._check(s)
        self.state[s] = FREE

    def plan(self, counts, end=()):
        """counts: {slot: new samples}; end: slots whose audio ends with this call.  -> [plan record] in slot order."""
        counts, end = dict(counts), list(end)
        if len(set(end)) != len(end):
            raise SlotError("a slot is named twice in end")
        for s in list(counts) + end:
            self._check_open(s)
            if self.state[s] == ENDED:
                raise SlotError(f"slot {s} was fed its end; reset it to start a new stream")
        for s, n in counts.items():
            if not isinstance(n, int) or n < 0:
                raise ValueError(f"slot {s}: sample count must be a non-negative int, got {n!r}")
        return [self.advance(s, self.recv[s] + counts.get(s, 0), s in end) for s in sorted(set(counts) | set(end))]

    def commit(self, plan):
        for p in plan:
            for k, field in self.counters.items():
                getattr(self, k)[p.slot] = getattr(p, field)
            if p.ended:
                self.state[p.slot] = ENDED

    # ---- a slot's stream leaves / comes back: `rows` = {name: per-slot device tensor}, each slot's row travels under its name
    def export(self, s: int, config: dict, rows: dict) -> dict:
        """Slot s as plain values and tensors: the config, copies of its rows and its counters."""
        self._check_open(s)
        return {"config": config, **{k: r[s].clone() for k, r in rows.items()}, **{k: getattr(self, k)[s] for k in self.counters}}

    def fits(self, part, config: dict, rows: dict) -> bool:
        """Whether `part` is an export under the same config, with counters and rows of the right kind."""
        return (isinstance(part, dict) and part.get("config") == config
                and all(isinstance(part.get(k), int) and part[k] >= 0 for k in self.counters)
                and all(torch.is_tensor(part.get(k)) and part[k].shape == r.shape[1:] and part[k].dtype == r.dtype
                        for k, r in rows.items()))

    def adopt(self, s: int, part: dict, rows: dict, state: str):
        """Slot s goes on from an exported `part` (one that fits) in `state`: ordinary row copies on the current stream."""
        self._check(s)
        for k, r in rows.items():
            r[s].copy_(part[k], non_blocking=True)
        self.state[s] = state
        for k in self.counters:
            getattr(self, k)[s] = part[k]


def there(part):
    """The config an exported part names, for the text of a refusal."""
    return part.get("config") if isinstance(part, dict) else part


class Staging:
    """The block a feed sends to the device with one asynchronous copy: i64 words (descriptors and tile tables) first, then the
    CPU chunks of the call as `dtype`, each starting on an 8-byte boundary.  `place` returns a chunk's device address, or
    -1 - (its element offset behind the words) for `upload` to patch."""

    def __init__(self, dev, dtype):
        self.dev, self.dtype = dev, dtype
        self.esize = torch.empty(0, dtype=dtype).element_size()
        self.every = 8 // self.esize
        self.keep, self.host, self.n = [], [], 0            # device chunks kept alive; (element offset, CPU chunk); elements placed

    def place(self, w) -> int:
        if w is None or not w.numel():
            return 0
        if w.is_cuda:
            w = w.to(device=self.dev, dtype=self.dtype).contiguous()
            self.keep.append(w)
            return w.data_ptr()
        off = self.n
        self.host.append((off, w.to(self.dtype).contiguous()))
        self.n = -(-(off + w.numel()) // self.every) * self.every
        return -1 - off

    def upload(self, words, chunk_at):
        """words: the i64 words; chunk_at: the indices in it of values `place` returned.  -> (device block, its address)."""
        head = 8 * len(words)
        nbytes = head + self.esize * self.n
        dbuf = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        base = dbuf.data_ptr()
        for i in chunk_at:
            if words[i] < 0:
                words[i] = base + head + self.esize * (-1 - words[i])
        stage = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)   # a fresh pinned block per call (copied asynchronously)
        stage[:head].view(torch.int64).copy_(torch.tensor(words, dtype=torch.int64))
        if self.n:
            samples = stage[head:].view(self.dtype)
            for off, w in self.host:
                samples[off:off + w.numel()].copy_(w)
        dbuf.copy_(stage, non_blocking=True)
        return dbuf, base
