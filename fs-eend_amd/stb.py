"""Block-online EEND-EDA with a speaker-tracing buffer (STB) for many streams at once.

The reference's online EEND-EDA baseline (FS-EEND/train/tfm_STB.py:147-204, conf/spk_STB.yaml, with find_best_perm, cal_cor,
upd_buf and upd_buf_FIFO of train/utils/utils.py) runs the offline model on [buffer; new block], block after block, one recording
at a time, with the speaker count and the assignment taken on the host.  `StbSession` runs the same loop for `slots` streams: the
streams whose block is ready are grouped by their row count T = L + n (the host knows L exactly), and a group is ONE batched pass

    centre (eend_stb_center_f32) -> encoder -> attractors, every stream with its own frame order (eend_lstm_orders_f32)
    -> counter, head -> track (eend_stb_track_f32: sigmoid, correlations, assignment, emitted block, buffer selection)

with nothing read back: `step` never waits for the device.  In steady state there is one group, during warm-up at most
buf_size / blk_size + 1.  A stream's results are a function of its own frames, key, seed and the parameters alone.

Deliberate deviations from the reference:
  1. the buffer draw of policy "kld" is the exponential race on a counter-based hash of (stream seed, block, row) instead of
     WeightedRandomSampler: the same distribution, reproducible per stream (include/eend_hip.h states the hash);
  2. assignment ties: padding rows and columns have correlation 0 with everything; only pairs of a tracked row and a predicted
     column come from the solver, the other rows take the columns left over in ascending order;
  3. with no tracked speaker the selection weights are uniform and the emitted block has width 0 (the reference divides by zero);
     a buffered row whose posteriors sum to 0 gets the weight floor 1e-6 (the reference's is NaN);
  4. as eda_model.test: every stream has its own count, and all 15 columns are kept when no probability is below `th`.
Out of scope: snapshots, graph capture, upd_buf_ver2, STB training.
"""
from typing import Callable, Dict, Iterable, Optional

import numpy as np
import torch
from torch import Tensor

from . import ops
from .eda_model import MAX_N_SPEAKERS, TransformerEDADiarization, _slab_logits, check_order
from .lib import EendHipError
from .multistream import DONE, FREE, OPEN, SlotError

F32, I32 = torch.float32, torch.int32
_M32, _M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def _mix(x: int) -> int:
    """murmur3's 32-bit finaliser, the mixing function of csrc/stb.hip."""
    x &= _M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & _M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & _M32
    x ^= x >> 16
    return x


def stream_seed(seed: int, key: int) -> int:
    """The 32-bit seed of a stream's buffer draws from the session's seed and the stream's key."""
    key = int(key) & _M64
    return _mix(_mix(int(seed) & _M32) + ((key & _M32) ^ (key >> 32)))


def draw_order(seed: int, key: int, k: int, T: int) -> np.ndarray:
    """The order in which the encoder LSTM reads the T rows of block k of stream `key` (the reference shuffles np.arange(T) on the
    global numpy state, model :62-65; here on a Generator of its own, so a stream does not depend on what else draws)."""
    rng = np.random.default_rng([int(seed) & _M64, int(key) & _M64, int(k), int(T)])
    return rng.permutation(T).astype(np.int32)


class StbSession:
    """`slots` independent block-online EEND-EDA streams on one offline model (eda_model.TransformerEDADiarization)."""

    def __init__(self, model, slots: int, buf_size: int = 1000, blk_size: int = 100, th: float = 0.5, policy: str = "kld",
                 seed: int = 0, orders: Optional[Callable[[int, int, int], Iterable[int]]] = None, debug: bool = False):
        """orders(key, k, T) -> the frame order of block k of stream `key` (default: draw_order).  debug: keep, per block of the
        last step, what went through the pass (`last_blocks`: centred rows, order, logits, count, perm, kept rows) -- for tests;
        without it the kernel's perm / kept-row outputs are not even written."""
        if not isinstance(model, TransformerEDADiarization):
            raise EendHipError("StbSession runs eda_model.TransformerEDADiarization")
        if slots <= 0:
            raise SlotError("a session needs at least one slot")
        if blk_size < 1 or blk_size > buf_size:
            raise ValueError(f"blk_size {blk_size} must be in 1 .. buf_size ({buf_size})")
        if policy not in ops.STB_POLICIES:
            raise ValueError(f"unknown buffer policy {policy!r}: one of {sorted(ops.STB_POLICIES)}")
        dev = model.enc.encoder.weight.device
        if dev.type != "cuda":
            raise EendHipError("StbSession: the model must be on the GPU (the HIP path has no CPU fallback)")
        F = int(model.enc.in_size)
        if buf_size + blk_size > ops.STB_MAX_ROWS or F > ops.STB_MAX_FEATURES:
            raise EendHipError(f"StbSession: buf_size + blk_size <= {ops.STB_MAX_ROWS} and in_size <= {ops.STB_MAX_FEATURES}")
        self.model, self.dev, self.F, self.S = model, dev, F, int(slots)
        self.buf_size, self.blk_size, self.th, self.policy, self.seed = int(buf_size), int(blk_size), float(th), policy, int(seed)
        self._orders, self.debug = orders, bool(debug)
        self.x_buf = torch.zeros(self.S, 2, self.buf_size, F, dtype=F32, device=dev)       # ping-pong halves per slot
        self.y_buf = torch.zeros(self.S, 2, self.buf_size, MAX_N_SPEAKERS, dtype=F32, device=dev)
        self.width = torch.zeros(self.S, dtype=I32, device=dev)
        self.state = [FREE] * self.S
        self.key = [0] * self.S
        self.half = [0] * self.S
        self.L = [0] * self.S
        self.k = [0] * self.S
        self.pend = [None] * self.S
        self.out = [[] for _ in range(self.S)]
        self._next_key = 0
        self.last_blocks = []          # debug only: per block of the last step its slot, k, L, n, xc, order, logits, count, perm, sel

    # ---- slots ----
    def _check(self, s):
        if not isinstance(s, int) or isinstance(s, bool) or not 0 <= s < self.S:
            raise SlotError(f"slot {s!r} out of range 0..{self.S - 1}")

    def open(self, key: Optional[int] = None) -> int:
        """Claim the lowest free slot for a new stream.  `key` feeds the stream's seed and its frame orders (default: a counter)."""
        for s, st in enumerate(self.state):
            if st == FREE:
                break
        else:
            raise SlotError(f"all {self.S} slots are in use")
        if key is None:
            key, self._next_key = self._next_key, self._next_key + 1
        self.state[s], self.key[s] = OPEN, int(key)
        self.half[s] = self.L[s] = self.k[s] = 0
        self.pend[s], self.out[s] = None, []
        return s

    def close(self, s: int):
        self._check(s)
        if self.state[s] == FREE:
            raise SlotError(f"slot {s} is not open")
        self.state[s], self.pend[s], self.out[s] = FREE, None, []

    # ---- stepping ----
    def _held(self, s):
        return 0 if self.pend[s] is None else int(self.pend[s].shape[0])

    def step(self, push: Optional[Dict[int, Tensor]] = None, flush=()):
        """Take frames and run every block that is ready.  push {slot: feats (m, F) GPU tensor}; flush: slots whose stream ends after
        this call's frames (their remainder of >= 1 frames runs as a short last block).  -> {slot: (probs (n, 15) f32 with zero
        columns beyond the width, width i32 (1,))} for the slots that ran, n a multiple of blk_size but for a flushed remainder;
        device tensors, nothing is waited for."""
        push, flush = dict(push or {}), list(flush)
        for s in list(push) + flush:
            self._check(s)
        if len(set(flush)) != len(flush):
            raise SlotError("a slot is named twice")
        for s in list(push) + flush:
            if self.state[s] != OPEN:
                raise SlotError(f"{'push to' if s in push else 'flush of'} slot {s}, which is {self.state[s]}")
        feats = {}
        for s, x in push.items():
            if not isinstance(x, Tensor) or not x.is_cuda:
                raise EendHipError(f"push[{s}]: expected a GPU tensor (the HIP path has no CPU fallback)")
            if x.dim() != 2 or x.shape[1] != self.F:
                raise EendHipError(f"push[{s}]: expected (frames, {self.F}), got {tuple(x.shape)}")
            feats[s] = x.detach().to(device=self.dev, dtype=F32)
        # every block this call will run is known on the host: draw and validate all their frame orders before anything changes
        orders = {}
        for s in range(self.S):
            if self.state[s] != OPEN:
                continue
            held = self._held(s) + (int(feats[s].shape[0]) if s in feats else 0)
            sizes = [self.blk_size] * (held // self.blk_size) + ([held % self.blk_size] if s in flush and held % self.blk_size else [])
            L, k = self.L[s], self.k[s]
            for n in sizes:
                T = L + n
                o = self._orders(self.key[s], k, T) if self._orders is not None else draw_order(self.seed, self.key[s], k, T)
                orders[(s, k)] = check_order(o, T)
                L, k = min(T, self.buf_size), k + 1
        for s, x in feats.items():
            if x.shape[0]:
                self.pend[s] = x.contiguous() if self.pend[s] is None else torch.cat([self.pend[s], x], dim=0)
        self.last_blocks = []
        emitted = {}
        while True:
            ready = [(s, self.blk_size) for s in range(self.S) if self.state[s] == OPEN and self._held(s) >= self.blk_size]
            ready += [(s, self._held(s)) for s in flush if 0 < self._held(s) < self.blk_size]
            if not ready:
                break
            groups = {}
            for s, n in ready:
                groups.setdefault(self.L[s] + n, []).append((s, n))
            for T in sorted(groups):
                self._run_group(T, groups[T], emitted, orders)
        for s in flush:
            self.state[s] = DONE
        out = {}
        for s, ys in emitted.items():
            out[s] = (ys[0] if len(ys) == 1 else torch.cat(ys, dim=0), self.width[s:s + 1].clone())
        return out

    def _run_group(self, T, members, emitted, orders):
        B, F, dev = len(members), self.F, self.dev
        W = ops.STB_DESC_WORDS
        # one pinned block per group: the descriptors, then the frame orders
        host = torch.empty(B * W + (B * T + 1) // 2, dtype=torch.int64, pin_memory=True)
        desc_h = host[:B * W].view(B, W).numpy()
        order_h = host[B * W:].view(I32)[:B * T].view(B, T).numpy()
        xc = torch.empty(B, T, F, dtype=F32, device=dev)
        blocks = []
        for b, (s, n) in enumerate(members):
            L, h = self.L[s], self.half[s]
            x_i = self.pend[s][:n]
            y = torch.empty(n, MAX_N_SPEAKERS, dtype=F32, device=dev)
            order_h[b] = orders[(s, self.k[s])]
            desc_h[b] = [self.x_buf[s, h].data_ptr(), L, x_i.data_ptr(), n, self.y_buf[s, h].data_ptr(),
                         self.x_buf[s, 1 - h].data_ptr(), self.y_buf[s, 1 - h].data_ptr(), self.width[s:s + 1].data_ptr(),
                         y.data_ptr(), self.k[s], stream_seed(self.seed, self.key[s]), 0]
            blocks.append(dict(slot=s, k=self.k[s], L=L, n=n, T=T, x_i=x_i, y=y))
        ctl = host.to(dev, non_blocking=True)
        desc = ctl[:B * W].view(B, W)
        order = ctl[B * W:].view(I32)[:B * T].view(B, T)
        ops.stb_center(desc, xc, self.buf_size, self.blk_size)
        model = self.model
        emb, _ = model._encode([xc[b] for b in range(B)])
        attractors, probs, count = model.eda._attractors(emb, T, order, MAX_N_SPEAKERS, self.th)
        logits = _slab_logits(emb, attractors, T)
        perm = torch.empty(B, MAX_N_SPEAKERS, dtype=I32, device=dev) if self.debug else None
        sel = torch.full((B, self.buf_size), -1, dtype=I32, device=dev) if self.debug else None
        ops.stb_track(logits, count, xc, desc, perm, sel, self.buf_size, self.blk_size, ops.STB_POLICIES[self.policy])
        for b, blk in enumerate(blocks):
            s, n = blk["slot"], blk["n"]
            self.pend[s] = self.pend[s][n:] if self._held(s) > n else None
            self.half[s], self.L[s], self.k[s] = 1 - self.half[s], min(T, self.buf_size), self.k[s] + 1
            self.out[s].append(blk["y"])
            emitted.setdefault(s, []).append(blk["y"])
            if self.debug:
                blk.update(xc=xc[b], order=order[b], logits=logits[b], count=count[b:b + 1], probs=probs[b], perm=perm[b], sel=sel[b])
        if self.debug:
            self.last_blocks += blocks

    # ---- results ----
    def frames(self, s: int) -> int:
        self._check(s)
        return sum(int(y.shape[0]) for y in self.out[s])

    def buffer(self, s: int):
        """The stream's buffer as it stands: (x_buf (L, F), y_buf (L, 15), width) -- views and a device int, nothing is waited for."""
        self._check(s)
        if self.state[s] == FREE:
            raise SlotError(f"slot {s} is not open")
        h, L = self.half[s], self.L[s]
        return self.x_buf[s, h, :L], self.y_buf[s, h, :L], self.width[s:s + 1]

    def result(self, s: int) -> Tensor:
        """(frames so far, max width): the emitted blocks right-padded with zeros and concatenated (tfm_STB.py:201-203).  Waits for
        the device (the width is read)."""
        self._check(s)
        if self.state[s] == FREE:
            raise SlotError(f"slot {s} is not open")
        width = int(self.width[s].item()) if self.out[s] else 0        # the width never shrinks: the last one is the largest
        if not self.out[s]:
            return torch.zeros(0, 0, dtype=F32, device=self.dev)
        return torch.cat(self.out[s], dim=0)[:, :width]
