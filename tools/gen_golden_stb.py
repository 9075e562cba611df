"""Golden vectors of block-online EEND-EDA with a speaker-tracing buffer (runs ONLY where the reference checkout exists, like
tools/gen_golden_eda.py).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_stb.py

The reference's functions are evaluated out of its files by path (ast: train/tfm_STB.py imports Lightning and torchaudio): the
helpers find_best_perm, cal_cor, upd_buf (FS-EEND/train/utils/utils.py) and upd_buf_FIFO (LS-EEND/train/utils/utils.py), and the
block loop of SpeakerDiarization.test_step, cut after its `for x, clip_l in zip(feats, clip_lengths)` statement (what follows scores
the result against labels).  Data only is written, to tests/golden/stb_*.npz:

  stb_perm   (a) find_best_perm on small pairs, zero-padded columns on either side, c <= S + 1 so that its answer is unique
  stb_kld    (b) upd_buf with WeightedRandomSampler replaced by a recorder that stores the weights and returns a given index list
  stb_fifo   (c) upd_buf_FIFO
  stb_loop_* (d) the whole loop on the reference's own offline model (built as tools/gen_golden_eda.py builds it: default
             initialisation under the seed, oracle.fixtures.perturb_, the counter gain), one encoder layer, both policies, with
             the exponential race of include/eend_hip.h as the sampler and the frame orders of fs_eend_amd.stb.draw_order put
             in place of np.random.shuffle.  blk 8 / buf 24 / 45 frames ends in a short last block; blk 8 / buf 20 / 44 frames
             fills the buffer at a block's end so that the next block's rows do not all fit.  Per block: order, logits (T, 15),
             count, perm, the kept rows, width; the emitted posteriors; and the reference's own fp32-vs-float64 gap of the
             emitted posteriors (max abs), from the same module and loop under .double().

The loop cases are searched (perturbation seed, threshold) until a test cannot hide a flip, and this is ASSERTED: every count in
1 .. 14 with 1e-2 of clearance between `th` and every probability, the best assignment >= 0.05 of total correlation above the
runner-up, the buf_size-th and the next key >= 1e-3 apart (relative), every decision the same in fp32 and float64.  The reference
hard-codes th = 0.5 in the loop; the model handed to the loop applies the case's threshold instead.
"""
import ast
import copy
import importlib.util
import os
import sys
import time

sys.dont_write_bytecode = True
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.nn.functional as F
from scipy.optimize import linear_sum_assignment

from fs_eend_amd.stb import draw_order, stream_seed
from oracle import fixtures as FX
from tests import stb_ref as SR

REF = "/root/reference"
REF_MODEL = f"{REF}/FS-EEND/nnet/model/offl_tfm_enc_lstm_enc_dec.py"
FS_UTILS = f"{REF}/FS-EEND/train/utils/utils.py"
LS_UTILS = f"{REF}/LS-EEND/train/utils/utils.py"
FS_LOSS = f"{REF}/FS-EEND/train/utils/loss.py"
FS_STB = f"{REF}/FS-EEND/train/tfm_STB.py"
IN_SIZE = 345
COUNTER_GAIN = 16.0
THRESHOLDS = [0.5] + [round(0.5 + s * d / 100, 2) for d in range(1, 31) for s in (-1, 1)]     # 0.5 first, as the reference has it
VERBOSE = "-v" in sys.argv
FROM = next((int(a[7:]) for a in sys.argv[1:] if a.startswith("--from=")), None)      # start the seed search elsewhere
for _name in ("seed", "xseed", "sseed", "key", "frames"):                   # --seed=N etc.: try a loop case with other seeds
    for _a in sys.argv[1:]:
        if _a.startswith(f"--{_name}="):
            OVERRIDE = dict(globals().get("OVERRIDE", {}), **{_name: int(_a.split("=")[1])})
OVERRIDE = globals().get("OVERRIDE", {})
ONLY = {a for a in sys.argv[1:] if not a.startswith("-")}          # optional: the loop cases to (re)generate
CFG = dict(n_units=256, n_heads=4, n_layers=1, dropout=0.1)

# seed / xseed: the model's initialisation and the input; pseed_from: where the search for the perturbation seed starts (4000
# seeds from there; per seed only the thresholds that block 0's probabilities leave standing are run).  Under random weights a
# loop that keeps all the margins in every block, both policies and both precisions is rare: the values below are where the
# search ended (stb_loop_short_last after about 5400 seeds; for stb_loop_full_at_block_end seven (seed, xseed) pairs were tried and
# seed 38 / xseed 819 has one at perturbation seed 839), so a run of this script goes straight to them.  --seed= / --xseed= /
# --sseed= / --key= / --frames= / --from= try a case elsewhere.
LOOPS = [
    dict(name="stb_loop_short_last", blk=8, buf=24, frames=45, seed=30, xseed=811, sseed=5, key=3, pseed_from=5445),
    dict(name="stb_loop_full_at_block_end", blk=8, buf=20, frames=44, seed=38, xseed=819, sseed=6, key=4, pseed_from=839),
]


def reference_defs(path, names, ns, cls=None, cut=None):
    """Evaluate the named function definitions (module level, or methods of class `cls`) out of a reference file.  cut: keep a
    function's statements up to and including the first one for which cut(node) holds, then return `preds`."""
    tree = ast.parse(open(path).read())
    body = tree.body
    if cls is not None:
        body = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls).body
    for node in body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            if cut is not None:
                at = next(i for i, st in enumerate(node.body) if cut(st))
                node.body = node.body[:at + 1] + [ast.Return(value=ast.Name(id="preds", ctx=ast.Load()))]
                ast.fix_missing_locations(node)
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


def _np(t):
    return t.detach().cpu().numpy()


def helpers():
    ns = {"torch": torch, "F": F, "np": np, "Tensor": torch.Tensor, "linear_sum_assignment": linear_sum_assignment}
    find_best_perm, cal_cor, upd_buf = reference_defs(FS_UTILS, ["find_best_perm", "cal_cor", "upd_buf"], ns)
    ns_ls = dict(ns)
    (upd_buf_fifo,) = reference_defs(LS_UTILS, ["upd_buf_FIFO"], ns_ls)
    return ns, find_best_perm, cal_cor, upd_buf, upd_buf_fifo


def activity(rng, T, cols):
    out = np.zeros((T, cols), dtype=np.float32)
    for j in range(cols):
        t, on = 0, rng.random() < 0.5
        while t < T:
            run = int(rng.integers(2, 6))
            out[t:t + run, j] = rng.uniform(0.7, 0.98) if on else rng.uniform(0.02, 0.3)
            on, t = not on, t + run
    return out + rng.uniform(-0.01, 0.01, size=out.shape).astype(np.float32)


def gen_perm(find_best_perm):
    """(a): S tracked and c predicted columns zero-padded to max(S, c), c <= S + 1."""
    rng = np.random.default_rng(2024)
    arrays, pairs = {}, []
    for i, (T, S, c) in enumerate([(12, 2, 2), (20, 3, 3), (16, 2, 3), (24, 4, 3), (9, 1, 2), (30, 5, 5), (18, 3, 4)]):
        Sn = max(S, c)
        act = activity(rng, T, Sn)
        mix = rng.permutation(Sn)
        y = np.zeros((T, Sn), dtype=np.float32)
        y[:, :S] = act[:, :S]
        yp = np.zeros((T, Sn), dtype=np.float32)
        yp[:, :c] = np.clip(act[:, mix[:c]] + rng.normal(0, 0.05, size=(T, c)), 0.01, 0.99).astype(np.float32)
        perm = np.asarray(find_best_perm(torch.from_numpy(y), torch.from_numpy(yp)))
        mine, margin = SR.assign(SR.correlations(y, yp), S, c)
        assert margin >= 0.05, f"perm pair {i}: margin {margin}"
        arrays[f"y{i}"], arrays[f"yp{i}"], arrays[f"perm{i}"] = y, yp, perm.astype(np.int32)
        pairs.append(dict(T=T, S=S, c=c, margin=margin))
    p = FX.save_case("stb_perm", dict(kind="stb_perm", pairs=pairs), arrays)
    print(f"stb_perm: {len(pairs)} pairs -> {os.path.relpath(p)}")


class Recorder:
    """Stands for WeightedRandomSampler in upd_buf's namespace: stores the weights, returns the given indices."""

    def __init__(self):
        self.weights, self.give = None, None

    def __call__(self, weights, num_samples, replacement=True):
        assert not replacement
        self.weights = _np(weights).copy()
        picked = self.give(self.weights, num_samples)
        assert len(picked) == num_samples
        return iter(list(picked))


def gen_buffers(ns, upd_buf, upd_buf_fifo):
    """(b) and (c) on one set of inputs: 3 cases (T, S', buf_size), zero columns and an exactly zero entry included."""
    rng = np.random.default_rng(2025)
    rec = Recorder()
    ns["WeightedRandomSampler"] = rec
    kld, fifo, meta = {}, {}, []
    for i, (L, n, Sn, buf) in enumerate([(20, 8, 3, 20), (24, 5, 4, 24), (10, 4, 1, 12)]):
        x_buf = rng.normal(-3, 2, size=(L, 6)).astype(np.float32)
        x_i = rng.normal(-3, 2, size=(n, 6)).astype(np.float32)
        z_buf = activity(rng, L, Sn)
        y_i = activity(rng, n, Sn)
        if Sn > 2:
            z_buf[:, Sn - 1] = 0.0                              # a padded column of the buffer
            z_buf[3, 0] = 0.0                                   # p == 0 -> 1e-6
        give = sorted(rng.permutation(L + n)[:buf].tolist())
        rec.give = lambda w, m, give=give: rng.permutation(give).tolist()       # any order: upd_buf sorts
        args = [torch.from_numpy(a) for a in (x_buf, x_i, z_buf, y_i)]
        xb, yb = upd_buf(*[a.clone() for a in args], buf)
        kld.update({f"x_buf{i}": x_buf, f"x_i{i}": x_i, f"z_buf{i}": z_buf, f"y_i{i}": y_i, f"give{i}": np.asarray(give, dtype=np.int32),
                    f"weights{i}": rec.weights, f"x_out{i}": _np(xb), f"y_out{i}": _np(yb)})
        xf, yf = upd_buf_fifo(*[a.clone() for a in args], buf)
        fifo.update({f"x_buf{i}": x_buf, f"x_i{i}": x_i, f"z_buf{i}": z_buf, f"y_i{i}": y_i, f"x_out{i}": _np(xf), f"y_out{i}": _np(yf)})
        meta.append(dict(L=L, n=n, Sn=Sn, buf_size=buf))
    print("stb_kld ->", os.path.relpath(FX.save_case("stb_kld", dict(kind="stb_kld", cases=meta), kld)))
    print("stb_fifo ->", os.path.relpath(FX.save_case("stb_fifo", dict(kind="stb_fifo", cases=meta), fifo)))


class Unfit(Exception):
    pass


class LoopModel:
    """What the loop calls as self.model: the reference's own `test` with the case's threshold and the block's frame order, and
    a record of every call."""

    def __init__(self, m, ref_np, th, case):
        self.m, self.ref_np, self.th, self.case, self.calls = m, ref_np, th, case, []

    def test(self, src, ilens, th=None):
        k, T = len(self.calls), int(src[0].shape[0])
        order = draw_order(self.case["sseed"], self.case["key"], k, T).astype(np.int64)
        with torch.no_grad():
            emb = self.m.enc(src)
            attractors, probs = self.m.eda.estimate(emb[:, order, :])
            logits = torch.bmm(emb, attractors.transpose(1, 2))
        p = _np(probs[0]).astype(np.float64)
        below = np.nonzero(p < self.th)[0]
        count = int(below[0]) if below.size else 15
        if not 1 <= count <= 14 or np.abs(p - self.th).min() < 1e-2:
            raise Unfit(f"block {k}: count {count}, clearance {np.abs(p - self.th).min():.3e}")
        shuffle = self.ref_np.random.shuffle
        self.ref_np.random.shuffle = lambda a: a.__setitem__(slice(None), order)
        try:
            with torch.no_grad():
                active, emb_call, attr_call = self.m.test(src, ilens, th=self.th)
        finally:
            self.ref_np.random.shuffle = shuffle
        assert torch.equal(active[0], logits[0, :ilens[0], :count]), "the recorded logits are not what test() returned"
        self.calls.append(dict(order=order.astype(np.int32), logits=_np(logits[0]), probs=_np(probs[0]), count=count, xc=_np(src[0])))
        return active, emb_call, attr_call


class Self:
    pass


def run_loop(loop, ns_loop, m, ref_mod, x, case, th, policy, upd_buf, upd_buf_fifo, ns_utils, find_best_perm):
    """-> dict(calls, perms, sels, widths, emitted, gaps, margins)"""
    seed32 = stream_seed(case["sseed"], case["key"])
    model = LoopModel(m, ref_mod.np, th, case)
    perms, sels, margins, gaps, bufs = [], [], [], [], []

    def fbp(y, y_pred):
        perm = find_best_perm(y, y_pred)
        L, c, S = y.shape[0], model.calls[-1]["count"], perms_S[0]
        _, margin = SR.assign(SR.correlations(_np(y), _np(y_pred)), S, c)
        if abs(c - S) > 1:
            # two or more padding rows (c > S + 1) or all-zero predicted columns (c < S - 1): which of them goes where is arbitrary
            raise Unfit(f"count {c} against {S} tracked: more than one padding row or column, the reference's assignment is not unique")
        if margin < 0.05:
            raise Unfit(f"assignment margin {margin:.3e}")
        perms.append(np.asarray(perm).astype(np.int32))
        margins.append(margin)
        perms_S[0] = y.shape[1]
        return perm

    def sampler(weights, num_samples, replacement=True):
        k = len(model.calls) - 1
        keys = SR.race_keys(_np(weights).astype(np.float64), seed32, k)
        sel, gap = SR.race_select(keys, num_samples)
        if gap < 1e-3:
            raise Unfit(f"key gap {gap:.3e}")
        gaps.append(gap)
        return iter(sel.tolist())

    def upd(x_buf, x_i, z_buf, y_i, buf_size):
        T = x_buf.shape[0] + x_i.shape[0]
        if policy == "fifo":
            out = upd_buf_fifo(x_buf, x_i, z_buf, y_i, buf_size)
            sel = np.arange(T - buf_size, T)
        else:
            ns_utils["WeightedRandomSampler"] = sampler
            out = upd_buf(x_buf, x_i, z_buf, y_i, buf_size)
            keys = SR.race_keys(SR.weights(_np(torch.cat([z_buf, y_i])), z_buf.shape[1]), seed32, len(model.calls) - 1)
            sel, _ = SR.race_select(keys, buf_size)
            assert torch.equal(out[0], torch.cat([x_buf, x_i])[torch.from_numpy(sel)]), "float64 weights select other rows than the f32 ones"
        sels.append((len(model.calls) - 1, sel.astype(np.int32)))
        bufs.append((_np(out[0]), _np(out[1])))
        return out

    perms_S = [None]
    ns_loop.update(find_best_perm=fbp, upd_buf=upd)
    me = Self()
    me.blk_size, me.buf_size, me.model = case["blk"], case["buf"], model
    # block 0 sets the tracked width without an assignment: the loop's y_buf is test()'s output, so its width is the count
    orig_test = model.test

    def test(src, ilens, th=None):
        out = orig_test(src, ilens, th=th)
        if len(model.calls) == 1:
            perms_S[0] = model.calls[0]["count"]
        return out
    model.test = test
    labels = [torch.ones(x.shape[0], 1, dtype=x.dtype)]
    preds = loop(me, ([x], labels, ["rec"]), 0)
    widths = [model.calls[0]["count"]] + [len(p) for p in perms]
    return dict(calls=model.calls, perms=perms, sels=sels, widths=widths, emitted=_np(preds[0]), margins=margins, gaps=gaps, bufs=bufs)


def same_decisions(a, b):
    return ([c["count"] for c in a["calls"]] == [c["count"] for c in b["calls"]] and a["widths"] == b["widths"]
            and all(np.array_equal(p, q) for p, q in zip(a["perms"], b["perms"]))
            and all(k == l and np.array_equal(s, t) for (k, s), (l, t) in zip(a["sels"], b["sels"])))


def gen_loops(ns_utils, find_best_perm, upd_buf, upd_buf_fifo):
    spec = importlib.util.spec_from_file_location("ref_offl_eda", REF_MODEL)
    ref_mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_mod)
    ns_loss = {"torch": torch, "F": F, "np": np}
    pad_labels, pad_preds = reference_defs(FS_LOSS, ["pad_labels", "pad_preds"], ns_loss)
    ns_loop = {"torch": torch, "F": F, "np": np, "time": time, "pad_labels": pad_labels, "pad_preds": pad_preds}
    (loop,) = reference_defs(FS_STB, ["test_step"], ns_loop, cls="SpeakerDiarization",
                             cut=lambda st: isinstance(st, ast.For) and isinstance(st.target, ast.Tuple)
                             and [e.id for e in st.target.elts] == ["x", "clip_l"])
    for case in LOOPS:
        if ONLY and case["name"] not in ONLY:
            continue
        case = dict(case, **OVERRIDE)
        x = FX.make_src([case["frames"]], IN_SIZE, case["xseed"])[0]
        found = None
        first = case["pseed_from"] if FROM is None else FROM
        for pseed in range(first, first + 4000):
            torch.manual_seed(case["seed"])
            m = ref_mod.TransformerEDADiarization(n_speakers=None, in_size=IN_SIZE, **CFG).eval()
            FX.perturb_(m, pseed)
            with torch.no_grad():
                m.eda.counter.weight.mul_(COUNTER_GAIN)
            m64 = None
            # block 0 is the same call for every threshold: only thresholds that its probabilities leave standing are run
            xc0 = x[:case["blk"]] - x[:case["blk"]].mean(dim=0, keepdim=True)
            order0 = draw_order(case["sseed"], case["key"], 0, xc0.shape[0]).astype(np.int64)
            with torch.no_grad():
                p0 = _np(m.eda.estimate(m.enc([xc0])[:, order0, :])[1][0]).astype(np.float64)
            for th in THRESHOLDS:
                below = np.nonzero(p0 < th)[0]
                if not below.size or below[0] < 1 or np.abs(p0 - th).min() < 1e-2:
                    continue
                if m64 is None:
                    m64 = copy.deepcopy(m).double()
                try:
                    runs = {}
                    for policy in ("kld", "fifo"):
                        a = run_loop(loop, ns_loop, m, ref_mod, x, case, th, policy, upd_buf, upd_buf_fifo, ns_utils, find_best_perm)
                        b = run_loop(loop, ns_loop, m64, ref_mod, x.double(), case, th, policy, upd_buf, upd_buf_fifo, ns_utils,
                                     find_best_perm)
                        if not same_decisions(a, b):
                            raise Unfit("a decision differs between fp32 and float64")
                        a["gap64"] = float(np.abs(a["emitted"].astype(np.float64) - b["emitted"]).max())
                        runs[policy] = a
                    found = (pseed, th, runs, m)
                    break
                except Unfit as e:
                    if VERBOSE:
                        print(f"  {case['name']} pseed {pseed} th {th}: {e}")
            if found:
                break
        assert found, f"{case['name']}: no perturbation seed / threshold gives a loop with the margins"
        pseed, th, runs, m = found
        arrays, pol_meta = {}, {}
        for policy, r in runs.items():
            n_blocks = len(r["calls"])
            assert n_blocks == -(-case["frames"] // case["blk"]) and all(1 <= c["count"] <= 14 for c in r["calls"])
            for k, c in enumerate(r["calls"]):
                arrays[f"{policy}.order{k}"], arrays[f"{policy}.logits{k}"] = c["order"], c["logits"]
            for k, p in enumerate(r["perms"]):
                arrays[f"{policy}.perm{k + 1}"] = p
            for (k, s), (xb, yb) in zip(r["sels"], r["bufs"]):
                arrays[f"{policy}.sel{k}"], arrays[f"{policy}.x_buf{k}"], arrays[f"{policy}.y_buf{k}"] = s, xb, yb
            arrays[f"{policy}.emitted"] = r["emitted"]
            pol_meta[policy] = dict(counts=[c["count"] for c in r["calls"]], widths=r["widths"], select_blocks=[k for k, _ in r["sels"]],
                                    min_margin=min(r["margins"]), min_key_gap=min(r["gaps"]) if r["gaps"] else None, gap=r["gap64"],
                                    th_clearance=float(min(np.abs(c["probs"].astype(np.float64) - th).min() for c in r["calls"])))
            assert pol_meta[policy]["select_blocks"], "the buffer never overflows"
        meta = dict(kind="stb_loop", cfg=CFG, in_size=IN_SIZE, seed=case["seed"], pseed=pseed, xseed=case["xseed"], frames=case["frames"],
                    blk_size=case["blk"], buf_size=case["buf"], th=th, sseed=case["sseed"], key=case["key"], counter_gain=COUNTER_GAIN,
                    policies=pol_meta, checksums=FX.param_checksums(m.state_dict()), torch=torch.__version__)
        p = FX.save_case(case["name"], meta, arrays)
        print(f"{case['name']}: seed {case['seed']} xseed {case['xseed']} sseed {case['sseed']} key {case['key']} pseed {pseed} th {th} " + ", ".join(
            f"{k}: counts {v['counts']} widths {v['widths']} margin {v['min_margin']:.3f} key gap {v['min_key_gap']} gap {v['gap']:.2e}"
            for k, v in pol_meta.items()) + f" -> {os.path.relpath(p)} ({os.path.getsize(p) / 1024:.0f} KiB)")


def main():
    ns, find_best_perm, cal_cor, upd_buf, upd_buf_fifo = helpers()
    if not ONLY:
        gen_perm(find_best_perm)
        gen_buffers(ns, upd_buf, upd_buf_fifo)
    gen_loops(ns, find_best_perm, upd_buf, upd_buf_fifo)


if __name__ == "__main__":
    main()
