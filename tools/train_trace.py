"""The training counterpart of tools/model_trace.py: for fixed-seed runs of the two native training steps (train.FsTrainStep,
train_ls.LsTrainStep), every call into libeend_hip.so in order -- the entry's name and its scalar arguments (the int / float / long
positions of lib.PROTOTYPES; a pointer shows only as `*` or, when NULL, `0`: addresses are not recorded) -- followed by the SHA-256 of
the step's results: flat.grads after the backward, flat.params / flat.m / flat.v after the optimiser, the loss slots, the BatchNorm
running statistics and, after forward(fused_loss=False), the head's logits and normalised attractors.  Every hashed buffer is written
in full by the step (flat.* are zero-filled at construction, bf.loss is torch.zeros(4), head_l2dot fills all B*T*C rows), so no
partial view is needed.  Two trees of the Python layer behave the same exactly when their listings are identical:
    python tools/train_trace.py > a.txt;  (in the other tree, this file copied in)  python tools/train_trace.py > b.txt;  diff a.txt b.txt
Only public classes, methods and the class attributes the tests monkeypatch are used, so the file runs unchanged in an older tree.
The mirrors and inputs are those of the smallest committed training goldens (fs_train_small, ls_train_small).
A listing is about 7000 lines; `python tools/train_trace.py --digest < a.txt` (no GPU needed) condenses one to a line per case -- the
number of calls, the SHA-256 of the call lines and the SHA-256 of the result lines -- which is what profiles/ keeps: two listings are
identical exactly when their digests are."""
import ctypes, hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if "--digest" in sys.argv:
    name, parts = None, {}

    def flush():
        if name is not None:
            print(f"{name}\n  calls {len(parts['c']):4d} {hashlib.sha256(''.join(parts['c']).encode()).hexdigest()}\n"
                  f"  results {len(parts['r']):2d} {hashlib.sha256(''.join(parts['r']).encode()).hexdigest()}")

    for line in sys.stdin:
        if line.startswith("== "):
            flush()
            name, parts = line.rstrip("\n"), dict(c=[], r=[])
        elif line.strip():
            parts["c" if line.startswith("  eend_") else "r"].append(line)
    flush()
    sys.exit(0)

import torch

from fs_eend_amd import lib
from fs_eend_amd import train as TR
from fs_eend_amd import train_ls as TL
from fs_eend_amd.trainer import prepare_labels
from oracle import fixtures as FX
from tests.helpers import build_fs_mirror, build_ls_mirror

DEV = "cuda"
SCALARS = (ctypes.c_int, ctypes.c_float, ctypes.c_long)
calls = []


def _wrap(L, name, argtypes):
    fn = getattr(L, name)

    def traced(*args):
        shown = []
        for a, ty in zip(args, argtypes):
            if ty in SCALARS:
                shown.append(repr(float(a)) if ty is ctypes.c_float else str(int(a)))
            else:
                shown.append("0" if a is None else "*")
        calls.append(f"  {name}({', '.join(shown)})")
        return fn(*args)

    setattr(L, name, traced)


L = lib.load()
for protos in (lib.PROTOTYPES, lib.LONG_PROTOTYPES):
    for name, argtypes in protos.items():
        _wrap(L, name, argtypes)


def case(name, fn):
    """Run fn with the call list empty; print the calls it made, then the hashes of the tensors it returned (a dict, in order)."""
    calls.clear()
    out = fn()
    torch.cuda.synchronize()
    print(f"== {name}")
    print("\n".join(calls))
    for path, t in out.items():
        raw = t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()
        print(f"  {path:28s} {tuple(t.shape)} {hashlib.sha256(raw).hexdigest()}")
    sys.stdout.flush()


FMETA, _ = FX.load_case("fs_train_small")
LMETA, _ = FX.load_case("ls_train_small")
META = dict(fs=FMETA, ls=LMETA)
CHUNK = LMETA["cfg"]["recurrent_chunk_size"]


def engine(kind, dropout=0.0):
    """A fresh mirror of the golden's parameters and its training step (the caller prepares the operand copies, as step() does)."""
    meta = dict(META[kind], cfg=dict(META[kind]["cfg"], dropout=dropout))
    m = (build_fs_mirror if kind == "fs" else build_ls_mirror)(meta).to(DEV).train()
    eng = (TR.FsTrainStep if kind == "fs" else TL.LsTrainStep)(m, warmup=meta["warm"], grad_clip=meta["clip"], drop_seed=1234)
    return eng


def batch(kind, lengths=None, nspk=None):
    meta = META[kind]
    lengths, nspk = lengths or meta["lengths"], nspk or meta["nspk"]
    feats = [f.to(DEV) for f in FX.make_src(lengths, meta["in_size"], meta["xseed"])]
    labels = prepare_labels([l.to(DEV) for l in FX.make_labels(lengths, nspk, meta["lseed"])], lengths)
    return feats, labels, list(lengths)


def snap(out, tag, eng, bf=None, grads_only=False):
    """Copies of what the step has produced so far (later steps overwrite the buffers in place)."""
    fl = eng.flat
    out[f"{tag}.grads"] = fl.grads.clone()
    if not grads_only:
        out[f"{tag}.params"], out[f"{tag}.m"], out[f"{tag}.v"] = fl.params.clone(), fl.m.clone(), fl.v.clone()
        out[f"{tag}.gsumsq"] = eng.gsumsq.clone()
    if bf is not None:
        out[f"{tag}.loss"] = bf.loss.clone()
    for k, b in eng.model.named_buffers():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            out[f"{tag}.{k}"] = b.clone()


def split_step(out, tag, eng, feats, labels, ilens, **fw):
    """step() in its parts, so that the gradients are seen before the optimiser."""
    bf = eng.forward(feats, labels, ilens, **fw)
    eng.backward(bf)
    snap(out, tag + ".bwd", eng, bf, grads_only=True)
    eng.all_reduce_grads()
    eng.optimizer_step()
    snap(out, tag + ".opt", eng)
    return bf


def steps(kind, n=2, dropout=0.0, lengths=None, nspk=None, ilens=None, pit=False):
    def run():
        eng = engine(kind, dropout)
        feats, labels, il = batch(kind, lengths, nspk)
        out = {}
        for s in range(n):
            r = eng.step(feats, labels, ilens or il, pit=pit)
            snap(out, f"s{s}", eng)
            out[f"s{s}.bce"], out[f"s{s}.emb"] = r["bce"].clone(), r["emb"].clone()
        return out
    return run


def split(kind, p_drop=0.0, **fw):
    def run():
        eng = engine(kind, p_drop)
        eng.prep_weights()
        feats, labels, il = batch(kind)
        out = {}
        for s in range(2):
            split_step(out, f"s{s}", eng, feats, labels, il, **fw)
        return out
    return run


def unfused(kind, emb_loss_grad):
    def run():
        eng = engine(kind, 0.1)
        eng.prep_weights()
        feats, labels, il = batch(kind)
        bf = eng.forward(feats, labels, il, fused_loss=False)
        B, T, Tp, C = bf.shape
        dl = (torch.randn(B, T, C, generator=torch.Generator().manual_seed(5)) * 1e-3).to(DEV)
        eng.backward(bf, dlogits=dl, emb_loss_grad=emb_loss_grad)
        out = dict(logits_full=bf.logits_full.clone(), attr_n=bf.attr_n.clone())
        snap(out, "bwd", eng, bf, grads_only=True)
        return out
    return run


def accumulate(kind):
    def run():
        eng = engine(kind, 0.1)
        eng.prep_weights()
        feats, labels, il = batch(kind)
        out = {}
        for i, sel in enumerate(([0, 1], [2])):
            bf = eng.forward([feats[j] for j in sel], [labels[j] for j in sel], [il[j] for j in sel])
            eng.backward(bf)
            eng.accumulate_grads(i, 2)
            snap(out, f"micro{i}", eng, bf, grads_only=True)
        eng.all_reduce_grads()
        eng.optimizer_step()
        snap(out, "opt", eng)
        return out
    return run


def resume(kind):
    def run():
        eng = engine(kind, 0.1)
        feats, labels, il = batch(kind)
        eng.step(feats, labels, il)
        st, sd = eng.optimizer_state(), {k: v.clone() for k, v in eng.model.state_dict().items()}
        eng2 = engine(kind, 0.1)
        eng2.model.load_state_dict(sd)
        eng2.load_optimizer_state(st)
        eng2.prep_weights()
        out = {}
        split_step(out, "resumed", eng2, feats, labels, il)
        return out
    return run


def patched(obj, attr, value, fn):
    def run():
        old = getattr(obj, attr)
        setattr(obj, attr, value)
        try:
            return fn()
        finally:
            setattr(obj, attr, old)
    return run


for kind in ("fs", "ls"):
    K = kind.upper()
    case(f"{K} two steps, dropout 0 (ragged labels: the zero-pad branch)", steps(kind))
    case(f"{K} two steps, dropout 0.1", steps(kind, dropout=0.1))
    case(f"{K} two steps in parts, dropout 0.1 (gradients before the optimiser)", split(kind, 0.1))
    case(f"{K} forward(dropout=False) on a dropout 0.1 mirror", split(kind, 0.1, dropout=False))
    case(f"{K} one step, pit=True", steps(kind, n=1, dropout=0.1, pit=True))
    case(f"{K} equal lengths and columns (the stacked-labels branch)", steps(kind, n=1, dropout=0.1, lengths=[200, 200], nspk=[2, 2]))
    case(f"{K} fused_loss=False, emb_loss_grad 0.5", unfused(kind, 0.5))
    case(f"{K} fused_loss=False, emb_loss_grad 0.0", unfused(kind, 0.0))
    case(f"{K} gacc_stream_min_rows = 0", patched(TR.TrainStepBase, "gacc_stream_min_rows", 0, split(kind, 0.1)))
    case(f"{K} accumulate_grads over two micro-batches", accumulate(kind))
    case(f"{K} optimizer_state -> load_optimizer_state into a fresh engine, one more step", resume(kind))

case("FS ilens shorter than the features", steps("fs", n=1, dropout=0.1, ilens=[190, 160, 100]))
case("FS attn_train_fused = False", patched(TR.TrainStepBase, "attn_train_fused", False, split("fs", 0.1)))
case("LS proj_stream_min_rows = 0 and gacc_stream_min_rows = 0",
     patched(TL.LsTrainStep, "proj_stream_min_rows", 0, patched(TR.TrainStepBase, "gacc_stream_min_rows", 0, split("ls", 0.1))))
case("LS MACARON_FUSED = 0", patched(TL, "MACARON_FUSED", 0, split("ls", 0.1)))
case(f"LS T = {2 * CHUNK + CHUNK // 2} (not a multiple of the retention chunk {CHUNK}: Tv != T)",
     steps("ls", n=1, dropout=0.1, lengths=[2 * CHUNK + CHUNK // 2, 170], nspk=[2, 3]))
case("FS T = 520 (Tp > 512: qt / kt and the two-kernel attention)", steps("fs", n=1, dropout=0.1, lengths=[520], nspk=[2]))
