"""GPU: block-online EEND-EDA with a speaker-tracing buffer -- eend_lstm_orders_f32, the two kernels of csrc/stb.hip and
fs_eend_amd.stb.StbSession against the float64 restatement tests/stb_ref.py and the golden loop of the reference
(tools/gen_golden_stb.py).

Bars.  Centred rows and posteriors: 2 f32 ulp of the float64 value (the kernels compute both in float64 and round once).  Decisions
(perm, kept rows, widths) and copied buffer rows: equal; the cases are built or searched so that the reference alone shows an
assignment margin >= 1e-3 and a key gap >= 1e-9 relative, asserted first.  Logits of a batched pass against model.test at B = 1,
and the end-to-end golden: the project's conditioning rule, 2^13 times the reference's stored fp32-vs-float64 gap.
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle import fixtures as FX
from tests import eda_ref as ER
from tests import stb_cases as SC
from tests import stb_ref as SR

pytestmark = pytest.mark.gpu

RATIO = 2.0 ** 13
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGINS = os.path.join(ROOT, "profiles", "stb_parity_margins.json")
I32, I64, F32 = torch.int32, torch.int64, torch.float32


def _ulp_ok(got, want, n=2):
    """|got - want| <= n f32 ulp of want, elementwise; got f32 array, want float64 array."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    tol = n * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    bad = np.abs(got - want) > tol
    return not bad.any(), float((np.abs(got - want) / tol).max()) if got.size else 0.0


def _np(t):
    return t.detach().cpu().numpy()


# ---- eend_lstm_orders_f32 ----

def _lstm(ops, G, order, W):
    B, T = G.shape[0], G.shape[1]
    hT, cT = (torch.empty(B, 256, dtype=F32, device=G.device) for _ in range(2))
    h_all = torch.empty(B, T, 256, dtype=F32, device=G.device)
    ops.lstm(G, order, None, W, None, None, hT, cT, h_all, B, T)
    return hT, cT, h_all


def test_lstm_orders(hip_lib, dev):
    from fs_eend_amd import ops
    g = torch.Generator().manual_seed(5)
    B, T = 3, 37
    G = torch.randn(B, T, 1024, generator=g).to(dev)
    W = (torch.randn(1024, 256, generator=g) * 0.08).to(dev)
    orders = torch.stack([torch.randperm(T, generator=g) for _ in range(B)]).to(dev, I32)
    assert not torch.equal(orders[0], orders[1]) and not torch.equal(orders[1], orders[2])
    got = _lstm(ops, G, orders, W)
    for b in range(B):
        alone = _lstm(ops, G[b:b + 1].contiguous(), orders[b].contiguous(), W)
        for a, e in zip(got, alone):
            assert torch.equal(a[b:b + 1], e)
    shared = orders[1:2].expand(B, T).contiguous()
    for a, e in zip(_lstm(ops, G, shared, W), _lstm(ops, G, orders[1].contiguous(), W)):
        assert torch.equal(a, e)
    # the 2-D form is refused where it means nothing
    with pytest.raises(ops._lib.EendHipError):
        ops.lstm(G, orders[:2].contiguous(), None, W, None, None, got[0], got[1], None, B, T)


# ---- the kernels of csrc/stb.hip, one launch at a time ----

class _Launch:
    """Device tensors and the descriptor table of one launch over `cases` (all of one T, F, buf_size, blk_size)."""

    def __init__(self, dev, cases):
        from fs_eend_amd import ops
        c0 = cases[0]
        self.B, self.T, self.F, self.buf, self.blk = len(cases), c0["T"], c0["F"], c0["buf_size"], c0["blk_size"]
        self.keep = []
        rows = []
        self.x_dst, self.y_dst, self.width, self.y_out = [], [], [], []
        for c in cases:
            assert (c["T"], c["F"], c["buf_size"], c["blk_size"]) == (self.T, self.F, self.buf, self.blk)
            x_buf = torch.from_numpy(c["x_buf"]).to(dev) if c["L"] else torch.zeros(1, self.F, device=dev)
            y_buf = torch.from_numpy(c["y_buf"]).to(dev) if c["L"] else torch.zeros(1, 15, device=dev)
            x_i = torch.from_numpy(c["x_i"]).to(dev)
            cap = min(self.T, self.buf)
            # the destination halves are allocated at exactly the rows the contract names, with a guard row behind them
            x_dst = torch.full((cap + 1, self.F), 777.0, device=dev)
            y_dst = torch.full((cap + 1, 15), 777.0, device=dev)
            width = torch.tensor([c["S"]], dtype=I32, device=dev)
            y_out = torch.full((c["n"] + 1, 15), 777.0, device=dev)
            self.keep += [x_buf, y_buf, x_i]
            self.x_dst.append(x_dst); self.y_dst.append(y_dst); self.width.append(width); self.y_out.append(y_out)
            rows.append([x_buf.data_ptr(), c["L"], x_i.data_ptr(), c["n"], y_buf.data_ptr(), x_dst.data_ptr(), y_dst.data_ptr(),
                         width.data_ptr(), y_out.data_ptr(), c["k"], c["seed32"], 0])
        self.desc = torch.tensor(rows, dtype=I64).to(dev)
        assert self.desc.shape == (self.B, ops.STB_DESC_WORDS)

    def center(self):
        from fs_eend_amd import ops
        out = torch.empty(self.B, self.T, self.F, dtype=F32, device=self.desc.device)
        ops.stb_center(self.desc, out, self.buf, self.blk)
        return out

    def track(self, logits, counts, xc, policy):
        from fs_eend_amd import ops
        dev = self.desc.device
        perm = torch.full((self.B, 15), -7, dtype=I32, device=dev)
        sel = torch.full((self.B, self.buf), -1, dtype=I32, device=dev)
        ops.stb_track(logits, torch.tensor(counts, dtype=I32, device=dev), xc, self.desc, perm, sel, self.buf, self.blk,
                      ops.STB_POLICIES[policy])
        torch.cuda.synchronize()
        return perm, sel


def _center_case(L, n, seed, F=345):
    rng = np.random.default_rng(seed)
    return dict(L=L, n=n, T=L + n, F=F, buf_size=24, blk_size=8, S=0, k=0, seed32=0,
                x_buf=rng.normal(-3, 2, size=(L, F)).astype(np.float32), x_i=rng.normal(-3, 2, size=(n, F)).astype(np.float32),
                y_buf=np.zeros((L, 15), dtype=np.float32))


@pytest.mark.parametrize("L", [0, 1, 24])
@pytest.mark.parametrize("n", [1, 8])
def test_center(hip_lib, dev, L, n):
    case = _center_case(L, n, 100 * L + n)
    got = _Launch(dev, [case]).center()
    torch.cuda.synchronize()
    want = SR.center(case["x_buf"], case["x_i"])
    ok, worst = _ulp_ok(_np(got[0]), want)
    print(f"centre L={L} n={n}: worst {worst:.3f} of the 2-ulp bar")
    assert ok, worst
    # the same sequence among batch mates of the same T (another split of buffer and block where there is one): the same bits
    mates = [_center_case(L, n, 7), case, _center_case(L + n - 1, 1, 8) if L + n - 1 <= 24 and L + n > 1 else _center_case(L, n, 9)]
    among = _Launch(dev, mates).center()
    torch.cuda.synchronize()
    assert torch.equal(among[1], got[0])
    ok, _ = _ulp_ok(_np(among[2]), SR.center(mates[2]["x_buf"], mates[2]["x_i"]))
    assert ok


def _check_track(dev, case, policy):
    want, st = SC.reference(case, policy)
    # on the reference alone: no decision of this case sits on a rounding
    assert want["margin"] >= 1e-3, f"{case['name']}: assignment margin {want['margin']:.3e}"
    assert want["gap"] >= 1e-9, f"{case['name']}: key gap {want['gap']:.3e}"
    la = _Launch(dev, [case])
    xc = torch.from_numpy(want["xc"]).to(dev)[None].contiguous()
    logits = torch.from_numpy(case["logits"]).to(dev)[None].contiguous()
    perm, sel = la.track(logits, [case["c"]], xc, policy)
    Sn, n, T, cap = want["width"], case["n"], case["T"], min(case["T"], case["buf_size"])
    assert int(la.width[0].item()) == Sn
    assert _np(perm[0])[:Sn].tolist() == want["perm"][:Sn].tolist(), (case["name"], _np(perm[0]), want["perm"], case["match"])
    assert _np(perm[0])[Sn:].tolist() == list(range(Sn, 15))
    assert _np(sel[0])[:cap].tolist() == want["sel"].tolist() and (_np(sel[0])[cap:] == -1).all()
    y = _np(la.y_out[0])
    assert (y[n:] == 777.0).all()                                        # nothing behind the block
    assert (y[:n, Sn:] == 0).all()
    exact = np.zeros((n, 15))
    src = np.asarray(case["logits"], dtype=np.float64)[case["L"]:]
    for r in range(Sn):
        if want["perm"][r] < want["count"]:
            exact[:, r] = 1.0 / (1.0 + np.exp(-src[:, want["perm"][r]]))
    ok, worst = _ulp_ok(y[:n], exact)
    assert ok, f"{case['name']}: posteriors {worst:.3f} of the 2-ulp bar"
    # the new buffer: the kept rows in time order, raw features (block 0: the centred ones) bit for bit
    xb, yb = _np(la.x_dst[0]), _np(la.y_dst[0])
    assert (xb[cap:] == 777.0).all() and (yb[cap:] == 777.0).all()
    assert np.array_equal(xb[:cap], st.x_buf)
    old = want["sel"] < case["L"]
    assert np.array_equal(yb[:cap][old], st.y_buf[old])                  # rows that were in the buffer are copied
    ok, worst = _ulp_ok(yb[:cap], st.y_buf.astype(np.float64), n=1)      # the block's rows: the same f32 up to a double rounding
    assert ok, worst
    return want


@pytest.mark.parametrize("policy", ["kld", "fifo"])
@pytest.mark.parametrize("case", SC.CASES, ids=[c[0] for c in SC.CASES])
def test_track_synthetic(hip_lib, dev, case, policy):
    c = SC.build(*case, F=345 if case[0] in ("buf20_blk8", "block0") else SC.F_SMALL)
    _check_track(dev, c, policy)


def test_track_batch_mates(hip_lib, dev):
    """Sequences of one launch with different widths, counts, block indices and seeds: each as the reference has it alone."""
    cases = [SC.build("buf20_blk8", 20, 8, 3, 3, 20, 8, 13), SC.build("c_S_plus_3_tie_rule", 20, 8, 2, 5, 20, 8, 9),
             SC.build("c15_S14", 20, 8, 14, 15, 20, 8, 5)]
    wants = [SC.reference(c, "kld") for c in cases]
    la = _Launch(dev, cases)
    xc = torch.stack([torch.from_numpy(w[0]["xc"]) for w in wants]).to(dev)
    logits = torch.stack([torch.from_numpy(c["logits"]) for c in cases]).to(dev)
    perm, sel = la.track(logits, [c["c"] for c in cases], xc, "kld")
    for b, (c, (w, st)) in enumerate(zip(cases, wants)):
        assert w["margin"] >= 1e-3 and w["gap"] >= 1e-9
        assert int(la.width[b].item()) == w["width"]
        assert _np(perm[b])[:w["width"]].tolist() == w["perm"][:w["width"]].tolist()
        assert _np(sel[b])[:20].tolist() == w["sel"].tolist()
        assert np.array_equal(_np(la.x_dst[b])[:20], st.x_buf)


# ---- the session ----

@pytest.fixture(scope="module")
def mirror(dev):
    meta, _ = FX.load_case("eda_T37")                                   # the one-layer golden model of the offline baseline
    return meta, ER.build_mirror(meta).to(dev)


def _fixed_orders(key, k, T):
    return np.random.default_rng([99, key, k, T]).permutation(T)


def _drive(sess, plan, dev):
    """plan {name: (feats (frames, F) cpu, first step, frames per push, key)} -> per name (slot, [blocks of last_blocks], [outputs])."""
    slots, fed, blocks, outs = {}, {}, {}, {}
    step = 0
    while len(fed) < len(plan) or any(fed[nm] is not None for nm in fed):
        push, flush = {}, []
        for nm, (x, first, per, key) in plan.items():
            if step < first or fed.get(nm, 0) is None:
                continue
            if nm not in slots:
                slots[nm], fed[nm], blocks[nm], outs[nm] = sess.open(key=key), 0, [], []
            a = fed[nm]
            push[slots[nm]] = x[a:a + per].to(dev)
            fed[nm] = a + per
            if fed[nm] >= x.shape[0]:
                flush.append(slots[nm])
                fed[nm] = None
        got = sess.step(push, flush)
        by_slot = {s: nm for nm, s in slots.items()}
        for blk in sess.last_blocks:
            blocks[by_slot[blk["slot"]]].append(blk)
        for s, (y, w) in got.items():
            outs[by_slot[s]].append((y, w))
        step += 1
    return slots, blocks, outs


def _streams(F=345):
    g = torch.Generator().manual_seed(4242)
    return {"a": torch.randn(45, F, generator=g) * 2 - 3, "b": torch.randn(8, F, generator=g) * 2 - 3,
            "c": torch.randn(21, F, generator=g) * 2 - 3}


@pytest.mark.parametrize("policy", ["kld", "fifo"])
def test_session_against_loop(hip_lib, dev, mirror, policy):
    from fs_eend_amd.stb import StbSession, stream_seed
    meta, model = mirror
    xs = _streams()
    sess = StbSession(model, 3, buf_size=24, blk_size=8, th=meta["th"], policy=policy, seed=11, orders=_fixed_orders, debug=True)
    plan = {"a": (xs["a"], 0, 16, 5), "b": (xs["b"], 1, 8, 6), "c": (xs["c"], 2, 3, 7)}
    slots, blocks, outs = _drive(sess, plan, dev)
    bar = RATIO * meta["gaps"]["logits"]["rel"]
    report = {}
    for nm, (x, _, _, key) in plan.items():
        frames = x.shape[0]
        assert [b["n"] for b in blocks[nm]] == [8] * (frames // 8) + ([frames % 8] if frames % 8 else [])
        assert stream_seed(11, key) == SR.stream_seed(11, key)
        st = SR.State(345)
        margins, gaps, worst_logit = [], [], 0.0
        for k, blk in enumerate(blocks[nm]):
            assert blk["k"] == k and blk["L"] == st.x_buf.shape[0]
            x_i = x[sum(b["n"] for b in blocks[nm][:k]):][:blk["n"]].numpy()
            assert np.array_equal(_np(blk["x_i"]), x_i)
            assert np.array_equal(_np(blk["order"]), _fixed_orders(key, k, blk["T"]).astype(np.int32))
            xc = _np(blk["xc"])
            ok, worst = _ulp_ok(xc, SR.center(st.x_buf, x_i))
            assert ok, f"{nm} block {k}: centred rows {worst:.3f} of the 2-ulp bar"
            # the batched pass gives the logits of model.test at B = 1 on the same rows and order, within the bar of test_eda_gpu.py
            model.test([blk["xc"]], [blk["T"]], th=meta["th"], order=_np(blk["order"]))
            alone = _np(model.last_logits[0]).astype(np.float64)
            err = float(np.abs(_np(blk["logits"]) - alone).max() / np.sqrt((alone ** 2).mean()))
            worst_logit = max(worst_logit, err)
            assert err <= bar, f"{nm} block {k}: logits {err:.3e} > {bar:.3e}"
            count = int(blk["count"].item())
            want = SR.track(st, x_i, xc, _np(blk["logits"]), count, 24, policy, SR.stream_seed(11, key))
            assert want["margin"] >= 1e-3 and want["gap"] >= 1e-9, (nm, k, want["margin"], want["gap"])
            margins.append(want["margin"]); gaps.append(want["gap"])
            Sn, cap = want["width"], min(blk["T"], 24)
            assert _np(blk["perm"])[:Sn].tolist() == want["perm"][:Sn].tolist()
            assert _np(blk["sel"])[:cap].tolist() == want["sel"].tolist()
            ok, worst = _ulp_ok(_np(blk["y"]), want["y"].astype(np.float64), n=1)
            assert ok and (_np(blk["y"])[:, Sn:] == 0).all()
        xb, yb, w = sess.buffer(slots[nm])
        assert int(w.item()) == st.S and np.array_equal(_np(xb), st.x_buf)
        ok, _ = _ulp_ok(_np(yb), st.y_buf.astype(np.float64), n=1)
        assert ok
        res = sess.result(slots[nm])
        assert tuple(res.shape) == (frames, st.S) and sess.frames(slots[nm]) == frames
        assert torch.equal(res, torch.cat([y for y, _ in outs[nm]], dim=0)[:, :st.S])
        fin = [m for m in margins if np.isfinite(m)]
        report[nm] = dict(blocks=len(blocks[nm]), width=st.S, logits_err=worst_logit, logits_bar=bar,
                          min_margin=min(fin) if fin else None, min_gap=min([g for g in gaps if np.isfinite(g)], default=None))
        print(nm, report[nm])
    for s in slots.values():
        sess.close(s)


def _run_alone(model, th, x, key, per, dev, slots=1, others=None):
    from fs_eend_amd.stb import StbSession
    sess = StbSession(model, slots, buf_size=24, blk_size=8, th=th, policy="kld", seed=3, orders=_fixed_orders, debug=bool(others))          # the debug outputs change no result
    plan = dict(others or {})
    plan["me"] = (x, 1 if others else 0, per, key)
    slot, _, _ = _drive(sess, plan, dev)
    s = slot["me"]
    xb, yb, w = sess.buffer(s)
    return sess.result(s).clone(), xb.clone(), yb.clone(), w.clone()


def test_independence(hip_lib, dev, mirror):
    """A stream alone and among three others in other phases: torch.equal results and buffers."""
    meta, model = mirror
    xs = _streams()
    g = torch.Generator().manual_seed(17)
    alone = _run_alone(model, meta["th"], xs["a"], 21, 8, dev)
    others = {"o1": (torch.randn(61, 345, generator=g) * 2 - 3, 0, 16, 1), "o2": (torch.randn(30, 345, generator=g) * 2 - 3, 0, 8, 2),
              "o3": (torch.randn(19, 345, generator=g) * 2 - 3, 2, 5, 3)}
    among = _run_alone(model, meta["th"], xs["a"], 21, 8, dev, slots=4, others=others)
    for a, e in zip(among, alone):
        assert a.shape == e.shape and torch.equal(a, e)


def _record(case, rows):
    data = {}
    if os.path.exists(MARGINS):
        with open(MARGINS) as f:
            data = json.load(f)
    data[case] = rows
    with open(MARGINS, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


@pytest.mark.parametrize("policy", ["kld", "fifo"])
@pytest.mark.parametrize("name", ["stb_loop_short_last", "stb_loop_full_at_block_end"])
def test_golden_loop_end_to_end(hip_lib, dev, name, policy):
    """The reference's own loop on its own model (tools/gen_golden_stb.py) against one stream of a session: every decision equal,
    the emitted posteriors within 2^13 times the reference's stored fp32-vs-float64 gap."""
    from fs_eend_amd.stb import StbSession
    meta, arr = FX.load_case(name)
    pm = meta["policies"][policy]
    model = ER.build_mirror(meta).to(dev)
    x = FX.make_src([meta["frames"]], meta["in_size"], meta["xseed"])[0].to(dev)
    sess = StbSession(model, 1, buf_size=meta["buf_size"], blk_size=meta["blk_size"], th=meta["th"], policy=policy, seed=meta["sseed"], debug=True)
    s = sess.open(key=meta["key"])
    out = sess.step({s: x}, flush=[s])
    blocks = sess.last_blocks
    assert len(blocks) == len(pm["counts"]) and tuple(out[s][0].shape) == (meta["frames"], 15)
    assert [int(b["count"].item()) for b in blocks] == pm["counts"]
    widths = []
    for k, b in enumerate(blocks):
        assert np.array_equal(_np(b["order"]), arr[f"{policy}.order{k}"])
        width = pm["widths"][k]
        widths.append(width)
        if k:
            assert _np(b["perm"])[:width].tolist() == arr[f"{policy}.perm{k}"].tolist(), k
        cap = min(b["T"], meta["buf_size"])
        want_sel = arr[f"{policy}.sel{k}"].tolist() if k in pm["select_blocks"] else list(range(b["T"]))
        assert _np(b["sel"])[:cap].tolist() == want_sel, k
        assert not _np(b["y"])[:, width:].any()
    res = sess.result(s)
    want = arr[f"{policy}.emitted"]
    assert tuple(res.shape) == want.shape and int(sess.width[s].item()) == pm["widths"][-1]
    err, bar = float(np.abs(_np(res).astype(np.float64) - want).max()), RATIO * pm["gap"]
    print(f"{name} {policy}: err {err:.3e} bar {bar:.3e} err/bar {err / bar:.3f}")
    _record(f"{name}.{policy}", dict(err=err, bar=bar, ratio=err / bar, min_margin=pm["min_margin"], min_key_gap=pm["min_key_gap"],
                                     th_clearance=pm["th_clearance"]))
    assert err <= bar


def test_errors_change_nothing(hip_lib, dev, mirror):
    from fs_eend_amd.lib import EendHipError
    from fs_eend_amd.multistream import SlotError
    from fs_eend_amd.stb import StbSession
    meta, model = mirror
    with pytest.raises(ValueError):
        StbSession(model, 2, buf_size=8, blk_size=9)
    with pytest.raises(ValueError):
        StbSession(model, 2, policy="lifo")
    with pytest.raises(EendHipError):
        StbSession(model, 2, buf_size=4000, blk_size=100)               # buf_size + blk_size > 4096
    with pytest.raises(SlotError):
        StbSession(model, 0)
    sess = StbSession(model, 2, buf_size=24, blk_size=8, th=meta["th"], seed=1, orders=_fixed_orders)
    s = sess.open()
    x = (torch.randn(5, 345) * 2 - 3).to(dev)
    sess.step({s: x})

    def snapshot():
        return (list(sess.state), list(sess.k), list(sess.L), list(sess.half), [sess._held(i) for i in range(2)],
                [len(o) for o in sess.out])
    before = snapshot()
    good = (torch.randn(3, 345) * 2 - 3).to(dev)
    with pytest.raises(EendHipError):
        sess.step({s: torch.zeros(3, 345)})                             # a CPU tensor
    with pytest.raises(EendHipError):
        sess.step({s: torch.zeros(3, 344, device=dev)})                 # a wrong feature width
    with pytest.raises(SlotError):
        sess.step({1: good})                                            # a free slot
    with pytest.raises(SlotError):
        sess.step({s: good, 1: good})                                   # ... and nothing of the good one is taken
    with pytest.raises(SlotError):
        sess.step({s: good}, flush=[s, s])
    with pytest.raises(SlotError):
        sess.step({7: good})
    with pytest.raises(SlotError):
        sess.result(1)
    assert snapshot() == before
    out = sess.step({s: good}, flush=[s])                               # 8 frames: one block, then the slot is done
    assert list(out) == [s] and tuple(out[s][0].shape) == (8, 15)
    before = snapshot()
    with pytest.raises(SlotError):
        sess.step({s: good})                                            # a flushed slot
    with pytest.raises(SlotError):
        sess.step(flush=[s])
    assert snapshot() == before
    assert tuple(sess.result(s).shape)[0] == 8
    assert sess.last_blocks == []                                       # kept only under debug=True
    sess.close(s)
    with pytest.raises(SlotError):
        sess.close(s)
    # an `orders` callable that fails on a block of this very call (the second of two): raised before anything is taken
    def bad_orders(key, k, T):
        return np.zeros(T, dtype=np.int64) if k == 1 else _fixed_orders(key, k, T)
    sess = StbSession(model, 2, buf_size=24, blk_size=8, th=meta["th"], seed=1, orders=bad_orders)
    s = sess.open()
    sess.step({s: x})
    before = snapshot()
    with pytest.raises(ValueError):
        sess.step({s: (torch.randn(11, 345) * 2 - 3).to(dev)})          # 16 frames: blocks 0 and 1
    assert snapshot() == before
    out = sess.step({s: good})                                          # 8 frames: block 0 alone still runs
    assert tuple(out[s][0].shape) == (8, 15) and sess.k[s] == 1
