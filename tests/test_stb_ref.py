"""CPU: tests/stb_ref.py, the float64 restatement the GPU tests of the speaker-tracing buffer compare against, checked itself
against what the reference's own functions produced (tools/gen_golden_stb.py -> tests/golden/stb_*.npz), the exponential race
against exact inclusion probabilities, the synthetic cases of the GPU tests for their margins, and the host side of the two C-ABI
entries."""
import itertools

import numpy as np
import pytest

from oracle import fixtures as FX
from tests import stb_cases as SC
from tests import stb_ref as SR

# both shapes of the whole-loop golden, by name: a missing file fails here instead of dropping its tests
LOOPS = ["stb_loop_short_last", "stb_loop_full_at_block_end"]


def test_find_best_perm_golden():
    meta, arr = FX.load_case("stb_perm")
    assert len(meta["pairs"]) >= 6
    kinds = set()
    for i, pair in enumerate(meta["pairs"]):
        y, yp = arr[f"y{i}"], arr[f"yp{i}"]
        S, c = pair["S"], pair["c"]
        assert c <= S + 1 and y.shape[1] == max(S, c)
        assert not y[:, S:].any() and not yp[:, c:].any()                # the padding is where the pair says
        perm, margin = SR.assign(SR.correlations(y, yp), S, c)
        assert margin >= 0.05
        assert perm.tolist() == arr[f"perm{i}"].tolist(), i
        kinds.add(np.sign(c - S))
    assert kinds == {-1, 0, 1}                                           # padded columns on either side, and none


def test_upd_buf_golden():
    meta, arr = FX.load_case("stb_kld")
    for i, case in enumerate(meta["cases"]):
        z = np.concatenate([arr[f"z_buf{i}"], arr[f"y_i{i}"]], axis=0)
        w = SR.weights(z, case["Sn"])
        want = arr[f"weights{i}"].astype(np.float64)                     # the reference's are f32 and normalised to sum 1
        assert np.abs(w / w.sum() - want).max() <= 1e-5 * want.max()
        x, y = SR.keep_rows(arr[f"x_buf{i}"], arr[f"x_i{i}"], arr[f"z_buf{i}"], arr[f"y_i{i}"], arr[f"give{i}"])
        assert np.array_equal(x, arr[f"x_out{i}"]) and np.array_equal(y, arr[f"y_out{i}"])


def test_upd_buf_fifo_golden():
    meta, arr = FX.load_case("stb_fifo")
    for i, case in enumerate(meta["cases"]):
        z = np.concatenate([arr[f"z_buf{i}"], arr[f"y_i{i}"]], axis=0)
        sel, _ = SR.select_rows(z, case["Sn"], case["buf_size"], "fifo", 0, 0)
        x, y = SR.keep_rows(arr[f"x_buf{i}"], arr[f"x_i{i}"], arr[f"z_buf{i}"], arr[f"y_i{i}"], sel)
        assert np.array_equal(x, arr[f"x_out{i}"]) and np.array_equal(y, arr[f"y_out{i}"])


@pytest.mark.parametrize("policy", ["kld", "fifo"])
@pytest.mark.parametrize("name", LOOPS)
def test_loop_golden(name, policy):
    """The loop fed the STORED logits and counts: perms, selections, widths equal, emitted rows within 1e-6; the buffers after a
    selection hold the same rows (block 0's centred rows and the posteriors are the reference's fp32 ones there: 4e-6 and 1e-6)."""
    from fs_eend_amd.stb import draw_order
    meta, arr = FX.load_case(name)
    pm = meta["policies"][policy]
    x = FX.make_src([meta["frames"]], meta["in_size"], meta["xseed"])[0].numpy()
    seen = []

    def model_test(xc, order):
        k = len(seen)
        assert np.array_equal(order, arr[f"{policy}.order{k}"])
        seen.append(xc)
        return arr[f"{policy}.logits{k}"], pm["counts"][k]

    st = SR.State(meta["in_size"])
    blocks = []
    for s in range(0, x.shape[0], meta["blk_size"]):                     # stb_ref.loop, with a look at the buffers on the way
        x_i = x[s:s + meta["blk_size"]]
        xc = SR.center(st.x_buf, x_i)
        logits, count = model_test(xc, draw_order(meta["sseed"], meta["key"], st.k, xc.shape[0]))
        out = SR.track(st, x_i, xc, logits, count, meta["buf_size"], policy, SR.stream_seed(meta["sseed"], meta["key"]))
        blocks.append(out)
        k = len(blocks) - 1
        if k in pm["select_blocks"]:
            assert out["sel"].tolist() == arr[f"{policy}.sel{k}"].tolist(), k
            assert np.abs(st.x_buf - arr[f"{policy}.x_buf{k}"]).max() <= 4e-6
            assert np.abs(st.y_buf[:, :out["width"]] - arr[f"{policy}.y_buf{k}"]).max() <= 1e-6
        else:
            assert out["sel"].tolist() == list(range(xc.shape[0]))
        if k:
            assert abs(count - blocks[k - 1]["width"]) <= 1           # at most one padding row or column: the answer is unique
            assert out["perm"][:out["width"]].tolist() == arr[f"{policy}.perm{k}"].tolist(), k
            assert out["margin"] >= 0.05
    assert [b["width"] for b in blocks] == pm["widths"]
    assert len(pm["select_blocks"]) >= 1
    width = max(pm["widths"])
    emitted = np.concatenate([b["y"][:, :width] for b in blocks], axis=0)
    assert emitted.shape == arr[f"{policy}.emitted"].shape
    assert np.abs(emitted - arr[f"{policy}.emitted"]).max() <= 1e-6
    # the same through stb_ref.loop
    seen.clear()
    blocks2, result, st2 = SR.loop(model_test, x, meta["blk_size"], meta["buf_size"], policy, SR.stream_seed(meta["sseed"], meta["key"]),
                                   lambda k, T: draw_order(meta["sseed"], meta["key"], k, T))
    assert np.array_equal(result, emitted) and np.array_equal(st2.x_buf, st.x_buf)


def _inclusion(w, m):
    """Exact inclusion probabilities of drawing m of len(w) items without replacement, each draw proportional to w."""
    p = np.zeros(len(w))
    for seq in itertools.permutations(range(len(w)), m):
        left, pr = float(np.sum(w)), 1.0
        for i in seq:
            pr *= w[i] / left
            left -= w[i]
        p[list(seq)] += pr
    return p


def test_race_draw_distribution():
    """Keep-counts of the race over 2000 seeds against the exact inclusion probabilities of successive draws, within 4 standard
    errors (the race keeps item i with exactly that probability: the largest of w_i / E_i, E_i unit exponentials)."""
    w = np.array([0.05, 0.4, 1.0, 1.7, 0.2, 3.0])
    m, N = 3, 2000
    want = _inclusion(w, m)
    assert abs(want.sum() - m) < 1e-12
    counts = np.zeros(len(w))
    for seed in range(N):
        sel, _ = SR.race_select(SR.race_keys(w, SR.stream_seed(seed, 0), seed % 7), m)
        assert len(sel) == m and sorted(set(sel.tolist())) == sel.tolist()
        counts[sel] += 1
    se = np.sqrt(N * want * (1 - want))
    print("z-scores", np.round((counts - N * want) / se, 2))
    assert (np.abs(counts - N * want) <= 4 * se).all()


def test_race_ties_and_hash():
    sel, gap = SR.race_select(np.array([1.0, 2.0, 2.0, 2.0, 0.5]), 2)
    assert sel.tolist() == [1, 2] and gap == 0.0                         # equal keys: the lower index wins
    sel, _ = SR.race_select(np.array([3.0, 3.0, 3.0]), 1)
    assert sel.tolist() == [0]
    # the mixing function as the header states it, on fixed points of its own definition
    assert SR.mix(0) == 0 and SR.mix(1) == 0x514E28B7 and SR.mix(0xFFFFFFFF) == 0x81F16F39
    hs = {SR.draw_hash(9, k, t) for k in range(4) for t in range(64)}
    assert len(hs) == 256 and all(0 <= h < 2 ** 32 for h in hs)
    from fs_eend_amd import stb
    assert all(stb._mix(v) == SR.mix(v) for v in (0, 1, 12345, 0xDEADBEEF))
    assert stb.stream_seed(3, 2 ** 40 + 17) == SR.stream_seed(3, 2 ** 40 + 17)
    o = stb.draw_order(1, 2, 3, 37)
    assert o.dtype == np.int32 and sorted(o.tolist()) == list(range(37)) and np.array_equal(o, stb.draw_order(1, 2, 3, 37))
    assert not np.array_equal(o, stb.draw_order(1, 2, 4, 37)) and not np.array_equal(o, stb.draw_order(1, 3, 3, 37))


def test_zero_tracked_and_zero_rows():
    assert SR.weights(np.zeros((5, 0)), 0).tolist() == [1.0] * 5         # no tracked speaker: uniform
    w = SR.weights(np.array([[0.0, 0.0], [0.5, 0.5], [1.0, 0.0]]), 2)
    assert w[0] == 1e-6 and w[1] == 1e-6 and abs(w[2] - (np.log(2.0) + 1e-6 * np.log(2e-6))) < 1e-12
    st = SR.State(3)
    out = SR.track(st, np.ones((4, 3), np.float32), np.zeros((4, 3)), np.zeros((4, 15)), 0, 8, "kld", 1)
    assert out["width"] == 0 and not out["y"].any() and st.S == 0
    out = SR.track(st, np.ones((2, 3), np.float32), np.zeros((6, 3)), np.zeros((6, 15)), 0, 8, "kld", 1)
    assert out["width"] == 0 and st.x_buf.shape[0] == 6


@pytest.mark.parametrize("case", SC.CASES, ids=[c[0] for c in SC.CASES])
def test_synthetic_cases_have_margins(case):
    """What test_stb_gpu.py::test_track_synthetic asserts first, checked without a device; the tie-rule case is one."""
    c = SC.build(*case)
    for policy in ("kld", "fifo"):
        want, st = SC.reference(c, policy)
        assert want["margin"] >= 1e-3 and want["gap"] >= 1e-9
        assert st.x_buf.shape[0] == min(c["T"], c["buf_size"])
        Sn = want["width"]
        if c["L"] and c["S"] and c["c"]:
            inv = {int(r): q for q, r in enumerate(c["match"]) if q < c["c"] and r < c["S"]}
            assert all(want["perm"][r] == q for r, q in inv.items()), (want["perm"], c["match"])
        if c["name"] == "c_S_plus_3_tie_rule":
            rest = [q for q in range(Sn) if q not in want["perm"][:c["S"]].tolist()]
            assert want["perm"][c["S"]:Sn].tolist() == rest == sorted(rest)


def test_cabi_domain(hip_lib):
    """EEND_EINVAL before any launch (fake non-NULL pointers are never dereferenced on these paths)."""
    L = hip_lib
    p = 4096
    ok = dict(B=1, T=28, F=345, buf=20, blk=8)
    bad = [dict(ok, buf=4000, blk=100), dict(ok, F=513), dict(ok, F=0), dict(ok, T=0), dict(ok, T=29), dict(ok, blk=0),
           dict(ok, buf=7), dict(ok, B=0)]
    for a in bad:
        assert L.eend_stb_center_f32(p, p, a["B"], a["T"], a["F"], a["buf"], a["blk"], None) == -1, a
        assert L.eend_stb_track_f32(p, p, p, p, None, None, a["B"], a["T"], a["F"], a["buf"], a["blk"], 0, None) == -1, a
    assert L.eend_stb_track_f32(p, p, p, p, None, None, 1, 28, 345, 20, 8, 2, None) == -1          # an unknown policy
    assert L.eend_stb_center_f32(None, p, 1, 28, 345, 20, 8, None) == -1
    assert L.eend_stb_track_f32(None, p, p, p, None, None, 1, 28, 345, 20, 8, 0, None) == -1
    assert L.eend_lstm_orders_f32(p, 37, None, p, None, None, p, p, None, 3, 37, 256, None) == -1  # no order
    assert L.eend_lstm_orders_f32(None, 37, p, p, None, None, p, p, None, 3, 37, 256, None) == -1  # no G
    assert L.eend_lstm_orders_f32(p, 36, p, p, None, None, p, p, None, 3, 37, 256, None) == -1     # g_rows < T
    assert L.eend_abi_version() == 5                                                               # the entries are additive


def test_session_refuses_without_gpu():
    import torch
    from fs_eend_amd.eda_model import TransformerEDADiarization
    from fs_eend_amd.lib import EendHipError
    from fs_eend_amd.stb import StbSession
    m = TransformerEDADiarization(n_speakers=None, in_size=345, n_units=256, n_heads=4, n_layers=1, dropout=0.1).eval()
    with pytest.raises(ValueError):
        StbSession(m, 2, buf_size=8, blk_size=9)
    with pytest.raises(ValueError):
        StbSession(m, 2, policy="lifo")
    with pytest.raises(EendHipError):
        StbSession(m, 2)                                                 # a CPU model: no fallback
    with pytest.raises(EendHipError):
        StbSession(torch.nn.Linear(2, 2), 2)
