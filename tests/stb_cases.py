"""The synthetic single-block cases of tests/test_stb_gpu.py::test_track_synthetic, built in numpy so that their margins can be
checked without a device (tests/test_stb_ref.py::test_synthetic_cases_have_margins): for every case the reference alone must show an
assignment margin >= 1e-3 and, where rows are drawn, a key gap >= 1e-9 relative -- a decision that flips on rounding would let a
test hide a wrong correlation or weight.

A case's buffer columns are smoothed on/off activity patterns; predicted column q carries the pattern of tracked column match[q]
plus noise (columns beyond the tracked ones carry patterns of their own), so the best assignment is `match` by a wide margin."""
import numpy as np

from tests import stb_ref as SR

F_SMALL = 7

# name, L, n, S, c, buf_size, blk_size, seed; policies are crossed in the test
CASES = [
    ("block0", 0, 8, 0, 3, 24, 8, 1),
    ("block0_n1", 0, 1, 0, 2, 24, 8, 2),
    ("c0", 16, 8, 2, 0, 24, 8, 3),
    ("none_tracked_select", 20, 8, 0, 0, 20, 8, 4),
    ("c15_S14", 24, 8, 14, 15, 24, 8, 5),
    ("c15_S15", 24, 8, 15, 15, 24, 8, 6),
    ("c_below_S", 24, 8, 4, 2, 24, 8, 7),
    ("c_S_plus_1", 24, 8, 2, 3, 24, 8, 8),
    ("c_S_plus_3_tie_rule", 24, 8, 2, 5, 24, 8, 9),
    ("constant_column", 24, 8, 3, 3, 24, 8, 10),
    ("T_eq_buf_appends", 16, 8, 3, 3, 24, 8, 11),
    ("T_buf_plus_1_selects_n1", 24, 1, 3, 4, 24, 8, 12),
    ("buf20_blk8", 20, 8, 3, 3, 20, 8, 13),
    ("buf20_blk8_short", 20, 3, 2, 4, 20, 8, 14),
    ("L1000_n100", 1000, 100, 3, 4, 1000, 100, 15),
]


def _patterns(rng, T, cols):
    """(T, cols) logits of on/off activity in runs of a few rows, amplitude about +-3."""
    out = np.zeros((T, cols))
    for j in range(cols):
        t = 0
        on = rng.random() < 0.5
        while t < T:
            run = int(rng.integers(2, 7))
            out[t:t + run, j] = (3.0 if on else -3.0) + rng.normal(0, 0.3, size=min(run, T - t))
            on = not on
            t += run
    return out


def build(name, L, n, S, c, buf_size, blk_size, seed, F=F_SMALL):
    """-> dict of the kernel's inputs: x_buf (L, F), x_i (n, F), y_buf (L, 15), logits (T, 15), S, c, k, seed32, match."""
    rng = np.random.default_rng(1000 + seed)
    T = L + n
    act = _patterns(rng, T, 15)
    match = rng.permutation(max(S, c))                       # predicted column q carries tracked column match[q]'s pattern
    y_buf = np.zeros((L, 15), dtype=np.float32)
    y_buf[:, :S] = SR.sigmoid32(act[:L, :S] + rng.normal(0, 0.2, size=(L, S)))
    if name == "constant_column":
        y_buf[:, 1] = 0.5
    logits = rng.normal(0, 1, size=(T, 15)).astype(np.float32)          # columns beyond c are never read as posteriors
    for q in range(c):
        logits[:, q] = (act[:, match[q]] + rng.normal(0, 0.4, size=T)).astype(np.float32)
    x_buf = rng.normal(-3, 2, size=(L, F)).astype(np.float32)
    x_i = rng.normal(-3, 2, size=(n, F)).astype(np.float32)
    return dict(name=name, L=L, n=n, T=T, S=S, c=c, buf_size=buf_size, blk_size=blk_size, F=F, x_buf=x_buf, x_i=x_i, y_buf=y_buf,
                logits=logits, k=0 if L == 0 else 1 + seed, seed32=SR.stream_seed(seed, 40 + seed), match=match)


def reference(case, policy):
    """stb_ref.track on a case -> (its dict, the state after the block)."""
    st = SR.State(case["F"])
    st.x_buf, st.y_buf, st.S, st.k = case["x_buf"].copy(), case["y_buf"].copy(), case["S"], case["k"]
    xc = SR.center(case["x_buf"], case["x_i"]).astype(np.float32)
    out = SR.track(st, case["x_i"], xc, case["logits"], case["c"], case["buf_size"], policy, case["seed32"])
    out["xc"] = xc
    return out, st
