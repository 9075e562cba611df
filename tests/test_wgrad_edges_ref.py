"""CPU: the constructions of tests/wgrad_edge_ref.py really pin the weight-gradient kernels -- the int64 reference agrees with a
float64 matmul and with the conv1d autograd weight gradient, every operand of the GPU tables passes the exactness guard (so that a
correct kernel is bit-exact whatever its summation order), and every one-step mistake of the mutation table changes the reference at
every shape of tests/test_wgrad_edges.py it can act on.  A kernel making one of these mistakes could therefore not pass there.

Where a shape gives a mistake nothing to act on (a boundary row with one split, a second k-tile with K = 128, ...) the mutation returns
None; each test asserts that this happens only where the shape explains it, and that every mutation acts on at least one shape."""
import ctypes

import pytest
import torch
import torch.nn.functional as Fn

from tests import wgrad_edge_ref as E

GEMM = E.gemm_cases()
CONV = E.conv_cases()


def _operands(c, seed=0):
    return E.ints((c["M"], c["N"]), 1000 + seed + c["M"]), E.ints((c["M"], c["K"]), 2000 + seed + c["M"])


def test_int64_reference_equals_float64_matmul():
    for M, N, K in ((1, 128, 128), (97, 128, 256), (1000, 256, 128)):
        dy, x = E.ints((M, N), M), E.ints((M, K), M + 1)
        assert torch.equal(E.ref_dw(dy, x).double(), dy.double().t() @ x.double())
        assert torch.equal(E.ref_db(dy).double(), dy.double().sum(0))
        w = torch.randint(0, 3, (M,))
        assert torch.equal(E.ref_dw(dy, x, w).double(), (dy.double() * w[:, None]).t() @ x.double())


@pytest.mark.parametrize("nseq,Tp,ilens,ktaps,pad", [(2, 64, (64, 30), 19, 9), (3, 64, (1, 0, 9), 19, 9), (2, 128, (127, 65), 7, 3)])
def test_conv_reference_equals_conv1d_autograd(nseq, Tp, ilens, ktaps, pad):
    cout, cin = 8, 16
    dy, x = E.ints((nseq * Tp, cout), 3), E.ints((nseq * Tp, cin), 4)
    got = E.ref_conv_dw(dy, x, nseq, Tp, ilens, ktaps, pad)
    mask = (torch.arange(Tp)[None, :] < torch.tensor(ilens)[:, None]).double()[..., None]
    w = torch.zeros(cout, cin, ktaps, dtype=torch.float64, requires_grad=True)
    y = Fn.conv1d((x.double().view(nseq, Tp, cin) * mask).transpose(1, 2), w, padding=pad).transpose(1, 2)
    (y * dy.double().view(nseq, Tp, cout)).sum().backward()
    assert torch.equal(got.double(), w.grad)
    assert torch.equal(E.ref_conv_dw(dy, x, nseq, Tp, ilens, ktaps, pad, via_f64=True), got)


def test_blocked_layout_round_trip():
    for M in (16, 17, 31, 208):
        t = E.ints((M, 64), M).to(E.BF16)
        b = E.to_blocked(t, pad=3.0)
        assert b.shape == ((M + 15) // 16 * 16, 64) and torch.equal(E.from_blocked(b, M), t)
        assert (E.from_blocked(b, b.shape[0])[M:] == 3).all()
        # element (m, u) at ((m >> 4) * (F / 32) + (u >> 5)) * 512 + (m & 15) * 32 + (u & 31)
        m, u = M - 1, 37
        assert b.view(-1)[((m >> 4) * 2 + (u >> 5)) * 512 + (m & 15) * 32 + (u & 31)] == t[m, u]


def test_plan_table_matches_the_planner(hip_lib):
    """the plan classes of the tables are those of plan_wgrad on a 256-CU device (the query falls back to 256 without a device)"""
    def plan(M, N, K, cin, ws, bias):
        t, n, m = ctypes.c_int(), ctypes.c_int(), ctypes.c_long()
        assert hip_lib.eend_wgrad_plan(M, N, K, cin, ws, bias, ctypes.byref(t), ctypes.byref(n), ctypes.byref(m)) == 0
        return t.value, n.value, m.value
    for c in GEMM:
        for bias in (0, 1):
            assert plan(c["M"], c["N"], c["K"], 0, E.ws_floats(c, bias), bias) == (c["tile"], c["nsplit"], c["mps"]), E.case_id(c)
    for c in CONV:
        K = c["ktaps"] * 256
        assert plan(c["nseq"] * c["Tp"], 256, K, 256, c["cap"] * 256 * K, 0) == (c["tile"], c["nsplit"], c["mps"]), E.conv_id(c)
    t = ctypes.c_int()
    assert hip_lib.eend_wgrad_plan(100, 128, 128, 0, 128 * 128 - 1, 0, ctypes.byref(t), ctypes.byref(t), ctypes.byref(ctypes.c_long())) == -1
    assert hip_lib.eend_wgrad_plan(100, 64, 128, 0, 1 << 20, 0, ctypes.byref(t), ctypes.byref(t), ctypes.byref(ctypes.c_long())) == -1


def test_plan_classes_cover_what_they_claim():
    ns = {c["nsplit"] for c in GEMM if c["group"] == "b"}
    assert {n % 4 for n in ns} == {0, 1, 2, 3}                              # every remainder of the 4-way tile reduction
    assert any(n % 8 == 0 for n in ns) and any(n % 8 for n in ns)           # both block -> split mappings
    assert any(n < 16 for n in ns) and 16 in ns and any(n > 64 for n in ns)   # both bias reductions, and the 64-stride loop
    assert {c["tile"] for c in GEMM} == {128, 256}
    stages = {(c["M"] + 31) // 32 for c in GEMM if c["group"] == "a"}
    assert {1, 2, 3, 4, 5, 9, 32} <= stages                                 # under the 3-stage prologue, the ring, ring wraps
    for c in CONV:
        assert c["Tp"] % 64 == 0 and all(0 <= i <= c["Tp"] for i in c["ilens"]) and len(c["ilens"]) == c["nseq"]
    assert any(c["mps"] < c["Tp"] for c in CONV) and any(c["tile"] == 256 and c["nseq"] * c["Tp"] >= 16384 for c in CONV)


@pytest.mark.parametrize("c", GEMM, ids=E.case_id)
def test_row_mutations_are_detected(c):
    dy, x = _operands(c)
    E.assert_exact(dy, x)
    assert (dy[0] != 0).all() and (dy[-1] != 0).all() and (x != 0).all()
    dw, db = E.ref_dw(dy, x), E.ref_db(dy)
    M, ns, mps = c["M"], c["nsplit"], c["mps"]
    assert E.split_bounds(M, ns, mps)[-1][1] == M and (ns - 1) * mps < M
    for name in E.ROW_MUTATIONS:
        w = E.row_weights(name, M, ns, mps)
        if w is None:
            assert (name == "boundary_row_in_both_splits" and ns == 1) or (name == "drop_rows_beyond_last_64" and M % 64 == 0), name
            continue
        rows = (w != 1).nonzero().flatten()
        assert len(rows) > 0
        d = E.ref_dw(dy[rows], x[rows], w[rows] - 1)                          # (linear in w: the change alone, cheap)
        assert d.ne(0).any(), name
        if M <= 1000:
            assert torch.equal(E.ref_dw(dy, x, w), dw + d) and not torch.equal(E.ref_dw(dy, x, w), dw)
        # the bias sees the same rows.  A doubled and a dropped row may cancel in a column sum, never in all 128+ columns at once
        assert E.ref_db(dy[rows], w[rows] - 1).ne(0).any(), name
    # output-side mistakes
    tile, N, K = c["tile"], c["N"], c["K"]
    assert not torch.equal(E.transposed_output(dw), dw)
    t = E.tiles_k_major(dw, tile)
    assert (t is None) == (N // tile < 2 or K // tile < 2) and (t is None or not torch.equal(t, dw))
    b = E.bias_from_ktile1_too(db, K, tile)
    assert (b is None) == (K // tile < 2) and (b is None or not torch.equal(b, db))
    b = E.bias_first_ntile_only(db, N, tile)
    assert (b is None) == (N // tile < 2) and (b is None or not torch.equal(b, db))


def test_every_mutation_acts_somewhere():
    for name in E.ROW_MUTATIONS:
        assert sum(E.row_weights(name, c["M"], c["nsplit"], c["mps"]) is not None for c in GEMM) >= 20, name
    assert sum(c["N"] // c["tile"] >= 2 and c["K"] // c["tile"] >= 2 for c in GEMM) >= 2          # k-major tiles
    assert sum(c["K"] // c["tile"] >= 2 for c in GEMM) >= 4 and sum(c["N"] // c["tile"] >= 2 for c in GEMM) >= 4


@pytest.mark.parametrize("c", [c for c in CONV if c["nseq"] * c["Tp"] < 16384], ids=E.conv_id)
def test_conv_mutations_are_detected(c):
    nseq, Tp, il, kt, pad, mps = c["nseq"], c["Tp"], c["ilens"], c["ktaps"], c["pad"], c["mps"]
    M = nseq * Tp
    dy, x = E.ints((M, 256), 7 + M), E.ints((M, 256), 8 + M)
    E.assert_exact(dy, x)
    want = E.ref_conv_dw(dy, x, nseq, Tp, il, kt, pad)
    v0, s0 = E.conv_pairs(nseq, Tp, il, kt, pad)
    for name in E.CONV_MUTATIONS:
        v, s = E.conv_pairs(nseq, Tp, il, kt, pad, name, mps)
        acts = bool((v != v0).any() or ((s != s0) & v).any())
        assert torch.equal(E.ref_conv_dw(dy, x, nseq, Tp, il, kt, pad, name, mps), want) != acts, name
        if name == "conv_tap_off_by_one":
            assert acts == any(i > 0 for i in il)
        if name == "conv_ignore_ilen":
            assert acts == any(i < Tp for i in il)
        if name == "conv_neighbour_sequence":
            assert acts == any(i > 0 for i in il[1:])
        if name == "conv_clip_at_split_start":                                # a split begins inside a sequence, below its ilen + pad
            mid = any(g % Tp and g % Tp - pad < il[g // Tp] for g in range(0, M, mps))
            assert acts == mid


def test_every_conv_mutation_acts_in_every_geometry():
    geo = {}
    for c in CONV:
        v0, s0 = E.conv_pairs(c["nseq"], c["Tp"], c["ilens"], c["ktaps"], c["pad"])
        for name in E.CONV_MUTATIONS:
            v, s = E.conv_pairs(c["nseq"], c["Tp"], c["ilens"], c["ktaps"], c["pad"], name, c["mps"])
            k = (c["nseq"], c["Tp"], c["ktaps"], c["mps"], name)
            geo[k] = geo.get(k, False) or bool((v != v0).any() or ((s != s0) & v).any())
    for k, acts in geo.items():
        if k[4] == "conv_clip_at_split_start" and k[3] % k[1] == 0:
            assert not acts                                                    # every split begins with a sequence: nothing to clip
        else:
            assert acts, k


@pytest.mark.parametrize("M", [64, 4096])
def test_tie_construction_pins_round_to_nearest_even(M):
    x = E.as16(E.tie_x(M, 128, M), E.F16)
    dy = E.ints((M, 128), M + 1, vals=(-1, 0, 1))
    rne, tr = x.to(E.BF16), E.trunc_bf16(x)
    E.assert_exact(dy, rne.to(E.I64))
    for v, want in ((257, 256), (259, 260), (1028, 1024), (1036, 1040), (2047, 2048), (511, 512)):
        assert torch.tensor(float(v), dtype=E.F16).to(E.BF16).item() == want
    assert (rne.double() != tr.double()).any(1).all()                          # every row rounds up somewhere
    assert not torch.equal(E.ref_dw(dy, rne.to(E.I64)), E.ref_dw(dy, tr.to(E.I64)))
    assert not torch.equal(E.ref_dw(dy, rne.to(E.I64)), E.ref_dw(dy, x.to(E.I64)))    # and the rounding itself shows


@pytest.mark.parametrize("e", E.DY_SCALE_EXPONENTS)
def test_scaled_dy_is_exact_in_bf16(e):
    """integer * 2^e is exact in bf16 and in the f32 sums.  An f16 detour keeps 2^-20 only as a subnormal (k * 2^-24: a flushing path
    loses it) and loses 2^-40 on every path, which is why the GPU test runs both."""
    dy = E.ints((1000, 128), 5).double() * 2.0 ** e
    assert torch.equal(dy.to(E.BF16).double(), dy)
    x = E.ints((1000, 128), 6)
    a = dy.t() @ x.double()
    assert torch.equal(a.float().double(), a) and torch.equal(a, E.ref_dw(E.ints((1000, 128), 5), x).double() * 2.0 ** e)
    through_f16 = dy.to(E.F16).double()
    if e == -20:
        assert (through_f16.abs() < 6.2e-5).all()                              # below f16's smallest normal 2^-14
    else:
        assert (through_f16 == 0).all() and a.ne(0).any()


def test_blocked_padding_rows_would_show():
    """non-zero padding rows of a blocked operand meeting non-zero rows behind M of the other operand change dW"""
    for M in (193, 207):
        dy, x = E.ints((M, 128), M), E.ints((M, 128), M + 1)
        pad_x, pad_dy = E.ints((16, 128), 9, vals=(3, -3)), E.ints((16, 128), 10, vals=(3, -3))
        full = E.ref_dw(E.pad_rows(dy, pad_dy), E.pad_rows(x, pad_x))
        assert not torch.equal(full, E.ref_dw(dy, x))
        assert not torch.equal(E.ref_db(E.pad_rows(dy, pad_dy)), E.ref_db(dy))
    assert E.pad_rows(E.ints((208, 8), 1), E.ints((16, 8), 2)).shape[0] == 208


def test_colsum_table():
    for M, N, ns in E.COLSUM_CASES:
        assert N % 8 == 0 and min(ns, 1024, (M + 63) // 64) == ns
    assert {ns for _, _, ns in E.COLSUM_CASES} == {1, 15, 16, 17, 65}
