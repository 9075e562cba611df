"""CPU: the constructions of tests/linear_edge_ref.py do what tests/test_linear_edges.py relies on.  Both exactness guards hold for every
tabled case, every row that decides a LayerNorm / L2-norm case has non-zero variance / norm (reference() asserts it), every mutation
changes the reference of every case it applies to, every route of every entry is covered by a case, and -- the route query being
host arithmetic -- every case already takes the route it was written for here, without a GPU."""
import os
import re

import pytest
import torch

from tests import linear_edge_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = E.all_cases()


@pytest.fixture(scope="module")
def references():
    """name -> buffers of every tabled case; computing them runs guard (a) on the operands and guard (b) on the 2-byte outputs"""
    return {E.case_id(c): E.reference(c) for c in CASES}


def test_guards_hold_for_the_whole_table(references):
    assert len(references) == len(CASES) > 300
    for c in CASES:
        ref, exact = references[E.case_id(c)], E.exact_outputs(c)
        assert ref, E.case_id(c)
        for name, buf in ref.items():
            live = ~buf.isnan()
            assert live.any() and float(buf[live].abs().max()) < E.LIMIT
            if name in exact:                            # linear outputs are integers (half-integers under alpha = 0.5)
                assert torch.equal(buf[live] * 2, (buf[live] * 2).round()), (E.case_id(c), name)
                if exact[name] in (E.F16, E.BF16):
                    lim = 256 if exact[name] == E.BF16 else 2048
                    assert float(buf[live].abs().max()) <= lim, (E.case_id(c), name)
            else:
                assert E.tolerance(c, name) in E.TOL


def test_guard_rows_and_columns_are_nan(references):
    for c in CASES:
        if E.FAMILY[c["entry"]] == "heads":
            continue
        for name, buf in references[E.case_id(c)].items():
            assert buf[-E.GUARD_ROWS:].isnan().all() and not buf[:-E.GUARD_ROWS, 0].isnan().any(), (E.case_id(c), name)
            if c.get("ldo") and c["ldo"] > (c["N"] // 2 if E.FAMILY[c["entry"]] == "glu" else c["N"]):
                assert buf[:, -1].isnan().all(), E.case_id(c)


def test_the_guards_can_fail():
    big = torch.full((2, 4096), 64.0)
    with pytest.raises(AssertionError):
        E.assert_exact(big, big)                                         # 64 * 64 * 4096 = 2^24
    with pytest.raises(AssertionError):
        E.assert_exact(torch.ones(2, 8), torch.tensor([[1.0] * 7 + [0.0]]))   # a zero operand
    with pytest.raises(AssertionError):
        E.as16(torch.tensor([2049.0]), E.F16)
    with pytest.raises(AssertionError):
        E.as16(torch.tensor([257.0]), E.BF16)
    E.as16(torch.tensor([2048.0, -1023.5, float("nan")]), E.F16), E.as16(torch.tensor([256.0]), E.BF16)
    with pytest.raises(AssertionError):
        E.layer_norm(torch.ones(2, 256), None, None, 1e-5)


@pytest.mark.parametrize("mut", E.MUTATIONS)
def test_every_mutation_changes_every_case_it_applies_to(references, mut):
    n = 0
    for c in CASES:
        if not E.applies(mut, c):
            continue
        n += 1
        ref, bad = references[E.case_id(c)], E.reference(c, mut)
        assert set(bad) == set(ref)
        changed = [name for name in ref if not E.same(bad[name], ref[name])]
        assert changed, f"{mut} leaves {E.case_id(c)} unchanged"
        if mut in ("ktile_dropped", "ktile_doubled", "rows_shifted", "tail_row_from_clamp"):
            assert len(changed) == len(ref), f"{mut}: {E.case_id(c)} keeps {set(ref) - set(changed)}"
    assert n >= 10, (mut, n)


def test_a_mutation_is_outside_every_tolerance(references):
    """the outputs behind LayerNorm / L2 norm / Swish are compared with a tolerance: the mistakes still show through it"""
    for c in CASES:
        for mut in ("ktile_dropped", "rows_shifted"):
            if not E.applies(mut, c):
                continue
            ref, bad = references[E.case_id(c)], E.reference(c, mut)
            for name in ref:
                if name not in E.exact_outputs(c):
                    ok, err, bound = E.within(bad[name], ref[name], E.tolerance(c, name))
                    assert not ok, (E.case_id(c), mut, name, err, bound)


def test_every_route_of_every_entry_has_a_case():
    have = {}
    for c in CASES:
        have.setdefault(c["entry"], set()).add(c["route"])
    for e, _, _ in E.REFUSALS:
        have.setdefault(e, set()).add("refused")
    for e, routes in E.ROUTES_OF_ENTRY.items():
        assert have.get(e, set()) == routes, (e, routes ^ have.get(e, set()))
    assert set(E.ROUTES_OF_ENTRY) | {"conv1d_l2norm_f16"} == set(E.FAMILY)


def test_binding_names_the_header_routes_and_entries():
    from fs_eend_amd import lib as L
    txt = open(os.path.join(ROOT, "include", "eend_hip.h")).read()
    routes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define EEND_ROUTE_(\w+) \(?(-?\d+)\)?", txt)}
    assert routes.pop("null") == L.ROUTE_NULL == -1
    assert {L.ROUTES[v]: v for v in routes.values()} == routes
    enum = re.search(r"enum eend_linear_entry \{(.*?)\}", txt, flags=re.S).group(1)
    names = [n.strip()[len("EEND_ENTRY_"):].lower() for n in enum.replace("= 0", "").split(",")]
    assert names == list(L.LINEAR_ENTRIES) + ["count"]
    assert set(L.LINEAR_ENTRIES) == set(E.ROUTES_OF_ENTRY)
    fields = re.search(r"typedef struct eend_linear_route_args \{(.*?)\}", txt, flags=re.S).group(1)
    assert re.findall(r"\b(\w+)\s*[,;]", fields) == [f for f, _ in L.LinearRouteArgs._fields_]


def test_every_case_takes_the_route_it_was_written_for(hip_lib):
    """eend_linear_route runs the entries' own routing code and launches nothing, so the tags of the tables are checked here too"""
    from fs_eend_amd import lib as L
    assert hip_lib.eend_linear_route(len(L.LINEAR_ENTRIES), None) == -1 and hip_lib.eend_linear_route(-1, None) == -1
    for c in CASES:
        if c["entry"] in E.ROUTES_OF_ENTRY:
            assert L.linear_route(c["entry"], **E.route_fields(c)) == c["route"], E.case_id(c)
    for e, f, why in E.REFUSALS:
        assert L.linear_route(e, **f) == "refused", (e, why)


def test_route_thresholds(hip_lib):
    """the thresholds between two kernels, one step to either side"""
    from fs_eend_amd import lib as L
    lin = lambda **k: L.linear_route("linear_f16", **dict(dict(M=64, N=256, K=256, lda=256, ldw=256, ldo=256), **k))
    assert [lin(M=m) for m in (16, 17)] == ["skinny", "proj"]
    assert [lin(M=8, K=k, lda=k, ldw=k) for k in (512, 520)] == ["skinny", "skinny_splitk"]
    assert [lin(N=n, ldo=n) for n in (1024, 1280)] == ["proj", "gemm128_straight"]
    assert [lin(ldw=w) for w in (256, 264)] == ["proj", "gemm128_straight"]
    assert lin(bias=-1) == lin(act=1) == "gemm128_straight" and lin(K=192, lda=192, ldw=192) == "gemm128_looped"
    assert lin(M=8, a=8) == "proj" and lin(M=8, lda=260) == "refused"           # skinny needs 16-byte rows; proj too
    step = lambda **k: L.linear_route("linear_step_f32", **dict(dict(M=64, N=256, K=256, lda=256, ldw=256, ldo=256), **k))
    assert [step(M=m) for m in (16, 17)] == ["skinny", "f32_mfma"]
    assert [step(K=k, lda=k, ldw=k) for k in (768, 784)] == ["f32_mfma", "f32_mfma_splitk"]
    assert [step(K=k, lda=k, ldw=k) for k in (504, 520)] == ["skinny_rowgroups", "skinny_rowgroups_splitk"]
    assert step(N=24) == step(bias=4) == step(out_f32=4) == "skinny_rowgroups"
    fan = lambda **k: L.linear_route("convert_fanout_f16", **dict(dict(nseq=2, Tp=64, C=4), **k))
    assert [fan(C=c) for c in (32, 33)] == ["convert_rows", "gemm64x256"]
    assert fan(nseq=65536, Tp=64) == "gemm64x256"                                  # B * Tp * 512 reaches 2^31
    heads = lambda **k: L.linear_route("inproj_heads_bf16", **dict(dict(nseq=2, Tp=64, H=4, dh=64, K=256, lda=256, ldw=256), **k))
    assert [heads(), heads(H=2), heads(H=8), heads(ldw=264), heads(K=320, lda=320, ldw=320)] == \
        ["proj", "gemm128_straight", "gemm128_straight", "gemm128_straight", "gemm128_looped"]
    ln = lambda **k: L.linear_route("linear_res_ln_f16", **dict(dict(M=4, K=256, lda=256, ldw=256), **k))
    assert [ln(), ln(out_f32=-1), ln(M=17), ln(K=2048, lda=2048, ldw=2048)] == ["skinny", "gemm64x256", "gemm64x256", "skinny_splitk"]
