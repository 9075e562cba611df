"""CPU: the constructions of tests/traingemm_edge_ref.py do what tests/test_traingemm_edges.py relies on.  Both exactness guards hold for
every tabled case, every toleranced row has non-zero variance / norm (reference() asserts it), every mutation applies somewhere and
changes the reference of every case it applies to UNDER THE COMPARISON OF THE GPU TEST (torch.equal up to the sign of zero on the exact
outputs, the tolerance on the others), every 8 x gap32 bound is a bound (gap32 > 0) and the case ids are unique.  The persistent FFN cases
are resolved with the MI355X's 256 compute units here; the GPU test reads the count from the device."""
import pytest
import torch

from tests import linear_edge_ref as L
from tests import traingemm_edge_ref as E

CASES = [E.resolve(c) for c in E.all_cases()]


@pytest.fixture(scope="module")
def references():
    """case id -> (buffers, aux) of every tabled case; computing them runs guard (a) on the operands and guard (b) on the 2-byte outputs"""
    return {E.case_id(c): E.reference(c, with_aux=True) for c in CASES}


def test_case_ids_are_unique_and_every_entry_is_tabled():
    ids = [E.case_id(c) for c in E.all_cases()]
    assert len(ids) == len(set(ids)) > 200
    assert {c["entry"] for c in CASES} == set(E.FAMILY) == {e for e, _, _ in E.REFUSALS}
    assert sum(1 for c in CASES if c.get("persist")) == 3 and all(c["M"] == 128 * E.NCU_MI355X + 129 for c in CASES if c.get("persist"))


def test_guards_hold_for_the_whole_table(references):
    for c in CASES:
        ref, aux = references[E.case_id(c)]
        exact = E.exact_outputs(c)
        assert ref and (set(exact) & set(ref) or E.FAMILY[c["entry"]] in ("l2train", "resln")), E.case_id(c)
        for name, buf in ref.items():
            live = ~buf.isnan()
            assert live.any() and float(buf[live].abs().max()) < E.LIMIT, (E.case_id(c), name)
            if name in exact:
                if E.FAMILY[c["entry"]] != "lnbwd":          # linear outputs are integers (half-integers under alpha = 0.5)
                    assert torch.equal(buf[live] * 2, (buf[live] * 2).round()), (E.case_id(c), name)
                if exact[name] == E.BF16:
                    assert torch.equal(buf[live].to(E.BF16).double(), buf[live])
                if exact[name] == E.F16:
                    assert torch.equal(buf[live].to(E.F16).double(), buf[live])
            else:
                assert E.tolerance(c, name) in E.TOL, (E.case_id(c), name)
                if E.TOL[E.tolerance(c, name)][0] == "gap" and name in E.ROW_SCALARS:   # about one f32 ulp, never a lucky zero
                    assert 2.0 ** -25 < E.pooled_gap(c["entry"], name) < 2.0 ** -21, (E.case_id(c), name, E.pooled_gap(c["entry"], name))
                elif E.TOL[E.tolerance(c, name)][0] == "gap":
                    assert aux["gap"][name] > 0, f"{E.case_id(c)}: {name}: a zero gap32 is no bound"
                if E.TOL[E.tolerance(c, name)][0] == "scale":
                    assert aux["scale"][name] > 0


def test_guard_rows_and_columns_are_nan(references):
    for c in CASES:
        if E.FAMILY[c["entry"]] == "heads":
            continue
        for name, buf in references[E.case_id(c)][0].items():
            if name in ("dgamma", "dbeta", "dbias"):
                assert buf.shape == (256,) and not buf.isnan().any()
                continue
            assert buf.shape[0] == E.rows_of(c) + E.GUARD_ROWS and buf[-E.GUARD_ROWS:].isnan().all() and not buf[:-E.GUARD_ROWS].reshape(buf.shape[0] - E.GUARD_ROWS, -1)[:, 0].isnan().any(), (E.case_id(c), name)
            if c.get("ldo") and c["ldo"] > c["N"]:
                assert buf[:, c["N"]:].isnan().all() and buf.shape[1] == c["ldo"], E.case_id(c)


def test_the_guards_can_fail():
    with pytest.raises(AssertionError):
        E.sum_bound(torch.full((2, 4096), 64.0), torch.full((2, 4096), 64.0))    # 64 * 64 * 4096 = 2^24
    with pytest.raises(AssertionError):
        E.as16(torch.tensor([257.0]), E.BF16)
    with pytest.raises(AssertionError):
        E.as16(torch.tensor([2049.0]), E.F16)
    with pytest.raises(AssertionError):
        L.layer_norm(torch.ones(2, 256), None, None, 1e-5)


def test_masks_hold_every_kind_of_zero():
    for c in CASES:
        if c["entry"] in ("gemm_relu_bwd_bf16", "ffn_bwd_data_bf16"):
            a = E.operands(c)["act"]
            neg0 = (a == 0) & torch.signbit(a)
            pairs = a.view(a.shape[0], -1, 2)
            mixed = (pairs[..., 0] == 0) != (pairs[..., 1] == 0)
            assert neg0.any() and (a == E.SUBNORMAL16).any() and ((a == 0) & ~torch.signbit(a)).any() and mixed.any(), E.case_id(c)
            assert torch.equal(a.to(E.F16).double(), a) and torch.equal(torch.signbit(a.to(E.F16)), torch.signbit(a))
            frac = float((a == 0).double().mean())
            assert 0.3 < frac < 0.7, (E.case_id(c), frac)


def test_dropout_is_half_and_half():
    for c in CASES:
        if c.get("drop"):
            o = E.operands(c)
            k = E.keep2(torch.arange(E.rows_of(c)), 256, o["drop_seed"], 1)
            assert set(k.unique().tolist()) <= {0.0, 2.0}
            if k.numel() >= 4096:
                assert 0.4 < float((k == 0).double().mean()) < 0.6, E.case_id(c)


@pytest.mark.parametrize("mut", E.MUTATIONS)
def test_every_mutation_changes_every_case_it_applies_to(references, mut):
    n = 0
    for c in CASES:
        if not E.applies(mut, c):
            continue
        n += 1
        ref, aux = references[E.case_id(c)]
        bad = E.reference(c, mut)
        assert set(bad) == set(ref)
        changed = [name for name in ref if not E.compare(c, name, bad[name], ref[name], aux)[0]]
        assert changed, f"{mut} leaves {E.case_id(c)} unchanged under the GPU test's comparison"
        if mut in ("ktile_dropped", "ktile_doubled"):
            keeps = (set(ref) & set(E.exact_outputs(c))) - set(changed)       # (doubling a lone k-tile leaves a LayerNorm output as it was)
            assert not keeps, f"{mut}: {E.case_id(c)} keeps {keeps}"
    assert n >= 3, (mut, n)


def test_the_references_compare_equal_to_themselves(references):
    for c in CASES:
        ref, aux = references[E.case_id(c)]
        for name, buf in ref.items():
            assert E.compare(c, name, buf.clone(), buf, aux)[0], (E.case_id(c), name)


def test_refusals_name_a_tabled_entry_each():
    assert len(E.REFUSALS) == len({(e, tuple(sorted(f.items()))) for e, f, _ in E.REFUSALS})
    for e, f, why in E.REFUSALS:
        assert e in E.FAMILY and f and why
