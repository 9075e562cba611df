"""GPU: the slot form of the packed in-projection + causal attention kernel (csrc/attn_stream.hip, eend_inproj_attn_causal_slots_f16): the C
speaker slots of an utterance differ by a constant input row per slot, so K / V^T are projected once from slot 0's rows and an item runs
the flash passes of S consecutive slots.  Every case has 512 frames per sequence, the kernel's only length."""
import functools

import pytest
import torch

from tests.test_attn_packed import _case, _fp32

pytestmark = pytest.mark.gpu
F16, F32 = torch.float16, torch.float32
TP = 512
EINVAL = -1

CASES = [(1, 1, 0, 512), (2, 6, 0, 500), (3, 3, 2, 470), (2, 5, 1000, 512), (1, 12, 0, 512), (2, 4, 3, 33)]


def _divisors(C):
    return [S for S in range(1, C + 1) if C % S == 0]


def _slot_case(dev, B, C, seed):
    """x0 / w / b of test_attn_packed._case for the B slot-0 sequences, input-space slot offsets pd[c] ~ 0.3 N(0, 1) with pd[0] = 0, and
    slot_delta built from them in torch.  xs: what the slot form is given (slot 0's rows; the other slots' rows are NaN -- they must not be
    read); xf: the unrounded operands x0 + pd[c] in f32; xm: the materialised rows f16(x0 + pd[c])."""
    x0, w, b = _case(dev, B, TP, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    pd = (0.3 * torch.randn(C, 256, generator=g)).to(dev)
    pd[0] = 0.0
    xf = (x0.float().view(B, 1, TP, 256) + pd.view(1, C, 1, 256)).reshape(B * C * TP, 256)
    xm = xf.to(F16)
    xs = torch.full((B, C, TP, 256), float("nan"), dtype=F16, device=dev)
    xs[:, 0] = x0.view(B, TP, 256)
    wf = w.float()
    sd = (pd[:, None, :] * torch.cat([wf[:256], wf[512:]])[None]).sum(-1).contiguous()       # [C][512] = (W_q pd[c] | W_v pd[c])
    sd[0] = 0.0
    return dict(x0=x0, w=w, b=b, xf=xf, xm=xm, xs=xs.view(B * C * TP, 256), sd=sd)


def _run_slots(c, wp, B, C, delay, kv, S):
    from fs_eend_amd import ops
    o = torch.full((B * C * TP, 256), float("nan"), dtype=F16, device=c["xs"].device)
    ops.inproj_attn_causal_packed(c["xs"], wp, c["b"], o, B * C, 4, TP, delay, kv, slots=C, slot_delta=c["sd"], slots_per_item=S)
    assert torch.isfinite(o).all()
    return o


@functools.lru_cache(maxsize=None)
def _results(dev, B, C, delay, kv):
    """One run per divisor S of C and the automatic choice (key 0), shared by the tests below."""
    from fs_eend_amd import ops
    c = _slot_case(dev, B, C, B * 17 + C * 3 + delay)
    wp = ops.inproj_attn_pack(c["w"])
    outs = {S: _run_slots(c, wp, B, C, delay, kv, S) for S in [0] + _divisors(C)}
    return c, wp, outs


@pytest.mark.parametrize("B,C,delay,kv", CASES)
def test_result_does_not_depend_on_slots_per_item(hip_lib, dev, B, C, delay, kv):
    """an item of S slots is a work decomposition, not an arithmetic: every divisor S of C and the automatic choice agree bit for bit"""
    _, _, outs = _results(dev, B, C, delay, kv)
    for S, o in outs.items():
        assert torch.equal(o, outs[1]), f"S = {S} differs from S = 1"


@pytest.mark.parametrize("B,C,S,S_other", [(11, 6, 1, 6), (65, 2, 2, 1)])
def test_more_items_than_workgroups(hip_lib, dev, B, C, S, S_other):
    """264 and 260 items on 256 persistent workgroups: the walk to a second item, against the same inputs at another S"""
    from fs_eend_amd import ops
    c = _slot_case(dev, B, C, B + C)
    wp = ops.inproj_attn_pack(c["w"])
    assert torch.equal(_run_slots(c, wp, B, C, 0, 500, S), _run_slots(c, wp, B, C, 0, 500, S_other))


@pytest.mark.parametrize("B,C,delay,kv", CASES)
def test_slot0_is_the_per_slot_kernel(hip_lib, dev, B, C, delay, kv):
    """a zero delta added before the single rounding is exact: slot 0 equals the entry without slots on the slot-0 sequences"""
    from fs_eend_amd import ops
    c, wp, outs = _results(dev, B, C, delay, kv)
    o0 = torch.full((B * TP, 256), float("nan"), dtype=F16, device=dev)
    ops.inproj_attn_causal_packed(c["x0"], wp, c["b"], o0, B, 4, TP, delay, kv)
    assert torch.equal(outs[0].view(B, C, TP, 256)[:, 0], o0.view(B, TP, 256))


@pytest.mark.parametrize("B,C,delay,kv", CASES)
def test_accuracy_of_every_slot(hip_lib, dev, B, C, delay, kv):
    """against fp32 torch on the unrounded operands x0 + pd[c] (< 2e-2) and against the per-slot entry on the materialised rows
    f16(x0 + pd[c]) (< 3e-2): the project's bounds for this kernel.  (A CPU emulation of both roundings at these inputs: 0.4-1.1e-2 for
    the slot form and 0.4-1.6e-2 for the per-slot form against fp32, at most 1.6e-2 between the two; measured on the MI355X over the six
    cases: 0.37-1.56e-2, 0.47-1.74e-2 and at most 2.34e-2 -- the kernels' bf16 probabilities come on top of the emulated roundings.)"""
    from fs_eend_amd import ops
    c, wp, outs = _results(dev, B, C, delay, kv)
    want = _fp32(c["xf"], c["w"], c["b"], B * C, TP, delay, kv)
    o1 = torch.full((B * C * TP, 256), float("nan"), dtype=F16, device=dev)
    ops.inproj_attn_causal_packed(c["xm"], wp, c["b"], o1, B * C, 4, TP, delay, kv)
    e_new = (outs[0].float() - want).abs().max().item()
    e_old = (o1.float() - want).abs().max().item()
    e_between = (outs[0].float() - o1.float()).abs().max().item()
    print(f"slots vs fp32 {e_new:.2e} (per slot vs fp32 {e_old:.2e}); slots vs per slot {e_between:.2e}")
    assert e_new < 2e-2
    assert e_between < 3e-2


def test_rejections_and_choice(hip_lib, dev):
    """other lengths, slot counts outside 1 .. 12, a missing table and an S that does not divide C: EEND_EINVAL; the choice of S is a pure
    function of (utterances, slots, workgroups)"""
    from fs_eend_amd import ops
    L = hip_lib
    c = _slot_case(dev, 2, 6, 5)
    wp = ops.inproj_attn_pack(c["w"])
    o = torch.zeros(2 * 6 * TP, 256, dtype=F16, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(nseq, Tp, C, sd, S):
        return L.eend_inproj_attn_causal_slots_f16(c["xs"].data_ptr(), 256, wp.data_ptr(), c["b"].data_ptr(), o.data_ptr(), nseq, 4, Tp, 256, 0, Tp,
                                                   C, sd, S, stream)

    sd = c["sd"].data_ptr()
    assert call(12, 448, 6, sd, 0) == EINVAL and call(12, 256, 6, sd, 0) == EINVAL and call(6, 1024, 6, sd, 0) == EINVAL
    assert call(12, TP, 0, sd, 0) == EINVAL and call(13, TP, 13, sd, 0) == EINVAL
    assert call(12, TP, 6, None, 0) == EINVAL
    assert call(12, TP, 6, sd, 4) == EINVAL and call(12, TP, 6, sd, 12) == EINVAL
    assert call(11, TP, 6, sd, 0) == EINVAL                   # not a whole number of utterances
    assert call(12, TP, 6, sd, 0) == 0 and call(2, TP, 1, None, 0) == 0
    torch.cuda.synchronize()
    assert ops.inproj_attn_slots_choice(64, 6, 256) == 6
    assert ops.inproj_attn_slots_choice(1, 6, 256) == 1
    assert L.eend_inproj_attn_slots_choice(1, 13, 256) == EINVAL


def test_model_slot_delta_follows_parameter_update(hip_lib, dev):
    """slot_delta is a constant of the weights: after an in-place update of dec.convert.weight the next call rebuilds it, and the logits
    equal those of a freshly built model with the same weights bit for bit"""
    from fs_eend_amd import fs_model as FM
    torch.manual_seed(3)
    cfg = dict(n_units=256, n_heads=4, enc_n_layers=2, dec_n_layers=2, dropout=0.1, has_mask=True, max_seqlen=500,
               dec_dim_feedforward=512, conv_delay=9, mask_delay=0, decom_kernel_size=64)
    m = FM.OnlineTransformerDADiarization(n_speakers=None, in_size=345, **cfg).eval().to(dev)
    g = torch.Generator().manual_seed(11)
    lens = [500, 470]
    src = [(torch.randn(l, 345, generator=g) * 2 - 3).to(dev) for l in lens]
    first = [x.clone() for x in m.test(src, lens, 3)[0]]
    assert 3 in m._sd                                         # the 512-frame window took the slot form
    with torch.no_grad():
        m.dec.convert.weight.add_(0.05 * torch.randn(m.dec.convert.weight.shape, generator=g).to(dev))
    second = [x.clone() for x in m.test(src, lens, 3)[0]]
    assert all(torch.isfinite(x).all() for x in second)
    assert any(not torch.equal(a, b) for a, b in zip(first, second))
    fresh = FM.OnlineTransformerDADiarization(n_speakers=None, in_size=345, **cfg).eval().to(dev)
    fresh.load_state_dict(m.state_dict())
    third = fresh.test(src, lens, 3)[0]
    for a, b in zip(second, third):
        assert torch.equal(a, b)
