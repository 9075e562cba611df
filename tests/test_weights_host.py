"""The operand cache every model shares (fs_eend_amd.weights.PreparedOperands), on the CPU: when `_build_operands` runs again, that a
rebuild is a new object and empties the derived-constant cache, and which tensors each fingerprint sees."""
import torch
import torch.nn as nn

from fs_eend_amd.weights import PreparedOperands


class _Toy(PreparedOperands, nn.Module):
    """parameters + buffers, the base's fingerprint"""

    def __init__(self):
        super().__init__()
        self.lin = nn.Linear(4, 3)
        self.register_buffer("table", torch.zeros(5))
        self.builds = 0

    def _build_operands(self):
        self.builds += 1
        return {"w": self.lin.weight.detach().clone()}


class _ToyParamsOnly(_Toy):
    def _fingerprint_tensors(self):
        return list(self.parameters())


def test_second_prepare_reuses_the_operands():
    m = _Toy()
    P = m._prepare()
    assert m.builds == 1 and m._prep is P
    assert m._prepare() is P and m.builds == 1


def test_every_tracked_change_rebuilds_into_a_new_object():
    m = _Toy()
    seen = [m._prepare()]

    def rebuilt():
        P = m._prepare()
        assert all(P is not old for old in seen), "a rebuild must hand out a new dict: the sessions compare identity"
        assert m._prep is P and m.builds == len(seen) + 1
        assert m._prepare() is P and m.builds == len(seen) + 1
        seen.append(P)

    with torch.no_grad():
        m.lin.weight.add_(1.0)                          # a _version bump
    rebuilt()
    m.load_state_dict({k: v.clone() for k, v in m.state_dict().items()})
    assert m._prep is None                              # the post hook dropped the copies at once
    rebuilt()
    m.to(torch.float64)                                 # _apply
    assert m._prep is None
    rebuilt()
    assert seen[-1]["w"].dtype == torch.float64
    m.refresh_weights()
    assert m._prep is None
    rebuilt()


def test_a_data_write_is_the_documented_blind_spot():
    m = _Toy()
    P = m._prepare()
    m.lin.weight.data.copy_(torch.ones(3, 4))           # no _version bump
    assert m._prepare() is P and m.builds == 1
    assert not torch.equal(P["w"], m.lin.weight)        # the copies ARE stale: refresh_weights() is the caller's duty
    m.refresh_weights()
    assert torch.equal(m._prepare()["w"], m.lin.weight) and m.builds == 2


def test_derived_constants_live_until_the_next_rebuild():
    m = _Toy()
    m._prepare()
    calls = []
    build = lambda: calls.append(1) or torch.ones(2)
    a = m._derived(("pc", 3), build)
    assert m._derived(("pc", 3), build) is a and len(calls) == 1
    m._derived(("pc", 4), build)
    assert set(m._consts) == {("pc", 3), ("pc", 4)}
    m._prepare()
    assert set(m._consts) == {("pc", 3), ("pc", 4)}     # no rebuild: kept

    def bump():
        with torch.no_grad():
            m.lin.bias.add_(1.0)

    for change in (bump, m.refresh_weights, lambda: m.load_state_dict(m.state_dict()), lambda: m.to(torch.float64)):
        m._derived(("pc", 3), build)
        assert m._consts
        change()
        m._prepare()
        assert m._consts == {}, "every rebuild empties the derived cache"


def test_fingerprint_params_only_ignores_a_buffer_write():
    m = _ToyParamsOnly()
    P = m._prepare()
    m.table.add_(1.0)
    assert m._prepare() is P and m.builds == 1
    with torch.no_grad():
        m.lin.bias.add_(1.0)
    assert m._prepare() is not P and m.builds == 2


def test_fingerprint_params_and_buffers_sees_a_buffer_write():
    m = _Toy()
    P = m._prepare()
    m.table.add_(1.0)
    assert m._prepare() is not P and m.builds == 2


def test_models_keep_their_fingerprints():
    """FS / LS / FS-streaming: parameters + buffers; the EDA attractor: its parameters; the EDA model: the encoder's parameters."""
    from fs_eend_amd.eda_model import TransformerEDADiarization
    from fs_eend_amd.fs_model import OnlineTransformerDADiarization
    from fs_eend_amd.fs_stream import StreamingTransformerEDADiarization
    ids = lambda ts: [id(t) for t in ts]
    cfg = dict(n_units=256, n_heads=4, enc_n_layers=1, dec_n_layers=1, dropout=0.1, has_mask=True, max_seqlen=500, dec_dim_feedforward=64)
    for m in (OnlineTransformerDADiarization(n_speakers=None, in_size=23, **cfg), StreamingTransformerEDADiarization(in_size=23, **cfg)):
        assert ids(m._fingerprint_tensors()) == ids(list(m.parameters()) + list(m.buffers()))
        assert len(list(m.buffers())) > 0
    e = TransformerEDADiarization(n_speakers=None, in_size=23, n_units=256, n_heads=4, n_layers=1, dropout=0.1)
    assert ids(e._fingerprint_tensors()) == ids(e.enc.parameters())
    assert ids(e.eda._fingerprint_tensors()) == ids(e.eda.parameters())


def test_eda_refresh_drops_the_attractor_cache_too():
    from fs_eend_amd.eda_model import TransformerEDADiarization
    e = TransformerEDADiarization(n_speakers=None, in_size=23, n_units=256, n_heads=4, n_layers=1, dropout=0.1)
    for trigger in (e.refresh_weights, lambda: e.load_state_dict(e.state_dict()), lambda: e.to(torch.float32)):
        e._prep, e.eda._prep = {"stale": 1}, {"stale": 1}          # stand-ins: nothing is launched on the CPU
        trigger()
        assert e._prep is None and e.eda._prep is None
