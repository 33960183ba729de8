"""CPU tests of the trainers' weight copies (utils/model.py: WeightClock, WeightCopies, COPY_KINDS): one owner, one freshness rule.  No library call: the
two plane writers of the library are replaced by counters."""
import types

import pytest
import torch

ACTOR = (47, 256, 128, 128, 12)
CRITIC = (61, 256, 256, 128, 1)
KIN = 64
KINDS = {"cplanes": (0, 1, 2), "w0pad": (0,), "cplanes_t": (1, 2), "wt": (1, 2), "planes": (0, 1, 2), "planes_t": (1, 2)}  # the layers each kind is read for
PLANE_WRITER = {"cplanes": "bg_mlp_split_weights_pm", "cplanes_t": "bg_mlp_split_weights_pm", "planes": "bg_mlp_split_weights", "planes_t": "bg_mlp_split_weights"}


@pytest.fixture
def calls(monkeypatch):
    """The plane writers as counters: calls[name] = [(n, k, transpose, destination pointer), ...] of every call of library function `name`."""
    from booster_gym_amd import _lib

    log = {"bg_mlp_split_weights_pm": [], "bg_mlp_split_weights": []}

    def writer(name):
        def f(n, k, w, ld, rows, cols, transpose, out, stream):
            assert (ld, stream) == (cols, None)
            log[name].append((n, k, transpose, out.value))
            return 0
        return f

    monkeypatch.setattr(_lib, "load", lambda: types.SimpleNamespace(**{name: writer(name) for name in log}))
    monkeypatch.setattr(_lib, "current_stream_ptr", lambda: None)
    return log


def _flat_net(widths):
    """A Sequential of these widths on the CPU whose parameters are views of one flat buffer, as FlatAdam makes them (every tensor on a 4-float boundary)."""
    from booster_gym_amd.utils.model import _mlp

    torch.manual_seed(sum(widths))
    seq = _mlp(widths[0], widths[1:-1], widths[-1])
    params = list(seq.parameters())
    offsets, n = [], 0
    for p in params:
        offsets.append(n)
        n += (p.numel() + 3) // 4 * 4
    flat = torch.zeros(n)
    for p, off in zip(params, offsets):
        flat[off : off + p.numel()].copy_(p.data.reshape(-1))
        p.data = flat[off : off + p.numel()].view_as(p)
    layers = [m for m in seq if isinstance(m, torch.nn.Linear)]
    return seq, layers, flat, [offsets[2 * i] for i in range(len(layers))]


def _writes(calls):
    return sum(len(v) for v in calls.values())


@pytest.mark.parametrize("widths", [ACTOR, CRITIC])
def test_without_a_clock_every_get_rewrites(calls, widths):
    from booster_gym_amd.utils.model import WeightCopies

    _, layers, _, _ = _flat_net(widths)
    c = WeightCopies(layers, None, KIN)
    n = 0
    for kind in PLANE_WRITER:
        for i in KINDS[kind]:
            t = c.get(kind, i)
            for _ in range(2):
                assert c.get(kind, i) is t and not c.current(kind, i)
            n += 3
            assert _writes(calls) == n and len(calls[PLANE_WRITER[kind]]) >= 3 and calls[PLANE_WRITER[kind]][-1][3] == t.data_ptr()
    c.stamp()  # (nothing listed, no clock: nothing becomes current)
    assert not any(c.current(*key) for key in c.tensors)
    # the tensor-copy kinds follow the parameter on every get
    w0, wt = c.get("w0pad", 0), c.get("wt", 1)
    with torch.no_grad():
        layers[0].weight.add_(1.0); layers[1].weight.mul_(2.0)
    assert not torch.equal(w0[:, : widths[0]], layers[0].weight) and not torch.equal(wt, layers[1].weight.t())
    assert torch.equal(c.get("w0pad", 0)[:, : widths[0]], layers[0].weight) and torch.equal(c.get("wt", 1), layers[1].weight.t())


@pytest.mark.parametrize("widths", [ACTOR, CRITIC])
def test_with_a_clock_a_copy_is_written_once_per_tick(calls, widths):
    from booster_gym_amd.utils.model import COPY_KINDS, WeightClock, WeightCopies

    assert list(COPY_KINDS) == ["cplanes", "w0pad", "cplanes_t", "wt", "planes", "planes_t"]
    _, layers, _, _ = _flat_net(widths)
    clock = WeightClock()
    c = WeightCopies(layers, clock, KIN)
    n = 0
    for kind in PLANE_WRITER:
        for i in KINDS[kind]:
            rows, cols = layers[i].weight.shape
            kp = KIN if i == 0 else cols
            t = c.get(kind, i)
            n += 1
            assert _writes(calls) == n and c.current(kind, i)
            # shape and dtype of the table; the arguments of the writer as the kernels' call sites passed them
            planes = (2 if kind.startswith("c") else 1) * 3
            assert t.dtype == torch.int16 and t.numel() == planes * rows * kp and not t.any()
            assert calls[PLANE_WRITER[kind]][-1] == ((cols, rows, 1, t.data_ptr()) if kind.endswith("_t") else (rows, kp, 0, t.data_ptr()))
            assert c.get(kind, i) is t and c.get(kind, i) is t and _writes(calls) == n  # current: not written again
    clock.tick()
    assert not any(c.current(*key) for key in c.tensors)
    for key in list(c.tensors):
        c.get(*key)
        n += 1
        assert _writes(calls) == n and c.current(*key)  # rewritten on the first get after the tick
        c.get(*key)
        assert _writes(calls) == n
    # the tensor-copy kinds: the values themselves
    w0, wt = c.get("w0pad", 0), c.get("wt", 2)
    assert w0.shape == (widths[1], KIN) and w0.dtype == torch.float32 and torch.equal(w0[:, : widths[0]], layers[0].weight) and not w0[:, widths[0] :].any()
    assert wt.shape == (widths[2], widths[3]) and torch.equal(wt, layers[2].weight.t())
    with torch.no_grad():
        layers[0].weight.add_(1.0); layers[2].weight.mul_(2.0)
    assert c.get("w0pad", 0) is w0 and not torch.equal(w0[:, : widths[0]], layers[0].weight) and not torch.equal(c.get("wt", 2), layers[2].weight.t())
    clock.tick()
    assert torch.equal(c.get("w0pad", 0)[:, : widths[0]], layers[0].weight) and not w0[:, widths[0] :].any() and torch.equal(c.get("wt", 2), layers[2].weight.t())
    assert _writes(calls) == n  # (no plane was touched by those)


def _plan(fwd, bwd):
    from booster_gym_amd.utils.model import NetPlan

    return NetPlan(fwd, bwd, True, 0, (True,) * 4)


def _entries(ms):
    return [(m.offset, m.rows, m.cols, m.transpose, m.ld, m.pad) for m in ms]


@pytest.mark.parametrize("widths", [ACTOR, CRITIC])
def test_descriptors_are_those_the_optimiser_launch_got_before(calls, widths):
    """The bg_param_mirror entries of every plan, offsets against a flat buffer that the parameters are views of; the stamp; two owners on one clock."""
    from booster_gym_amd.utils.model import WeightClock, WeightCopies

    _, layers, flat, offs = _flat_net(widths)
    assert all(l.weight.data_ptr() == flat.data_ptr() + 4 * o for l, o in zip(layers, offs)) and offs[1] > 0
    shape = [tuple(l.weight.shape) for l in layers]
    clock = WeightClock()
    c = WeightCopies(layers, clock, KIN)
    split, split_fwd, chain = _plan("chain_split", "chain_split"), _plan("chain_split", "layer"), _plan("chain", "layer")
    assert c.descriptors(flat, split) == [] and c.listed == []  # only copies that exist are listed
    for i in range(3):
        c.get("cplanes", i)
    fwd = [(offs[i], shape[i][0], shape[i][1], 2, KIN if i == 0 else shape[i][1], shape[i][0] * (KIN if i == 0 else shape[i][1]) * 3) for i in range(3)]
    assert _entries(c.descriptors(flat, split)) == fwd and c.listed == [("cplanes", i) for i in range(3)]
    for i in (1, 2):
        c.get("cplanes_t", i)
    bwd = {i: (offs[i], shape[i][0], shape[i][1], 3, shape[i][0], shape[i][0] * shape[i][1] * 3) for i in (1, 2)}
    ms = c.descriptors(flat, split)
    assert _entries(ms) == [fwd[0], fwd[1], bwd[1], fwd[2], bwd[2]]
    assert [m.dst for m in ms] == [c.tensors[key].data_ptr() for key in c.listed] and c.listed[2] == ("cplanes_t", 1)
    # the fp32-chain plan: the padded first layer, and each transposed layer that exists; the planes it does not read are not listed
    assert c.descriptors(flat, chain) == []
    c.get("w0pad", 0)
    pad = (offs[0], shape[0][0], shape[0][1], 0, KIN, 0)
    assert _entries(c.descriptors(flat, chain)) == [pad]
    c.get("wt", 2)
    tr = {i: (offs[i], shape[i][0], shape[i][1], 1, shape[i][0], 0) for i in (1, 2)}
    assert _entries(c.descriptors(flat, chain)) == [pad, tr[2]]
    c.get("wt", 1)
    assert _entries(c.descriptors(flat, chain)) == [pad, tr[1], tr[2]]
    assert _entries(c.descriptors(flat, split_fwd)) == [fwd[0], fwd[1], tr[1], fwd[2], tr[2]]  # (the chained split forward in front of the per-layer backward)
    for i in range(3):
        c.get("planes", i)
    for i in (1, 2):
        c.get("planes_t", i)
    for plan in (_plan("layer_split", "layer_split"), _plan("library", "library")):
        assert c.descriptors(flat, plan) == [] and c.listed == []
    assert _entries(c.descriptors(flat, _plan("layer", "layer"))) == [pad, tr[1], tr[2]]

    # the stamp: what the launch listed is current at the new clock value, every other copy is stale and is rewritten by its next get
    c.descriptors(flat, split)
    n = _writes(calls)
    clock.tick()
    c.stamp()
    for key in c.tensors:
        assert c.current(*key) == (key[0] in ("cplanes", "cplanes_t")), key
    for i in range(3):
        c.get("cplanes", i)
    for i in (1, 2):
        c.get("cplanes_t", i)
    assert _writes(calls) == n
    c.get("planes", 0); c.get("planes_t", 1)
    assert _writes(calls) == n + 2 and len(calls["bg_mlp_split_weights"]) == 5 + 2

    # two owners over the same Sequential on one clock: stamping one leaves the other stale
    d = WeightCopies(layers, clock, KIN)
    for i in range(3):
        d.get("cplanes", i)
    assert all(d.current("cplanes", i) and c.current("cplanes", i) for i in range(3))
    c.descriptors(flat, split); d.descriptors(flat, split)
    clock.tick()
    c.stamp()
    assert all(c.current("cplanes", i) and not d.current("cplanes", i) for i in range(3))
    n = _writes(calls)
    for i in range(3):
        c.get("cplanes", i); d.get("cplanes", i)
    assert _writes(calls) == n + 3 and [x[3] for x in calls["bg_mlp_split_weights_pm"][-3:]] == [d.tensors["cplanes", i].data_ptr() for i in range(3)]


def test_rewrite_all_writes_what_exists_and_nothing_else(calls):
    from booster_gym_amd.utils.model import WeightClock, WeightCopies

    _, layers, _, _ = _flat_net(CRITIC)
    for clock in (None, WeightClock()):
        c = WeightCopies(layers, clock, KIN)
        c.rewrite_all()
        assert _writes(calls) == 0 and c.tensors == {}
        keys = [("cplanes", 0), ("cplanes", 2), ("cplanes_t", 1), ("planes_t", 2), ("w0pad", 0), ("wt", 1)]
        for key in keys:
            c.get(*key)
        for v in calls.values():
            v.clear()
        with torch.no_grad():
            layers[0].weight.add_(1.0); layers[1].weight.add_(1.0)
        c.rewrite_all()  # unconditionally: current copies too
        assert list(c.tensors) == keys
        assert [x[3] for x in calls["bg_mlp_split_weights_pm"]] == [c.tensors[k].data_ptr() for k in keys[:3]]
        assert [x[3] for x in calls["bg_mlp_split_weights"]] == [c.tensors["planes_t", 2].data_ptr()]
        assert torch.equal(c.tensors["w0pad", 0][:, :61], layers[0].weight) and torch.equal(c.tensors["wt", 1], layers[1].weight.t())
        assert all(c.current(*k) for k in keys) == (clock is not None)
        for v in calls.values():
            v.clear()


def test_a_trainer_hands_its_clock_to_its_copies_and_forgets_them_with_its_workspaces():
    from booster_gym_amd.utils.model import MLPTrainer, WeightClock

    seq, layers, _, _ = _flat_net(ACTOR)
    clock = WeightClock()
    a, b, alone = MLPTrainer(seq, clock=clock), MLPTrainer(seq, clock=clock), MLPTrainer(seq)
    assert a.copies.clock is b.copies.clock is clock and alone.copies.clock is None and a.copies is not b.copies
    a.prepare(torch.zeros(256, KIN))
    assert a.copies.kin == KIN and a.copies.kp(0) == KIN and a.copies.kp(1) == 256
    w0 = a.copies.get("w0pad", 0)
    a.prepare(torch.zeros(256, KIN))  # the same shape: the workspaces and the copies stay
    assert a.copies.get("w0pad", 0) is w0
    a.prepare(torch.zeros(128, KIN))
    assert a.copies.tensors == {}
