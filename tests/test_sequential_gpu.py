"""The column-affine kernel and the Sequential / Normalization / Denormalization modules on an MI355X: both launches against
torch's own fp32 expressions bit for bit, views, aliasing, error codes, fallbacks, the reference's recorded run (golden
``sequential.npz``) and agents whose actor is a ``Sequential``."""

from __future__ import annotations

import ctypes
import itertools

import numpy as np
import pytest
import torch

import _sequential

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 1e-5  # the standing bound, relative to the largest entry (as in tests/test_simba_gpu.py)
ROWS = (1, 3, 257, 2049)  # a single row, one block, a ragged last block, several blocks
WIDTHS = (1, 3, 4, 48, 50, 260)  # the scalar path (C % 4 != 0), the vector path, a width beyond one wave's lanes
FWD, BWD = "cusrl_column_affine_fwd", "cusrl_column_affine_bwd"


@pytest.fixture(scope="module")
def cusrl():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    import cusrl_amd

    cusrl_amd.config.set_device(DEV)
    return cusrl_amd


def _count(name):
    from cusrl_amd import _native

    return _native.launch_counts.get(name, 0)


def _on_device(case):
    return {key: value.to(DEV) for key, value in case.items()}


def _kernel_forward_backward(x, mean, std, dy, inverse):
    """(out, dx) through the autograd Function, with the launch census checked: one forward and one backward call."""
    from cusrl_amd import ops

    leaf = x.detach().requires_grad_(True)
    before = _count(FWD), _count(BWD)
    out = ops.ColumnAffine.apply(leaf, mean, std, inverse)
    (dx,) = torch.autograd.grad(out, leaf, grad_outputs=dy)
    assert (_count(FWD), _count(BWD)) == (before[0] + 1, before[1] + 1), "one forward and one backward call"
    return out.detach(), dx


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("rows,C", list(itertools.product(ROWS, WIDTHS)))
def test_kernel_gives_torchs_bits(cusrl, golden, rows, C):
    case = _on_device(_sequential.kernel_case(golden("sequential"), rows, C))
    assert all(t.data_ptr() % 16 == 0 for t in case.values())
    for inverse in (False, True):
        out, dx = _kernel_forward_backward(case["x"], case["mean"], case["std"], case["dy"], inverse)
        out_ref, dx_ref = _sequential.torch_forward_backward(case["x"], case["mean"], case["std"], case["dy"], inverse)
        differing = int((out != out_ref).sum()), int((dx != dx_ref).sum())
        print(f"[{rows}, {C}] inverse={inverse}: {differing[0]} forward and {differing[1]} backward entries differ from torch")
        assert torch.isfinite(out_ref).all() and torch.isfinite(dx_ref).all()
        assert _sequential.same_bits(out, out_ref), f"forward, inverse={inverse}"
        assert _sequential.same_bits(dx, dx_ref), f"backward, inverse={inverse}"


def test_infinities_and_nan_propagate_as_in_torch(cusrl, golden):
    case = _on_device(_sequential.kernel_case(golden("sequential"), 3, 4))
    x = case["x"].clone()
    x[0, 1], x[1, 2], x[2, 3] = float("inf"), float("-inf"), float("nan")
    for inverse in (False, True):
        out, dx = _kernel_forward_backward(x, case["mean"], case["std"], case["dy"], inverse)
        out_ref, dx_ref = _sequential.torch_forward_backward(x, case["mean"], case["std"], case["dy"], inverse)
        assert torch.isinf(out_ref).sum() == 2 and torch.isnan(out_ref).sum() == 1
        assert _sequential.same_bits(out, out_ref) and _sequential.same_bits(dx, dx_ref)


def _offset_view(t):
    """The same values one float off a 16-byte boundary."""
    buffer = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buffer[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("inverse", [False, True])
def test_views_give_the_bits_of_the_contiguous_call(cusrl, golden, inverse):
    g = golden("sequential")
    # a pointer off the 16-byte boundary at C = 4: the 4-byte lanes, the same bits
    case = _on_device(_sequential.kernel_case(g, 257, 4))
    aligned = _kernel_forward_backward(case["x"], case["mean"], case["std"], case["dy"], inverse)
    for shifted in ("x", "dy", "std"):
        moved = dict(case)
        moved[shifted] = _offset_view(case[shifted])
        offset = _kernel_forward_backward(moved["x"], moved["mean"], moved["std"], moved["dy"], inverse)
        assert all(torch.equal(a, b) for a, b in zip(aligned, offset)), f"{shifted} as an offset view"
    # a temporal batch [T, B, C] is the [T * B, C] launch
    case = _on_device(_sequential.kernel_case(g, 15, 6))
    flat = _kernel_forward_backward(case["x"], case["mean"], case["std"], case["dy"], inverse)
    temporal = _kernel_forward_backward(case["x"].view(5, 3, 6), case["mean"], case["std"], case["dy"].view(5, 3, 6), inverse)
    assert temporal[0].shape == temporal[1].shape == (5, 3, 6)
    assert all(torch.equal(a.view(15, 6), b) for a, b in zip(temporal, flat))
    # a non-contiguous x (and dy) is staged
    case = _on_device(_sequential.kernel_case(g, 48, 257))
    x_t, dy_t = case["x"].t(), case["dy"].t()  # [257, 48] views with strides (1, 257)
    assert not x_t.is_contiguous()
    mean, std = case["mean"][:48].contiguous(), case["std"][:48].contiguous()
    staged = _kernel_forward_backward(x_t, mean, std, dy_t, inverse)
    contiguous = _kernel_forward_backward(x_t.contiguous(), mean, std, dy_t.contiguous(), inverse)
    assert all(torch.equal(a, b) and a.is_contiguous() for a, b in zip(staged, contiguous))
    assert _sequential.same_bits(staged[0], _sequential.torch_expression(x_t, mean, std, inverse))


def _raw(name):
    from cusrl_amd import _native

    return getattr(_native.lib(), name)


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("rows,C", [(2049, 48), (257, 50)])
def test_in_place_through_the_raw_entry_points(cusrl, golden, rows, C):
    case = _on_device(_sequential.kernel_case(golden("sequential"), rows, C))
    for inverse in (0, 1):
        expected = _sequential.torch_expression(case["x"], case["mean"], case["std"], bool(inverse))
        x = case["x"].clone()
        assert _raw(FWD)(x.data_ptr(), case["mean"].data_ptr(), case["std"].data_ptr(), x.data_ptr(), rows, C, inverse, _stream()) == 0
        assert torch.equal(x, expected)
        expected = case["dy"] * case["std"] if inverse else case["dy"] / case["std"]
        dy = case["dy"].clone()
        assert _raw(BWD)(dy.data_ptr(), case["std"].data_ptr(), dy.data_ptr(), rows, C, inverse, _stream()) == 0
        assert torch.equal(dy, expected)


def test_error_codes(cusrl):
    """Straight through ctypes; none of these calls launches anything."""
    from cusrl_amd import _native

    invalid = _native._CONSTANTS["E_INVALID"]
    x, out = torch.ones(3, 4, device=DEV), torch.full((3, 4), 7.0, device=DEV)
    mean, std = torch.zeros(4, device=DEV), torch.ones(4, device=DEV)
    fwd, bwd, s = _raw(FWD), _raw(BWD), _stream()
    X, M, S, O = x.data_ptr(), mean.data_ptr(), std.data_ptr(), out.data_ptr()
    for arguments in ((None, M, S, O, 3, 4, 0), (X, None, S, O, 3, 4, 0), (X, M, None, O, 3, 4, 0), (X, M, S, None, 3, 4, 0),
                      (X, M, S, O, 3, 0, 0), (X, M, S, O, 3, -4, 0), (X, M, S, O, -1, 4, 0), (X, M, S, O, 3, 4, 2), (X, M, S, O, 3, 4, -1)):
        assert fwd(*arguments, s) == invalid, arguments
    for arguments in ((None, S, O, 3, 4, 0), (X, None, O, 3, 4, 0), (X, S, None, 3, 4, 0), (X, S, O, 3, 0, 1), (X, S, O, -1, 4, 1),
                      (X, S, O, 3, 4, 2)):
        assert bwd(*arguments, s) == invalid, arguments
    for inverse in (0, 1):  # rows == 0: a successful no-op
        assert fwd(X, M, S, O, 0, 4, inverse, s) == 0 and bwd(X, S, O, 0, 4, inverse, s) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full((3, 4), 7.0, device=DEV))
    assert ctypes.c_int(invalid).value < 0


@pytest.mark.parametrize("form", ["autocast", "double_differentiable", "float64", "trainable_statistics"])
def test_fallbacks_leave_the_kernel_alone(cusrl, form):
    from cusrl_amd import ops
    from cusrl_amd.nn.module import double_differentiable

    gen = torch.Generator().manual_seed(5)
    x = torch.randn(40, 12, generator=gen).to(DEV).requires_grad_(True)
    mean, std = torch.randn(12, generator=gen).to(DEV), (torch.rand(12, generator=gen) + 0.5).to(DEV)
    if form == "float64":
        x, mean, std = (t.detach().double().requires_grad_(t.requires_grad) for t in (x, mean, std))
    if form == "trainable_statistics":
        std.requires_grad_(True)
    for inverse in (False, True):
        before = _count(FWD), _count(BWD)
        with torch.autocast("cuda", enabled=form == "autocast"):
            if form == "double_differentiable":
                with double_differentiable():
                    assert not ops.column_affine_supported(x, mean, std)
                    out = ops.column_affine(x, mean, std, inverse)
            else:
                assert not ops.column_affine_supported(x, mean, std)
                out = ops.column_affine(x, mean, std, inverse)
            out_ref = _sequential.torch_expression(x, mean, std, inverse)
        assert out.dtype == out_ref.dtype and torch.equal(out, out_ref)
        inputs = [x, std] if form == "trainable_statistics" else [x]
        grads = torch.autograd.grad(out.float().square().sum(), inputs, create_graph=form == "double_differentiable")
        grads_ref = torch.autograd.grad(out_ref.float().square().sum(), inputs)
        assert all(torch.equal(a, b) for a, b in zip(grads, grads_ref))
        if form == "double_differentiable":  # a second differentiation goes through torch's own differentiable ops
            (second,) = torch.autograd.grad(grads[0].square().sum(), x)
            assert torch.isfinite(second).all() and second.abs().sum() > 0
        assert (_count(FWD), _count(BWD)) == before
    with torch.no_grad():  # outside those forms the same operands launch; without a gradient the forward launch alone
        before = _count(FWD), _count(BWD)
        ops.column_affine(x.detach().float(), mean.detach().float(), std.detach().float())
        assert (_count(FWD), _count(BWD)) == (before[0] + 1, before[1])
    if form == "double_differentiable":  # ... and inside the context a pass nobody differentiates launches too
        with double_differentiable(), torch.no_grad():
            ops.column_affine(x, mean, std)
        assert _count(FWD) == before[0] + 2


# ------------------------------------------------------------------------------------------------ the module
def _relative_to_largest(candidate, reference) -> float:
    reference = np.asarray(reference, dtype=np.float64)
    return float(np.abs(candidate.detach().cpu().numpy().astype(np.float64) - reference).max() / np.abs(reference).max())


@pytest.mark.parametrize("prefix", list(_sequential.CALLS))
def test_module_reproduces_the_reference_on_the_device(cusrl, golden, prefix):
    g = golden("sequential")
    module = _sequential.golden_module(cusrl, g, DEV)
    before = _count(FWD), _count(BWD)
    output, memory, keys, grad = _sequential.run_call(module, g, prefix, DEV)
    # one launch per affine layer and direction (the input asks for a gradient)
    assert (_count(FWD), _count(BWD)) == (before[0] + 2, before[1] + 2)
    assert keys == [str(k) for k in g[prefix + "repr_keys"]]
    errors = {"output": _relative_to_largest(output, g[prefix + "output"]), "grad_input": _relative_to_largest(grad, g[prefix + "grad_input"])}
    recorded = _sequential.recorded_memory(g, prefix)
    assert sorted(memory) == sorted(recorded)
    for key, value in recorded.items():
        assert memory[key].shape == value.shape
        errors["memory/" + key] = _relative_to_largest(memory[key], value)
    print(f"sequential {prefix}: " + ", ".join(f"{name} {error:.3e}" for name, error in errors.items()) + " of the largest entry")
    for name, error in errors.items():
        assert error <= BOUND, f"{prefix}{name}: {error:.3e} of the largest entry"
    with torch.no_grad():  # the no-grad pass: the forward launches alone, the same output bits
        before = _count(FWD), _count(BWD)
        kwargs = dict(_sequential.CALLS[prefix])
        if kwargs.pop("done", False):
            kwargs["done"] = torch.from_numpy(g["done"].copy()).to(DEV)
        observation = torch.from_numpy(g["input"].copy()).to(DEV)
        observation = observation[0].contiguous() if prefix == "step_" else observation
        again, _ = module(observation, memory={"2": torch.from_numpy(g["initial_memory/2"].copy()).to(DEV)}, **kwargs)
        assert torch.equal(again, output) and (_count(FWD), _count(BWD)) == (before[0] + 2, before[1])


# ------------------------------------------------------------------------------------------------ agents
def _statistics(dim):
    return torch.linspace(-1.0, 1.0, dim), torch.linspace(0.5, 2.0, dim)


def _statistic_parameters(agent):
    found = {name: param for name, param in agent.named_parameters() if name.startswith("actor.backbone.layers.0.")}
    assert sorted(found) == ["actor.backbone.layers.0.mean", "actor.backbone.layers.0.std"]
    return found


def _assert_optimizer_leaves_statistics_alone(agent, observation_dim):
    mean, std = _statistics(observation_dim)
    statistics = _statistic_parameters(agent)
    held = {id(p) for group in agent.optimizer.param_groups for p in group["params"]}
    assert not held & {id(p) for p in statistics.values()}
    if agent.flat_gradients is not None:
        assert not {id(p) for p in agent.flat_gradients.params} & {id(p) for p in statistics.values()}
    assert torch.equal(statistics["actor.backbone.layers.0.mean"].cpu(), mean)
    assert torch.equal(statistics["actor.backbone.layers.0.std"].cpu(), std)
    assert all(p.grad is None and not p.requires_grad for p in statistics.values())


def test_recurrent_agent_with_a_sequential_actor_trains(cusrl):
    """Normalization -> Mlp -> Gru as the actor's backbone: 8 envs, 4 steps per update, 2 iterations."""

    class Census(cusrl.Hook):
        def __init__(self):
            super().__init__()
            self.marks = []

        def pre_update(self, buffer):
            self.marks.append(("pre_update", _count(FWD)))

        def post_update(self):
            self.marks.append(("post_update", _count(FWD)))

    cusrl.set_global_seed(7)
    env = cusrl.testing.DummyTorchEnvironment(num_instances=8, observation_dim=10, action_dim=4, device=DEV)
    factory = cusrl.preset.RecurrentPpoAgentFactory(rnn_type="GRU", actor_hidden_size=16, critic_hidden_size=16, num_steps_per_update=4,
                                                    sampler_epochs=2, sampler_mini_batches=2).to_underlying()
    factory.actor_factory.backbone_factory = cusrl.Sequential.Factory(
        [cusrl.Normalization.Factory(*_statistics(10)), cusrl.Mlp.Factory([16], ends_with_activation=True),
         cusrl.Gru.Factory("gru", hidden_size=16)], hidden_dims=[None, None])
    census = Census()
    factory.register_hook(census)
    trainer = cusrl.Trainer(env, factory, num_iterations=2, verbose=False)
    agent = trainer.agent
    backbone = agent.actor.backbone
    assert isinstance(backbone, cusrl.Sequential) and backbone.is_recurrent and agent.actor.is_recurrent
    assert [type(layer).__name__ for layer in backbone.layers] == ["Normalization", "Mlp", "Rnn"]
    initial = {name: param.detach().clone() for name, param in agent.named_parameters()}
    start = _count(FWD)
    trainer.run_training_loop()
    torch.cuda.synchronize()
    assert [kind for kind, _ in census.marks] == ["pre_update", "post_update"] * 2
    counts = [start, *(count for _, count in census.marks)]
    rollout, update = (counts[1] - counts[0], counts[3] - counts[2]), (counts[2] - counts[1], counts[4] - counts[3])
    print(f"{FWD}: {rollout} calls during the two rollouts, {update} during the two updates")
    assert all(n >= 4 for n in rollout), "one launch per act step"
    assert all(n >= 2 * 2 for n in update), "one launch per minibatch step"
    for key in ("Agent/value_loss", "Agent/surrogate_loss", "Agent/kl_divergence"):
        if key in trainer.last_info:
            assert np.isfinite(trainer.last_info[key]), key
    assert np.isfinite(trainer.last_info["Agent/value_loss"])
    assert any(key.split(".")[0] == "actor_memory" and key.endswith("2") for key in agent.buffer.storage), list(agent.buffer.storage)
    _assert_optimizer_leaves_statistics_alone(agent, 10)
    statistics = _statistic_parameters(agent)
    changed = 0
    for name, param in agent.named_parameters():
        assert torch.isfinite(param).all(), name
        changed += int(not torch.equal(param, initial[name]))
        if name in statistics:
            assert torch.equal(param, initial[name]), name
    assert changed == len(initial) - len(statistics), "every trainable parameter takes part in the update, the statistics do not"


def _train_feed_forward(cusrl, capture, iterations=4, N=64, T=4):
    cusrl.set_global_seed(21)
    env = cusrl.testing.DummyTorchEnvironment(num_instances=N, observation_dim=12, action_dim=4, device=DEV)
    factory = cusrl.preset.PpoAgentFactory(num_steps_per_update=T, sampler_epochs=2, sampler_mini_batches=2, compile=True,
                                           optimizer_kwargs={"capturable": True, "fused": True}).to_underlying()
    factory.actor_factory.backbone_factory = cusrl.Sequential.Factory(
        [cusrl.Normalization.Factory(*_statistics(12)), cusrl.Mlp.Factory([32, 32], ends_with_activation=True)], hidden_dims=[None])
    trainer = cusrl.Trainer(env, factory, num_iterations=iterations, verbose=False)
    trainer.capture_rollout = capture  # (the switch of tests/test_captured_rollout.py)
    before = _count(FWD)
    trainer.run_training_loop()
    torch.cuda.synchronize()
    return trainer, _count(FWD) - before


def test_captured_rollout_with_a_sequential_actor_is_bit_identical_to_the_host_driven_loop(cusrl):
    """A feed-forward ``Sequential`` actor under compile=True (a recurrent actor's rollout is never captured): the env step
    replays from its graph with the affine launch inside, and buffer and parameters are the host-driven loop's bit for bit."""
    T = 4
    host, host_calls = _train_feed_forward(cusrl, capture=False, T=T)
    assert host._graphed_rollout is None
    captured, captured_calls = _train_feed_forward(cusrl, capture=True, T=T)
    graphed = captured._graphed_rollout
    assert graphed is not None and graphed.captured == T and len(graphed.rollouts) == 1
    assert isinstance(captured.agent.actor.backbone, cusrl.Sequential)
    print(f"{FWD}: {host_calls} calls host-driven, {captured_calls} with the rollout captured (a replay issues no C call)")
    assert host_calls > 0 and captured_calls > 0
    a, b = host.agent, captured.agent
    assert a.flat_optimizer is not None and b.flat_optimizer is not None
    for key in a.buffer.storage:
        assert torch.equal(a.buffer.storage[key], b.buffer.storage[key]), key
    for (name, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.isfinite(p).all() and torch.equal(p, q), name
    for agent in (a, b):
        _assert_optimizer_leaves_statistics_alone(agent, 12)
