"""Sequential, Normalization and Denormalization without a GPU: exports, the reference's error texts, the CPU expressions bit
for bit, the recorded reference run (golden ``sequential.npz``), memory handling, ``batch_invariant`` and the optimizer's view
of the non-trainable statistics."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import _sequential

NAMES = ("Sequential", "SequentialFactory", "Normalization", "NormalizationFactory", "Denormalization", "DenormalizationFactory")
REPR_KEYS = ["0/Normalization.output", "1/Mlp.output", "2/Gru.output", "3/Mlp.output", "4/Denormalization.output"]


@pytest.fixture(scope="module")
def cusrl():
    import cusrl_amd

    return cusrl_amd


def test_the_six_names_are_exported(cusrl):
    from cusrl_amd.nn import normalization, sequential

    for namespace in (cusrl, cusrl.nn):
        assert set(NAMES) <= set(namespace.__all__)
        for name in NAMES:
            home = sequential if name.startswith("Sequential") else normalization
            assert getattr(namespace, name) is getattr(home, name), name
    assert cusrl.Sequential.Factory is cusrl.SequentialFactory
    assert cusrl.Normalization.Factory is cusrl.NormalizationFactory
    assert cusrl.Denormalization.Factory is cusrl.DenormalizationFactory
    assert issubclass(cusrl.Denormalization, cusrl.Normalization)


def test_abi_version_stays_and_the_new_symbols_are_declared():
    from cusrl_amd import _native, ops

    assert _native.ABI_VERSION == 7
    assert {"cusrl_column_affine_fwd", "cusrl_column_affine_bwd"} <= set(_native.EXPORTED_SYMBOLS)
    assert callable(ops.column_affine) and callable(ops.column_affine_supported) and issubclass(ops.ColumnAffine, torch.autograd.Function)


def test_golden_holds_the_cases_of_record(golden):
    g = golden("sequential")
    assert [int(r) for r in g["kernel_rows"]] == [1, 3, 257, 2049] and [int(c) for c in g["kernel_widths"]] == [1, 3, 4, 48, 50, 260]
    std = g["kernel_std"]
    assert std.shape == (260,) and std.min() >= 1e-3 and std.max() <= 3
    assert g["input"].shape == (5, 3, 6) and g["done"].shape == (5, 3, 1) and g["initial_memory/2"].shape == (3, 8)
    assert g["done"].sum() == 1 and g["done"][2, 1, 0]  # one env's episode ends mid-sequence
    assert str(g["torch_version"])
    for prefix in _sequential.CALLS:
        assert [str(k) for k in g[prefix + "repr_keys"]] == REPR_KEYS
    assert [str(k) for k in g["seq_memory_keys"]] == [] and [str(k) for k in g["packed_memory_keys"]] == ["2"]


@pytest.mark.parametrize("kind", ["Normalization", "Denormalization"])
def test_factories_take_sequences_arrays_and_tensors_and_check_dims(cusrl, kind):
    module_type = getattr(cusrl, kind)
    mean, std = [0.5, -1.0, 2.0], [1.0, 2.0, 0.25]
    for form in (list, tuple, np.asarray, lambda v: np.asarray(v, dtype=np.float64), torch.tensor, lambda v: torch.tensor(v, dtype=torch.float64)):
        module = module_type.Factory(form(mean), form(std))()
        assert type(module) is module_type and (module.input_dim, module.output_dim) == (3, 3)
        assert module.mean.dtype == module.std.dtype == torch.float32
        assert torch.equal(module.mean, torch.tensor(mean)) and torch.equal(module.std, torch.tensor(std))
        assert not module.mean.requires_grad and not module.std.requires_grad
        assert isinstance(module.mean, torch.nn.Parameter) and list(module.state_dict()) == ["mean", "std"]
    factory = module_type.Factory(mean, std)
    assert factory(3, 3).input_dim == 3 and factory(3).output_dim == 3 and factory(None, 3).input_dim == 3
    with pytest.raises(ValueError, match="^Input dimension mismatch: expected 3, got 4$"):
        factory(4, 3)
    with pytest.raises(ValueError, match="^Output dimension mismatch: expected 3, got 5$"):
        factory(3, 5)
    with pytest.raises(ValueError, match="^Output dimension mismatch: expected 3, got 5$"):
        factory(None, 5)


@pytest.mark.parametrize("shape", [(7, 5), (4, 3, 5), (5,)])
def test_cpu_tensors_take_the_reference_expressions_bit_for_bit(cusrl, shape):
    from cusrl_amd import _native, ops

    gen = torch.Generator().manual_seed(11)
    mean, std = torch.randn(5, generator=gen), torch.rand(5, generator=gen) * 3 + 1e-3
    x = torch.randn(shape, generator=gen) * 3 + 1
    norm, denorm = cusrl.Normalization(mean.clone(), std.clone()), cusrl.Denormalization(mean.clone(), std.clone())
    assert not ops.column_affine_supported(x, mean, std)
    before = dict(_native.launch_counts)
    assert torch.equal(norm(x), (x - mean) / std) and torch.equal(denorm(x), x * std + mean)
    assert torch.equal(norm(x, done=None, sequential=False), (x - mean) / std)  # keyword arguments of a Sequential pass through
    assert torch.equal(ops.column_affine(x, mean, std), (x - mean) / std)
    assert torch.equal(ops.column_affine(x, mean, std, inverse=True), x * std + mean)
    assert _native.launch_counts == before
    # a round trip comes back within the two roundings of each direction
    back = denorm(norm(x))
    assert torch.allclose(back, x, rtol=4 * torch.finfo(torch.float32).eps, atol=4 * torch.finfo(torch.float32).eps * float(mean.abs().max()))
    # the gradients are torch's autograd: dy / std and dy * std, none for the statistics
    leaf = x.clone().requires_grad_(True)
    dy = torch.randn(shape, generator=gen)
    (dx,) = torch.autograd.grad(norm(leaf), leaf, grad_outputs=dy)
    assert torch.equal(dx, dy / std)
    (dx,) = torch.autograd.grad(denorm(leaf), leaf, grad_outputs=dy)
    assert torch.equal(dx, dy * std)


def test_state_dict_keys_are_the_references(cusrl, golden):
    g = golden("sequential")
    module = _sequential.build_module(cusrl)
    assert list(module.state_dict()) == [str(k) for k in g["state_keys"]]
    assert {"layers.0.mean", "layers.0.std", "layers.4.mean", "layers.4.std"} <= set(module.state_dict())
    module.load_state_dict(_sequential.golden_state(g), strict=True)
    for key, value in module.state_dict().items():
        assert torch.equal(value, torch.from_numpy(g["state/" + key])), key
    assert module.is_recurrent and (module.input_dim, module.output_dim) == (6, 4)


@pytest.mark.parametrize("prefix", ["plain_", "step_"])
def test_cpu_run_reproduces_the_reference(cusrl, golden, prefix):
    """The same torch, the same ops: exact.  (The two recorded calls with ``done`` need the done-split sequence layout, which
    this project has on the device only: tests/test_sequential_gpu.py replays them.)"""
    g = golden("sequential")
    module = _sequential.golden_module(cusrl, g)
    output, memory, keys, grad = _sequential.run_call(module, g, prefix)
    assert keys == [str(k) for k in g[prefix + "repr_keys"]] == REPR_KEYS
    assert np.array_equal(output.numpy(), g[prefix + "output"])
    assert sorted(memory) == [str(k) for k in g[prefix + "memory_keys"]] == ["2"]
    assert np.array_equal(memory["2"].detach().numpy(), g[prefix + "memory/2"])
    assert np.array_equal(grad.numpy(), g[prefix + "grad_input"])
    assert output.shape == ((5, 3, 4) if prefix == "plain_" else (3, 4))
    # step_memory is the forward's memory
    kwargs = {} if prefix == "plain_" else {"sequential": False}
    observation = torch.from_numpy(g["input"].copy())
    stepped = module.step_memory(observation if prefix == "plain_" else observation[0], {"2": torch.from_numpy(g["initial_memory/2"].copy())}, **kwargs)
    assert np.array_equal(stepped["2"].detach().numpy(), g[prefix + "memory/2"])


def test_both_constructor_forms_and_the_factory(cusrl):
    a, b, c = cusrl.Mlp(6, [8]), cusrl.Mlp(8, [5]), cusrl.Mlp(5, [], 3)
    for module in (cusrl.Sequential(a, b, c), cusrl.Sequential([a, b, c]), cusrl.Sequential(iter([a, b, c]))):
        assert list(module.layers) == [a, b, c] and (module.input_dim, module.output_dim) == (6, 3) and not module.is_recurrent
        assert module(torch.zeros(2, 6)).shape == (2, 3)
    assert list(cusrl.Sequential(a).layers) == [a]
    with pytest.raises(AssertionError):
        cusrl.Sequential([a], b)

    factories = [cusrl.Normalization.Factory([0.0] * 6, [1.0] * 6), cusrl.Mlp.Factory([8], ends_with_activation=True),
                 cusrl.Gru.Factory("gru", hidden_size=7), cusrl.Mlp.Factory([])]
    module = cusrl.Sequential.Factory(factories, hidden_dims=[None, None, None])(6, 4)
    assert [type(layer).__name__ for layer in module.layers] == ["Normalization", "Mlp", "Rnn", "Mlp"]
    assert [(layer.input_dim, layer.output_dim) for layer in module.layers] == [(6, 6), (6, 8), (8, 7), (7, 4)]
    assert module.is_recurrent and (module.input_dim, module.output_dim) == (6, 4)
    chained = cusrl.Sequential.Factory([cusrl.Mlp.Factory([8]), cusrl.Mlp.Factory([8])], hidden_dims=[5])(6, 2)
    assert [(layer.input_dim, layer.output_dim) for layer in chained.layers] == [(6, 5), (5, 2)]
    for hidden_dims in ([], [5], [5, 5, 5]):  # three factories want two hidden dims (`zip(..., strict=True)`)
        with pytest.raises(ValueError, match="zip\\(\\)"):
            cusrl.Sequential.Factory([cusrl.Mlp.Factory([8])] * 3, hidden_dims=hidden_dims)(6, 4)
    with pytest.raises(ValueError, match="Input dimension mismatch: expected 6, got 5"):
        cusrl.Sequential.Factory(factories, hidden_dims=[None, None, None])(5, 4)
    # Actor and Value take it like any backbone factory; the one-launch inference path does not match it
    from cusrl_amd.nn.module import fused_inference_layers

    factory = cusrl.Sequential.Factory(factories[:2], hidden_dims=[None])
    actor = cusrl.Actor.Factory(factory, cusrl.NormalDist.Factory())(6, 2)
    critic = cusrl.Value.Factory(factory)(6, 1)
    assert isinstance(actor.backbone, cusrl.Sequential) and isinstance(critic.backbone, cusrl.Sequential)
    assert critic(torch.zeros(3, 6))[0].shape == (3, 1)
    with torch.no_grad():
        assert fused_inference_layers(actor.backbone, actor.distribution.mean_head, torch.zeros(3, 6)) is None


def test_keyword_arguments_reach_every_layer_and_reprs_are_prefixed(cusrl):
    seen = []

    class Probe(cusrl.Module):
        def __init__(self, dim, recurrent=False):
            super().__init__(dim, dim, is_recurrent=recurrent)

        def forward(self, input, memory=None, **kwargs):
            seen.append((self.is_recurrent, memory, dict(kwargs)))
            self.intermediate_repr["latent"] = input + 1
            return (input * 2, None if memory is None else memory + 1) if self.is_recurrent else input * 2

    module = cusrl.Sequential(Probe(3), Probe(3, True), Probe(3, True), Probe(3))
    x, marker = torch.ones(2, 3), object()
    output, memory = module(x, memory={"1": torch.zeros(2, 1)}, done=marker, sequential=False)
    assert torch.equal(output, x * 16)
    assert [(r, k) for r, _, k in seen] == [(r, {"done": marker, "sequential": False}) for r in (False, True, True, False)]
    assert seen[0][1] is None and torch.equal(seen[1][1], torch.zeros(2, 1)) and seen[2][1] is None
    assert list(memory) == ["1"] and torch.equal(memory["1"], torch.ones(2, 1))  # a layer that returned no memory leaves no key
    assert list(module.intermediate_repr) == ["0/Probe.output", "0/Probe.latent", "1/Probe.output", "1/Probe.latent",
                                              "2/Probe.output", "2/Probe.latent", "3/Probe.output", "3/Probe.latent"]
    assert torch.equal(module.intermediate_repr["1/Probe.latent"], x * 2 + 1)
    module.clear_intermediate_repr()
    assert not module.intermediate_repr and all(not layer.intermediate_repr for layer in module.layers)
    assert module(x)[1] == {}  # no memory in, none out of these layers


def test_reset_memory_zeroes_only_the_recurrent_layers_rows_of_done_envs(cusrl, golden):
    module = _sequential.golden_module(cusrl, golden("sequential"))
    other = torch.full((3, 8), 7.0)
    memory = {"2": torch.arange(24, dtype=torch.float32).reshape(3, 8) + 1, "0": other}  # ("0" is not a recurrent layer's key)
    before = memory["2"].clone()
    module.reset_memory(memory, torch.tensor([[False], [True], [False]]))
    assert torch.equal(memory["2"][[0, 2]], before[[0, 2]]) and torch.equal(memory["2"][1], torch.zeros(8))
    assert torch.equal(other, torch.full((3, 8), 7.0))
    module.reset_memory(None, torch.tensor([[True]] * 3))  # nothing to reset
    module.reset_memory(memory)
    assert torch.equal(memory["2"], torch.zeros(3, 8)) and torch.equal(other, torch.full((3, 8), 7.0))
    feed_forward = cusrl.Sequential(cusrl.Mlp(4, [4]))
    feed_forward.reset_memory({"0": other}, None)
    assert torch.equal(other, torch.full((3, 8), 7.0))


def test_batch_invariant_propagates(cusrl):
    norm = cusrl.Normalization(torch.zeros(6), torch.ones(6))
    assert cusrl.Sequential(norm, cusrl.Mlp(6, [8])).batch_invariant is True
    assert cusrl.Sequential(norm, cusrl.Simba(6, 8)).batch_invariant is False
    assert cusrl.Sequential(cusrl.Sequential(cusrl.Simba(6)), cusrl.Mlp(6, [8])).batch_invariant is False


def test_the_optimizer_never_sees_the_statistics(cusrl):
    """``mean`` and ``std`` are parameters (they travel with the state dict) but not trainable: the optimizer's groups, and with
    them the flat gradient buffer, hold neither, and an update leaves their bits alone."""
    cusrl.set_global_seed(3)
    env = cusrl.testing.DummyTorchEnvironment(num_instances=8, observation_dim=6, action_dim=2, device="cpu")
    factory = cusrl.preset.PpoAgentFactory(num_steps_per_update=4, sampler_epochs=1, sampler_mini_batches=2, device="cpu").to_underlying()
    mean, std = torch.linspace(-1, 1, 6), torch.linspace(0.5, 2, 6)
    factory.actor_factory.backbone_factory = cusrl.Sequential.Factory(
        [cusrl.Normalization.Factory(mean, std), cusrl.Mlp.Factory([16], ends_with_activation=True)], hidden_dims=[None])
    agent = factory.from_environment(env)
    statistics = {name: param for name, param in agent.named_parameters() if name.rsplit(".", 1)[-1] in ("mean", "std")
                  and "layers.0" in name}
    assert len(statistics) == 2 and all(not param.requires_grad for param in statistics.values())
    held = {id(param) for group in agent.optimizer.param_groups for param in group["params"]}
    names = [name for group in agent.optimizer.param_groups for name in group["param_names"]]
    assert not held & {id(param) for param in statistics.values()} and not set(names) & set(statistics)
    if agent.flat_gradients is not None:
        assert not {id(param) for param in agent.flat_gradients.params} & {id(param) for param in statistics.values()}
    # one optimizer step by hand (the agent's own update needs the device: tests/test_sequential_gpu.py repeats this check behind
    # agent.update()): the statistics keep their bits and get no gradient, the trainable parameters move
    initial = {name: param.detach().clone() for name, param in agent.named_parameters()}
    observation, _, _ = env.reset()
    dist_params, _ = agent.actor(observation)
    (dist_params["mean"].square().sum() + agent.critic.evaluate(observation).sum()).backward()
    agent.optimizer.step()
    for name, param in statistics.items():
        assert torch.equal(param, initial[name]) and param.grad is None, name
    moved = [name for name, param in agent.named_parameters() if not torch.equal(param, initial[name])]
    assert moved and not set(moved) & set(statistics)
