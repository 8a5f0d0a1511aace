"""Policy distillation without a GPU: the stub modules and the experts of golden ``distillation.npz`` (recorded from the
reference, tests/golden/make_distillation_golden.py), ``ExpertPolicy`` construction and its file format, the hook's arguments
and what it writes into a transition, and the preset's composition."""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest
import torch
from torch import nn

import _bijectors
import _distillation as shared

# Against the RECORDED float32 outputs: the CPU's GEMM sums in an order of its own (ISA, thread count), so another machine's fp32
# bits may differ in the last place.  The fixture's own float32 is within 2e-7 of its float64 in units of the largest entry;
# 1e-6 holds every summation order and is a tenth of the package's parity bar.  Bit equality is asserted against the same
# expression evaluated by torch on the machine the test runs on.
RECORDED = 1e-6


@pytest.fixture(scope="module")
def cusrl():
    import cusrl_amd

    return cusrl_amd


@pytest.fixture(scope="module")
def g(golden):
    return golden("distillation")


# ------------------------------------------------------------------------------------------------ stub modules
def test_stub_module_matches_the_reference(cusrl, g):
    x = torch.from_numpy(g["stub/input"])
    default = cusrl.StubModule.Factory()(7, None)
    assert (default.input_dim, default.output_dim, default.is_recurrent) == (7, 1, False)
    assert np.array_equal(default(x).numpy(), g["stub/default"]) and default(x).shape == (2, 5, 1)
    four = cusrl.nn.StubModule(7, 4)
    assert np.array_equal(four(x, memory=None).numpy(), g["stub/four"]) and four(x).dtype == x.dtype
    assert not list(four.parameters())
    with pytest.raises(AssertionError):
        cusrl.StubModule.Factory()(None, 3)


def test_identity_matches_the_reference(cusrl, g):
    x = torch.from_numpy(g["stub/input"])
    identity = cusrl.Identity.Factory()(7, None)
    assert identity(x) is x and np.array_equal(identity(x).numpy(), g["stub/identity"])
    assert (identity.input_dim, identity.output_dim) == (7, 7)
    assert cusrl.nn.Identity.Factory()(7, 7).output_dim == 7
    with pytest.raises(AssertionError):
        cusrl.Identity.Factory()(7, 6)
    with pytest.raises(AssertionError):
        cusrl.Identity(7, 6)
    with pytest.raises(AssertionError):
        cusrl.Identity.Factory()(None, None)


# ------------------------------------------------------------------------------------------------ ExpertPolicy
@pytest.mark.parametrize("activation", shared.ACTIVATIONS)
def test_host_form_equals_the_reference_float32_outputs(cusrl, g, activation):
    *_, observation, output32, _ = shared.tensors(g, activation)
    expert = shared.native_expert(cusrl, g, activation)
    got = expert(observation)
    assert not got.requires_grad and got.dtype == torch.float32
    with torch.no_grad():
        assert torch.equal(got, shared.teacher(g, activation)(observation)), "not the bits of torch's expression on this machine"
    assert _bijectors.relative_to_largest(got, output32) <= RECORDED
    assert expert.reset(torch.zeros(observation.shape[0], dtype=torch.bool)) is None


def _actor(cusrl, activation="ELU", dropout=0.0, ends_with_activation=True):
    torch.manual_seed(5)
    return cusrl.Actor.Factory(cusrl.Mlp.Factory(shared.HIDDEN, activation, ends_with_activation, dropout),
                               cusrl.NormalDist.Factory())(shared.K, shared.A)


@pytest.mark.parametrize("activation", shared.ACTIVATIONS)
def test_from_actor_round_trips_through_save_and_load(cusrl, tmp_path, activation):
    actor = _actor(cusrl, activation)
    normalizer = cusrl.RunningMeanStd(shared.K, clamp=4.0, excluded_indices=[2])
    normalizer.update(torch.randn(64, shared.K) * 3 + 1)
    expert = cusrl.ExpertPolicy.from_actor(actor, normalizer)
    assert (expert.activation, expert.clamp, expert.epsilon, expert.num_layers) == (activation, 4.0, 1e-8, 3)
    assert all(not b.requires_grad and b.dtype == torch.float32 for b in expert.buffers()) and not list(expert.parameters())
    observation = torch.randn(9, shared.K) * 5
    with torch.no_grad():
        expected = actor(normalizer.normalize(observation))[0]["mean"]
    assert torch.equal(expert(observation), expected)
    assert expert.mean[2] == 0 and torch.equal(expert.std, normalizer.std)  # an excluded channel: mean 0, std sqrt(1 + epsilon)
    before = [p.detach().clone() for p in actor.parameters()]
    with torch.no_grad():
        for p in actor.parameters():
            p.add_(1.0)  # the expert holds copies
    assert torch.equal(expert(observation), expected) and all(not torch.equal(a, b) for a, b in zip(actor.parameters(), before))

    path = tmp_path / "expert.pt"
    expert.save(path)
    data = torch.load(path, weights_only=True)
    assert data["spec"] == {"format": "cusrl_amd.expert", "version": 1, "activation": activation, "alpha": 1.0, "clamp": 4.0,
                            "epsilon": 1e-8, "num_layers": 3, "normalized": True}
    assert all(isinstance(t, torch.Tensor) for t in data["tensors"].values())
    loaded = cusrl.ExpertPolicy.load(path, map_location="cpu")
    assert torch.equal(loaded(observation), expected) and loaded.spec() == expert.spec()
    plain = cusrl.ExpertPolicy.from_actor(_actor(cusrl, activation))
    plain.save(path)
    assert cusrl.ExpertPolicy.load(path).mean is None


def test_from_actor_keeps_the_elu_alpha(cusrl):
    actor = _actor(cusrl, "ELU")
    for layer in actor.backbone.layers:
        if isinstance(layer, nn.ELU):
            layer.alpha = 0.5
    expert = cusrl.ExpertPolicy.from_actor(actor)
    observation = torch.randn(6, shared.K) * 4
    with torch.no_grad():
        assert torch.equal(expert(observation), actor(observation)[0]["mean"])
    assert expert.alpha == 0.5


def test_from_actor_refuses_what_it_cannot_freeze(cusrl):
    with pytest.raises(ValueError, match="Dropout"):
        cusrl.ExpertPolicy.from_actor(_actor(cusrl, dropout=0.1))
    recurrent = cusrl.Actor.Factory(cusrl.Rnn.Factory("GRU", num_layers=1, hidden_size=8), cusrl.NormalDist.Factory())(shared.K, shared.A)
    with pytest.raises(ValueError, match="recurrent backbone Rnn"):
        cusrl.ExpertPolicy.from_actor(recurrent)
    mixed = _actor(cusrl, "ELU")
    mixed.backbone.layers[3] = nn.Tanh()
    with pytest.raises(ValueError, match=r"mixed activations ELU\(alpha=1.0\), Tanh\(\)"):
        cusrl.ExpertPolicy.from_actor(mixed)
    with pytest.raises(ValueError, match="GELU"):
        cusrl.ExpertPolicy.from_actor(_actor(cusrl, "GELU"))
    with pytest.raises(ValueError, match="ends_with_activation=False"):
        cusrl.ExpertPolicy.from_actor(_actor(cusrl, ends_with_activation=False))
    headless = SimpleNamespace(backbone=_actor(cusrl).backbone, distribution=nn.Softmax(-1))
    with pytest.raises(ValueError, match="found Softmax with mean_head NoneType"):
        cusrl.ExpertPolicy.from_actor(headless)
    with pytest.raises(ValueError, match="RunningMeanStd; found Linear"):
        cusrl.ExpertPolicy.from_actor(_actor(cusrl), nn.Linear(2, 2))


def test_load_refuses_other_files(cusrl, g, tmp_path):
    scripted = shared.scripted_expert_file(g, "Tanh", tmp_path)
    assert cusrl.ExpertPolicy.try_load(scripted) is None
    with pytest.raises(ValueError, match="not a file in the 'cusrl_amd.expert' format"):
        cusrl.ExpertPolicy.load(scripted)
    pickled = tmp_path / "module.pt"
    torch.save(nn.Linear(2, 2), pickled)  # a pickle that needs code to load: never unpickled
    assert cusrl.ExpertPolicy.try_load(pickled) is None
    other = tmp_path / "other.pt"
    torch.save({"spec": {"format": "something else"}}, other)
    assert cusrl.ExpertPolicy.try_load(other) is None


# ------------------------------------------------------------------------------------------------ the hook
def _hook(cusrl, *args, **kwargs):
    hook = cusrl.hook.PolicyDistillation(*args, **kwargs)
    hook.pre_init(SimpleNamespace(device=torch.device("cpu")))
    return hook


def test_hook_argument_errors_carry_the_reference_message(cusrl, g, tmp_path):
    for hook in (_hook(cusrl), _hook(cusrl, ""), _hook(cusrl, "some/path.pt", expert=shared.native_expert(cusrl, g, "ReLU"))):
        with pytest.raises(ValueError, match="^'expert_path' cannot be empty$"):
            hook.init()
    hook = cusrl.hook.PolicyDistillation("a.pt", "state", 0.25)  # the reference's positional signature
    assert (hook.expert_path, hook.observation_name, hook.weight, hook.target_name) == ("a.pt", "state", 0.25, "expert_action")
    assert hook.name == "policy_distillation" and "weight" in hook._mutable
    with pytest.raises(TypeError):
        cusrl.hook.PolicyDistillation("a.pt", "state", 0.25, nn.Linear(1, 1))  # `expert` is keyword-only


class _Recording(nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner, self.resets = inner, []

    def forward(self, observation):
        return self.inner(observation)

    def reset(self, done):
        self.resets.append(done)


@pytest.mark.parametrize("activation", shared.ACTIVATIONS)
def test_scripted_and_native_experts_write_the_same_expert_action(cusrl, g, tmp_path, activation):
    *_, observation, output32, _ = shared.tensors(g, activation)
    done = torch.rand(observation.shape[0], 1) < 0.3
    native_file = tmp_path / "native.pt"
    shared.native_expert(cusrl, g, activation).save(native_file)
    hooks = {
        "scripted": _hook(cusrl, shared.scripted_expert_file(g, activation, tmp_path)),
        "native": _hook(cusrl, expert=shared.native_expert(cusrl, g, activation)),
        "native file": _hook(cusrl, str(native_file)),
        "module": _hook(cusrl, expert=_Recording(shared.teacher(g, activation))),
    }
    written = {}
    for name, hook in hooks.items():
        hook.init()
        transition = {"observation": observation.clone(), "done": done.clone()}
        hook.post_step(transition)
        written[name] = transition["expert_action"]
        assert not written[name].requires_grad, name
        assert torch.equal(written[name], written["scripted"]), f"{name}: not what the TorchScript expert writes"
        assert _bijectors.relative_to_largest(written[name], output32) <= RECORDED, name
        assert hook.native_expert == name.startswith("native")
        assert hook.rollout_capture_safe == hook.post_step_device_free == name.startswith("native")
        assert hook.eager_phases() == (() if name.startswith("native") else ("step",))
        assert not list(hook.parameters()) and hook.state_dict() == {}  # neither optimised nor checkpointed
    assert isinstance(hooks["scripted"].expert, torch.jit.ScriptModule)
    assert isinstance(hooks["native file"].expert, cusrl.ExpertPolicy)
    (mask,) = hooks["module"].expert.resets
    assert mask.shape == (observation.shape[0],) and torch.equal(mask, done.squeeze(-1))


def test_hook_reads_the_named_observation_and_keeps_the_inherited_objective(cusrl, g):
    *_, observation, output32, _ = shared.tensors(g, "ELU")
    hook = _hook(cusrl, "", "state", 2.0, expert=shared.native_expert(cusrl, g, "ELU"))
    hook.init()
    transition = {"observation": torch.zeros_like(observation), "state": observation, "done": torch.zeros(observation.shape[0], 1, dtype=torch.bool)}
    hook.post_step(transition)
    assert _bijectors.relative_to_largest(transition["expert_action"], output32) <= RECORDED
    assert type(hook).objective is cusrl.hook.PolicyDistillationLoss.objective
    mean = (output32 + 0.5).requires_grad_()
    loss = hook.objective({}, {"curr_action_dist": {"mean": mean}, "expert_action": output32})["distillation_loss"]
    assert float(loss) == pytest.approx(0.5, rel=1e-5)  # weight 2 x mean(0.5 ** 2)


# ------------------------------------------------------------------------------------------------ the preset
def test_preset_builds_the_reference_hook_list(cusrl, g):
    expert = shared.native_expert(cusrl, g, "ELU")
    underlying = shared.factory(cusrl, "cpu", expert=expert).to_underlying()
    assert [hook.name for hook in underlying.hooks] == [str(name) for name in g["trace_hooks"]]
    assert [hook.name for hook in cusrl.preset.distillation_hook_suite("x.pt", normalize_observation=True)] == [
        "observation_normalization", "on_policy_preparation", "policy_distillation", "gradient_clipping"]
    suite = cusrl.preset.distillation_hook_suite("x.pt", "state", False, None)
    assert (suite[1].expert_path, suite[1].observation_name, suite[2].max_grad_norm) == ("x.pt", "state", None)
    factory = cusrl.preset.DistillationAgentFactory()
    assert (factory.num_steps_per_update, tuple(factory.actor_hidden_dims), factory.activation_fn, factory.lr, factory.sampler_epochs,
            factory.sampler_mini_batches, factory.init_distribution_std, factory.expert_path, factory.expert_observation_name,
            factory.normalize_observation, factory.max_grad_norm, factory.expert) == (
                24, (256, 128), "ReLU", 2e-4, 1, 8, None, "", "observation", False, 1.0, None)
    assert (underlying.optimizer_factory.defaults["lr"], underlying.sampler.num_epochs, underlying.sampler.num_mini_batches) == (2e-4, 1, 8)
    actor = underlying.actor_factory(shared.K, shared.A)
    critic = underlying.critic_factory(shared.K, 1)
    assert type(actor.backbone) is cusrl.Mlp and type(actor.backbone.layers[-1]) is nn.ReLU and type(actor.distribution) is cusrl.NormalDist
    assert type(critic.backbone) is cusrl.StubModule and critic.backbone.output_dim == 1
    names = [f"actor.{n}" for n, _ in actor.named_parameters()] + [f"critic.{n}" for n, _ in critic.named_parameters()]
    assert names == [str(name) for name in g["param_names"]]
