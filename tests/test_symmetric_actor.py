"""The symmetric actor without a GPU: the float64 restatement of its head kernels (tests/_symmetric_actor.py) against the
reference's recorded run (golden ``symmetric_actor.npz``) — here the restatement is what is tested, the reference the yardstick —
and the host logic of ``SymmetricArchitecture`` / ``SymmetricActorFactory`` / ``SymmetricActor`` and of the ops wrappers."""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _symmetric_actor as restated

TAGS = ("normal", "adaptive")


@pytest.fixture(scope="module")
def cusrl():
    import cusrl_amd

    return cusrl_amd


def _network64(g, tag):
    """The wrapped actor over the stacked rows in float64 torch: (parameters by name, mean2, std operand, std2 rows)."""
    params = {str(n): torch.from_numpy(g[f"{tag}_param/{n}"]).double().requires_grad_(True) for n in g[tag + "_param_names"]}
    dest, mult = g["observation_dest"], restated.multiplier(g["observation_dest"], g["observation_flipped"])
    observation = g[tag + "_observation"].astype(np.float64)
    stacked = torch.from_numpy(np.concatenate([observation, observation[:, dest] * mult]))
    hidden = torch.relu(stacked @ params["backbone.layers.0.weight"].t() + params["backbone.layers.0.bias"])
    latent = torch.relu(hidden @ params["backbone.layers.2.weight"].t() + params["backbone.layers.2.bias"])
    mean2 = latent @ params["distribution.mean_head.weight"].t() + params["distribution.mean_head.bias"]
    if tag == "normal":
        std2 = params["distribution.std.param"]  # (identity bijector: the [A] vector itself)
    else:
        raw = latent @ params["distribution.std_head.weight"].t() + params["distribution.std_head.bias"]
        std2 = torch.exp(raw.clamp(np.log(0.01), np.log(1.0)))
    return params, mean2, std2


@pytest.mark.parametrize("tag", TAGS)
def test_restated_combine_reproduces_the_reference_forward(golden, tag):
    g = golden("symmetric_actor")
    _, mean2, std2 = _network64(g, tag)
    mean, std = restated.combine64(mean2.detach().numpy(), std2.detach().numpy(), g["action_dest"], g["action_flipped"])
    np.testing.assert_allclose(mean, g[tag + "_mean"], rtol=1e-6, atol=1e-6 * np.abs(g[tag + "_mean"]).max())
    np.testing.assert_allclose(std, g[tag + "_std"], rtol=1e-6)
    # deterministic acting = the combined mean, its log-prob and compute_logp at the recorded action
    np.testing.assert_allclose(mean, g[tag + "_deterministic_action"], rtol=1e-6, atol=1e-6 * np.abs(mean).max())
    # (a log-prob is a sum of A terms that cancel: 1e-6 relative to their summed magnitudes, the yardstick's own fp32 rounding)
    for action, key in ((mean, "_deterministic_logp"), (g[tag + "_action"], "_compute_logp")):
        bound = 1e-6 * restated.normal_logp_magnitude64(mean, std, action)
        assert (np.abs(restated.normal_logp64(mean, std, action) - g[tag + key]) <= bound).all(), key
    # ... and the sample restatement is the same log-prob at action = mean + std * eps
    eps = np.random.default_rng(0).standard_normal(mean.shape).astype(np.float32)
    action, logp = restated.sample64(mean, std, eps)
    np.testing.assert_allclose(logp, restated.normal_logp64(mean, std, action), rtol=1e-12)


@pytest.mark.parametrize("tag", TAGS)
def test_restated_backward_reproduces_the_reference_gradients(golden, tag):
    g = golden("symmetric_actor")
    params, mean2, std2 = _network64(g, tag)
    dest, flipped, B = g["action_dest"], g["action_flipped"], g[tag + "_observation"].shape[0]
    d_o, d_m, _, _ = restated.combine_backward64(g[tag + "_c1"], None, dest, flipped, through_abs=False)
    d_mean2 = torch.from_numpy(np.concatenate([d_o, d_m]))
    std_values = std2.detach().numpy()
    std_m = np.broadcast_to(std_values, (B, len(dest))) if std_values.ndim == 1 else std_values[B:]
    s_o, s_m, _, _ = restated.combine_backward64(g[tag + "_c2"], std_m, dest, flipped, through_abs=True)
    d_std2 = torch.from_numpy((s_o + s_m).sum(axis=0) if std_values.ndim == 1 else np.concatenate([s_o, s_m]))
    names = list(params)
    grads = torch.autograd.grad([mean2, std2], [params[n] for n in names], [d_mean2, d_std2])
    for name, grad in zip(names, grads):
        expected = g[f"{tag}_grad/{name}"]
        np.testing.assert_allclose(grad.numpy(), expected, rtol=1e-6, atol=1e-6 * np.abs(expected).max(), err_msg=name)


def test_backward_restatement_counts_readers_and_zeroes_unread_columns():
    dest, flipped = [2, 0, 0, 1], [1, 3]
    g = np.arange(8, dtype=np.float64).reshape(2, 4) + 1
    d_o, d_m, magnitudes, counts = restated.combine_backward64(g, None, dest, flipped, through_abs=False)
    assert counts.tolist() == [2, 1, 1, 0] and np.array_equal(d_o, g / 2)
    assert np.array_equal(d_m[:, 0], -g[:, 1] / 2 + g[:, 2] / 2) and np.array_equal(d_m[:, 3], np.zeros(2))
    assert np.array_equal(magnitudes[:, 0], (g[:, 1] + g[:, 2]) / 2)
    std_m = np.array([[0.0, -1.0, 2.0, 5.0], [-0.0, 3.0, -2.0, 5.0]])
    _, s_m, _, _ = restated.combine_backward64(g, std_m, dest, flipped, through_abs=True)
    assert np.array_equal(s_m[:, 0], np.zeros(2))  # sgn(0) = 0
    assert np.array_equal(s_m[:, 1], np.array([-g[0, 3] / 2, g[1, 3] / 2]))  # sgn(-x) * -1 * g / 2


# ------------------------------------------------------------------------------------------------ host logic
def test_the_three_names_are_exported(cusrl):
    import cusrl_amd.hook.auxiliary as auxiliary

    for name in ("SymmetricActor", "SymmetricActorFactory", "SymmetricArchitecture"):
        assert name in cusrl.hook.__all__ and name in auxiliary.__all__
        assert getattr(cusrl.hook, name) is getattr(auxiliary, name) is getattr(auxiliary.symmetry, name)


def test_abi_version_stays_and_the_new_symbols_are_declared():
    from cusrl_amd import _native

    assert _native.ABI_VERSION == 7
    for symbol in ("cusrl_symmetric_head_fwd", "cusrl_symmetric_head_bwd", "cusrl_symmetric_head_sample"):
        assert symbol in _native.EXPORTED_SYMBOLS


def test_pre_init_replaces_the_actor_factory(cusrl):
    from cusrl_amd.hook import MirrorDef, SymmetricActor, SymmetricActorFactory, SymmetricArchitecture
    from cusrl_amd.nn.actor import Actor

    underlying = cusrl.preset.PpoAgentFactory(actor_hidden_dims=(32, 16), critic_hidden_dims=(32, 16)).to_underlying()
    original = underlying.actor_factory
    mirrors = MirrorDef([1, 0, 2, 3], [2]), MirrorDef([1, 0], [])
    spec = cusrl.EnvironmentSpec(4, 2, num_instances=3, mirror_observation=mirrors[0], mirror_action=mirrors[1])
    agent = SimpleNamespace(actor_factory=original, environment_spec=spec)
    SymmetricArchitecture().pre_init(agent)
    factory = agent.actor_factory
    assert isinstance(factory, SymmetricActorFactory) and isinstance(factory, Actor.Factory)
    assert factory.backbone_factory is original.backbone_factory and factory.distribution_factory is original.distribution_factory
    assert factory.latent_dim == original.latent_dim
    assert factory.mirror_observation is mirrors[0] and factory.mirror_action is mirrors[1]
    actor = factory(4, 2)
    assert isinstance(actor, SymmetricActor) and isinstance(actor.wrapped, Actor) and actor.wrapped.backbone is actor.backbone
    assert actor.noise_shape is None and actor.step_memory(torch.zeros(3, 4)) is None and actor.reset_memory(None) is None
    with pytest.raises(AssertionError, match="'mirror_observation' must be defined"):
        SymmetricActorFactory(original.backbone_factory, original.distribution_factory)(4, 2)


def test_the_three_error_cases_raise(cusrl):
    from cusrl_amd.hook import MirrorDef, SymmetricActor
    from cusrl_amd.nn.actor import Actor
    from cusrl_amd.nn.distribution import NormalDist, OneHotCategoricalDist
    from cusrl_amd.nn.module import Mlp
    from cusrl_amd.nn.rnn import Rnn

    mirrors = MirrorDef([1, 0, 2, 3], [2]), MirrorDef([1, 0], [])
    backbone = Mlp.Factory((8,), ends_with_activation=True)
    with pytest.raises(ValueError, match="SymmetricActor can only be used with Normal distributions"):
        SymmetricActor(Actor.Factory(backbone, OneHotCategoricalDist.Factory())(4, 2), *mirrors)
    recurrent = Actor.Factory(Rnn.Factory("GRU", hidden_size=8), NormalDist.Factory())(4, 2)
    assert recurrent.is_recurrent
    with pytest.raises(NotImplementedError, match="recurrent"):
        SymmetricActor(recurrent, *mirrors)
    plain = Actor.Factory(backbone, NormalDist.Factory())(4, 2)
    with pytest.raises(TypeError, match="must be a MirrorDef"):
        SymmetricActor(plain, ([1, 0, 2, 3], [2]), mirrors[1])  # the definition's arguments, not a MirrorDef
    with pytest.raises(TypeError, match="must be a MirrorDef"):
        SymmetricActor(plain, mirrors[0], None)


@pytest.mark.parametrize("tag", TAGS)
def test_host_form_follows_the_reference_and_carries_its_keys(cusrl, golden, tag):
    g = golden("symmetric_actor")
    actor = restated.golden_actor(cusrl, g, tag)
    observation = torch.from_numpy(g[tag + "_observation"])
    action_dist, memory = actor(observation)
    assert memory is None
    np.testing.assert_allclose(action_dist["mean"].detach().numpy(), g[tag + "_mean"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(action_dist["std"].detach().numpy(), g[tag + "_std"], rtol=1e-5)
    assert sorted(actor.intermediate_repr) == ["mirrored.action_dist", "mirrored.backbone.output", "mirrored.observation",
                                               "original.action_dist", "original.backbone.output"]
    assert torch.equal(actor.intermediate_repr["mirrored.observation"], actor.mirror_observation(observation))
    with torch.no_grad():
        _, (action, logp), _ = actor.explore(observation, deterministic=True)
    np.testing.assert_allclose(action.numpy(), g[tag + "_deterministic_action"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(logp.numpy(), g[tag + "_deterministic_logp"], rtol=1e-5)


def test_a_user_callable_is_evaluated_as_given(cusrl, golden):
    from cusrl_amd.hook import SymmetricActor

    g = golden("symmetric_actor")
    reference = restated.golden_actor(cusrl, g, "normal")
    calls = []

    def mirror_action(action):
        calls.append(tuple(action.shape))
        return reference.mirror_action(action)

    actor = SymmetricActor(reference.wrapped, lambda observation: reference.mirror_observation(observation), mirror_action)
    action_dist, _ = actor(torch.from_numpy(g["normal_observation"]))
    np.testing.assert_allclose(action_dist["mean"].detach().numpy(), g["normal_mean"], rtol=1e-5, atol=1e-6)
    assert calls == [(5, 8), (5, 8)]  # the mean's and the std's mirrored half


def test_ops_wrappers_refuse_a_wrong_table_on_the_host(cusrl):
    from cusrl_amd import _native, ops
    from cusrl_amd.hook import MirrorDef

    mirror = MirrorDef([1, 0, 2], [0])
    right, wrong = torch.from_numpy(mirror.host_table(3)), torch.from_numpy(mirror.host_table(5))
    mean2, std2, eps, g_out = torch.randn(8, 3), torch.rand(8, 3) + 0.1, torch.randn(4, 3), torch.randn(4, 3)
    before = dict(_native.launch_counts)
    for table, error in ((wrong, ValueError), (right.long(), TypeError), (right.float(), TypeError)):
        with pytest.raises(error, match="mirror table"):
            ops.symmetric_head_fwd(mean2, std2, table)
        with pytest.raises(error, match="mirror table"):
            ops.symmetric_head_sample(mean2, std2, table, eps)
        with pytest.raises(error, match="mirror table"):
            ops.symmetric_head_bwd(g_out, g_out, std2, table)
    with pytest.raises(ValueError, match=r"\[2B, A\]"):
        ops.symmetric_head_fwd(torch.randn(7, 3), std2, right)
    with pytest.raises(ValueError, match="std must be"):
        ops.symmetric_head_fwd(mean2, torch.rand(4), right)
    assert _native.launch_counts == before  # nothing reached the library
    assert ops.symmetric_head_supported(4096, 12) and ops.symmetric_head_supported(0, 1)
    assert not ops.symmetric_head_supported(4, _native.MAX_SYMMETRIC_HEAD_ACTIONS + 1) and not ops.symmetric_head_supported(2**28, 12)
