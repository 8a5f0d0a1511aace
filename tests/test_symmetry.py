"""Mirror symmetry on the host: MirrorDef and its device table, the hooks' constructors, validation and bookkeeping, and the
reference's results (tests/golden/symmetry.npz, make_symmetry_golden.py) through the host forms."""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cusrl_amd as cusrl
from cusrl_amd.hook import (
    MirrorDef,
    MirrorSymmetryLoss,
    ObservationNormalization,
    SymmetricDataAugmentation,
    TransitionMirroring,
)

DEF_NAMES = ("observation", "action", "state", "non_bijective")


def _def(golden, name):
    g = golden("symmetry")
    return MirrorDef(g[f"mirror_{name}_dest"].tolist(), g[f"mirror_{name}_flipped"].tolist())


@pytest.mark.parametrize("name", DEF_NAMES)
def test_mirror_def_matches_the_reference_bit_for_bit(golden, name):
    g = golden("symmetry")
    mirror = _def(golden, name)
    out = mirror(torch.from_numpy(g[f"mirror_{name}_in"]))
    expected = g[f"mirror_{name}_out"]
    assert out.numpy().view(np.uint32).tolist() == expected.view(np.uint32).tolist()  # signed zeros included
    assert repr(mirror) == str(g[f"mirror_{name}_repr"])


@pytest.mark.parametrize("name", DEF_NAMES)
def test_mirror_table_inverts_the_map(golden, name):
    g = golden("symmetry")
    mirror = _def(golden, name)
    c_in = g[f"mirror_{name}_in"].shape[1]
    table = mirror.host_table(c_in).view(np.uint32).astype(np.int64)
    c_out = mirror.output_dim
    assert table.size == 2 * c_out + c_in + 1
    codes, offsets, inverse = table[:c_out], table[c_out:c_out + c_in + 1], table[c_out + c_in + 1:]
    flip = 1 << 31
    dest = [int(c) & ~flip for c in codes]
    assert dest == [d % c_in for d in g[f"mirror_{name}_dest"].tolist()]
    flipped = {int(j) % c_out for j in g[f"mirror_{name}_flipped"]}
    assert [bool(c & flip) for c in codes] == [j in flipped for j in range(c_out)]
    for i in range(c_in):
        readers = [int(c) for c in inverse[offsets[i]:offsets[i + 1]]]
        assert [r & ~flip for r in readers] == [j for j in range(c_out) if dest[j] == i]
        assert all(bool(r & flip) == ((r & ~flip) in flipped) for r in readers)


def test_mirror_def_rejects_an_index_outside_the_input():
    with pytest.raises(IndexError):
        MirrorDef([0, 3], []).host_table(3)
    assert MirrorDef([-1, 0], [1]).host_table(3)[0] == 2  # negative indices count from the end, as in torch indexing


def _agent(spec, *, has_state, recurrent=False, device="cpu"):
    return SimpleNamespace(environment_spec=spec, has_state=has_state, device=torch.device(device), observation_dim=spec.observation_dim,
                           state_dim=spec.state_dim if has_state else spec.observation_dim, action_dim=spec.action_dim,
                           actor=SimpleNamespace(is_recurrent=recurrent), inference_mode=False, setup_module=lambda m: m,
                           to_tensor=torch.as_tensor)


def _spec(golden, *, state=True, **overrides):
    kwargs = dict(mirror_observation=_def(golden, "observation"), mirror_action=_def(golden, "action"),
                  mirror_state=_def(golden, "state") if state else None)
    kwargs.update(overrides)
    return cusrl.EnvironmentSpec(16, 8, state_dim=7 if state else None, num_instances=4, **kwargs)


def _init(hook, agent):
    hook.agent = agent
    hook.init()
    return hook


def test_transition_mirroring_matches_the_reference(golden):
    g = golden("symmetry")
    hook = _init(TransitionMirroring(), _agent(_spec(golden), has_state=True))
    transition = {"observation": torch.from_numpy(g["tm_in_observation"]), "state": torch.from_numpy(g["tm_in_state"])}
    hook.pre_act(transition)
    transition["action"] = torch.from_numpy(g["tm_in_action"])
    hook.post_act(transition)
    transition["next_observation"] = torch.from_numpy(g["tm_in_next_observation"])
    transition["next_state"] = torch.from_numpy(g["tm_in_next_state"])
    hook.post_step(transition)
    for key in ("observation", "state", "action", "next_observation", "next_state"):
        assert np.array_equal(transition[key].numpy(), g[f"tm_out_{key}"]), key


def test_transition_mirroring_known_answer():
    """The reference's own example: a swap with one flip, applied to observation, action and next observation."""
    spec = cusrl.EnvironmentSpec(2, 2, num_instances=1, mirror_observation=MirrorDef([1, 0], [0]),
                                 mirror_action=MirrorDef([1, 0], [1]))
    hook = _init(TransitionMirroring(), _agent(spec, has_state=False))
    transition = {"observation": torch.tensor([[1.0, 2.0]])}
    hook.pre_act(transition)
    assert transition["observation"].tolist() == [[-2.0, 1.0]]
    transition["action"] = torch.tensor([[3.0, 4.0]])
    hook.post_act(transition)
    assert transition["action"].tolist() == [[4.0, -3.0]]
    transition["next_observation"] = torch.tensor([[5.0, 6.0]])
    hook.post_step(transition)
    assert transition["next_observation"].tolist() == [[-6.0, 5.0]]


def test_transition_mirroring_index_range():
    spec = cusrl.EnvironmentSpec(2, 2, num_instances=1, mirror_observation=MirrorDef([1, 0], []),
                                 mirror_action=MirrorDef([1, 0], []))
    with pytest.raises(TypeError, match="'index' must be an int"):
        TransitionMirroring(index=0.5)
    for index in (0, -1):
        hook = _init(TransitionMirroring(index=index), _agent(spec, has_state=False))
        transition = {"observation": torch.tensor([[1.0, 2.0]])}
        hook.pre_act(transition)
        assert transition["observation"].tolist() == [[2.0, 1.0]]
    hook = _init(TransitionMirroring(index=1), _agent(spec, has_state=False))
    with pytest.raises(IndexError, match="Mirror index 1 is out of range for 1 symmetry transforms"):
        hook.pre_act({"observation": torch.tensor([[1.0, 2.0]])})


def test_constructor_validation_names_and_mutables():
    with pytest.raises(ValueError, match="'weight' must be None or non-negative"):
        MirrorSymmetryLoss(-0.1)
    loss = MirrorSymmetryLoss(0.5, symmetrize_action_std=True)
    assert loss.name == "mirror_symmetry_loss" and loss.weight == 0.5 and loss.symmetrize_action_std
    assert "weight" in loss._mutable
    augmentation = SymmetricDataAugmentation()
    assert augmentation.name == "symmetric_data_augmentation" and augmentation.augments_value and augmentation.training_only
    assert TransitionMirroring().name == "transition_mirroring" and TransitionMirroring.rollout_capture_safe


@pytest.mark.parametrize("missing, message", [("mirror_observation", "'mirror_observation' must be defined for symmetry hooks"),
                                              ("mirror_state", "'mirror_state' must be defined for symmetry hooks"),
                                              ("mirror_action", "'mirror_action' must be defined for symmetry hooks")])
@pytest.mark.parametrize("hook_type", [MirrorSymmetryLoss, SymmetricDataAugmentation, TransitionMirroring])
def test_missing_mirrors_are_refused(golden, hook_type, missing, message):
    hook = hook_type(0.5) if hook_type is MirrorSymmetryLoss else hook_type()
    with pytest.raises(ValueError, match=message):
        _init(hook, _agent(_spec(golden, **{missing: None}), has_state=True))


def test_recurrent_actors_and_unaugmented_values_are_refused(golden):
    for hook in (MirrorSymmetryLoss(0.5), SymmetricDataAugmentation()):
        with pytest.raises(NotImplementedError, match="recurrent"):
            _init(hook, _agent(_spec(golden), has_state=True, recurrent=True))
    with pytest.raises(ValueError, match="augments_value=False"):
        _init(SymmetricDataAugmentation(augments_value=False), _agent(_spec(golden), has_state=True))


def test_mirror_symmetry_loss_without_weight_is_inactive(golden):
    hook = _init(MirrorSymmetryLoss(None), _agent(_spec(golden), has_state=True))
    assert hook.objective({}, {}) is None


def test_augmentation_builds_the_reference_batch_on_the_host(golden):
    hook = _init(SymmetricDataAugmentation(), _agent(_spec(golden), has_state=True))
    gen = torch.Generator().manual_seed(3)
    batch = {"observation": torch.randn(5, 16, generator=gen), "next_observation": torch.randn(5, 16, generator=gen),
             "action": torch.randn(5, 8, generator=gen), "state": torch.randn(5, 7, generator=gen),
             "next_state": torch.randn(5, 7, generator=gen), "action_logp": torch.randn(5, 1, generator=gen),
             "advantage": torch.randn(5, 1, generator=gen), "value": torch.randn(5, 1, generator=gen),
             "return": torch.randn(5, 1, generator=gen)}
    original = dict(batch)
    hook.objective({"temporal": False}, batch)
    spec = hook.agent.environment_spec
    for key, mirror in (("observation", spec.mirror_observation), ("action", spec.mirror_action), ("next_state", spec.mirror_state)):
        assert batch[key].shape == (5, 2, original[key].shape[-1])
        assert torch.equal(batch[key][:, 0], original[key]) and torch.equal(batch[key][:, 1], mirror(original[key]))
    for key in ("action_logp", "advantage", "value", "return"):
        assert torch.equal(batch[key], original[key].unsqueeze(1).repeat_interleave(2, dim=1))


def test_observation_normalization_accepts_mirrors(golden):
    """Used to raise NotImplementedError for any mirrored spec; the host form follows the reference's formula."""
    g = golden("symmetry")
    for case, with_state in (("s", True), ("o", False)):
        spec = _spec(golden, state=with_state)
        spec.num_instances = 32
        agent = _agent(spec, has_state=with_state)
        hook = ObservationNormalization()
        hook.agent = agent
        hook.init()
        p = f"on_{case}_"
        for t in range(int(g[p + "steps"])):
            tr = {"observation": torch.from_numpy(g[p + f"obs_in_{t}"])}
            if with_state:
                tr["state"] = torch.from_numpy(g[p + f"state_in_{t}"])
            hook.pre_act(tr)
            tr.update(next_observation=torch.from_numpy(g[p + f"next_in_{t}"]), done=torch.from_numpy(g[p + f"done_{t}"]))
            if with_state:
                tr["next_state"] = torch.from_numpy(g[p + f"next_state_in_{t}"])
            hook.post_step(tr)
            np.testing.assert_allclose(hook.observation_rms.mean.numpy(), g[p + f"mean_{t}"], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(hook.observation_rms.var.numpy(), g[p + f"var_{t}"], rtol=1e-5, atol=1e-6)
            assert float(hook.observation_rms.count) == float(g[p + f"count_{t}"])
            if with_state:
                np.testing.assert_allclose(hook.state_rms.mean.numpy(), g[p + f"state_mean_{t}"], rtol=1e-5, atol=1e-6)
                np.testing.assert_allclose(hook.state_rms.var.numpy(), g[p + f"state_var_{t}"], rtol=1e-5, atol=1e-6)
