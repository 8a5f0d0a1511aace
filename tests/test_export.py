"""``ActorCritic.export`` and ``nn.DeployedPolicy`` without a GPU (host forms): the three agents of ``export.npz`` — recorded
by running the reference, tests/golden/make_export_golden.py — rebuilt here, exported, loaded and replayed; the file format;
the refusals; the distillation hook's loader."""

from __future__ import annotations

from types import SimpleNamespace

import pytest
import torch
from torch import nn

import _export as shared


@pytest.fixture(scope="module")
def cusrl():
    import cusrl_amd

    return cusrl_amd


@pytest.fixture(scope="module")
def g(golden):
    return golden("export")


@pytest.fixture(scope="module")
def exported(cusrl, g, tmp_path_factory):
    """``{case: (agent, path)}``: every case exported once."""
    directory = tmp_path_factory.mktemp("export")
    result = {}
    for case in shared.CASES:
        agent = shared.build_agent(cusrl, g, case)
        assert hasattr(agent, "export"), "ActorCritic has no export"
        result[case] = (agent, agent.export(directory, name=case))
    return result


def test_the_generator_checked_the_reference_export(g):
    assert list(g["cases"]) == list(shared.CASES) and g["exported_checked"].all()


@pytest.mark.parametrize("case", shared.CASES)
def test_export_writes_a_policy_file_that_reproduces_the_reference(cusrl, g, exported, case):
    agent, path = exported[case]
    assert path.endswith(f"{case}.pt")
    policy = cusrl.nn.DeployedPolicy.load(path)
    sequence, rows, K, A = shared.shape(g)
    assert (policy.observation_dim, policy.action_dim, policy.is_recurrent) == (K, A, case != "mlp")
    assert policy.memory is None
    actions, memories, resets = shared.replay(policy, g, case)
    assert shared.relative_to_largest(actions, torch.from_numpy(g[f"{case}/action"])) <= shared.PARITY
    if case == "mlp":
        assert policy.memory_dim == 0 and policy.memory is None
        return
    recorded, recorded_reset = torch.from_numpy(g[f"{case}/memory"]), torch.from_numpy(g[f"{case}/memory_reset"])
    assert policy.memory_dim == recorded.shape[-1] and tuple(policy.memory.shape) == (rows, policy.memory_dim)
    assert shared.relative_to_largest(memories, recorded) <= shared.PARITY
    assert shared.relative_to_largest(resets, recorded_reset) <= shared.PARITY
    done = torch.from_numpy(g[f"{case}/done"])
    assert done[0].any() and (done[2] & done[3]).any() and not done.any(0).all()  # the pattern the issue asks for
    assert (resets[done] == 0).all() and torch.equal(resets[~done], memories[~done])  # reset rows exactly zero, no other touched
    # done= in the call is a call followed by reset(done)
    fused_actions, _, fused_resets = shared.replay(policy, g, case, fused_done=True)
    assert torch.equal(fused_actions, actions) and torch.equal(fused_resets, resets)
    policy.reset()
    assert (policy.memory == 0).all()


@pytest.mark.parametrize("case", shared.CASES)
def test_the_file_is_plain_data_and_round_trips_bit_for_bit(cusrl, exported, tmp_path, case):
    agent, path = exported[case]
    data = torch.load(path, map_location="cpu", weights_only=True)  # nothing in the file is executed
    spec = data["spec"]
    assert spec["format"] == "cusrl_amd.policy" and spec["version"] == 1
    kinds = [stage["kind"] for stage in spec["stages"]]
    assert kinds == {"mlp": ["normalize", "mlp", "head"], "gru": ["normalize", "rnn", "head"], "lstm": ["rnn", "head"]}[case]
    assert spec["is_recurrent"] == (case != "mlp") and spec["memory_dim"] == {"mlp": 0, "gru": 12, "lstm": 2 * 2 * 8}[case]
    assert all(isinstance(t, torch.Tensor) and t.device.type == "cpu" and t.dtype == torch.float32 for t in data["tensors"].values())
    # the tensors are the agent's, bit for bit
    state = dict(agent.actor.named_parameters())
    head = kinds.index("head")
    assert torch.equal(data["tensors"][f"{head}.weight"], state["distribution.mean_head.weight"])
    if case != "lstm":
        rms = agent.hook["observation_normalization"].observation_rms
        assert torch.equal(data["tensors"]["0.mean"], rms.mean) and torch.equal(data["tensors"]["0.std"], rms.std)
        assert spec["stages"][0]["clamp"] == rms.clamp and spec["stages"][0]["epsilon"] == rms.epsilon
    if case == "gru":
        assert spec["stages"][1]["type"] == "GRU" and spec["stages"][1]["output_proj"] is True
        assert torch.equal(data["tensors"]["1.weight_hh_l0"], state["backbone.rnn.weight_hh_l0"])
        assert torch.equal(data["tensors"]["1.proj_weight"], state["backbone.output_proj.weight"])
    if case == "lstm":
        assert spec["stages"][0]["type"] == "LSTM" and spec["stages"][0]["num_layers"] == 2
    # save -> load -> save keeps every value and every bit
    policy = cusrl.DeployedPolicy.load(path)
    again = tmp_path / "again.pt"
    policy.save(again)
    data2 = torch.load(again, map_location="cpu", weights_only=True)
    assert data2["spec"] == spec and set(data2["tensors"]) == set(data["tensors"])
    assert all(torch.equal(data2["tensors"][name], tensor) for name, tensor in data["tensors"].items())
    assert "stages=" in repr(policy) and policy.to("cpu") is policy


def test_try_load_tells_other_files_apart(cusrl, exported, tmp_path):
    _, path = exported["mlp"]
    expert_file, garbage, wrong = tmp_path / "expert.pt", tmp_path / "garbage.pt", tmp_path / "wrong.pt"
    cusrl.ExpertPolicy([torch.randn(3, 5)], [torch.randn(3)]).save(expert_file)
    garbage.write_bytes(b"not a policy at all")
    assert cusrl.DeployedPolicy.try_load(expert_file) is None and cusrl.DeployedPolicy.try_load(garbage) is None
    assert cusrl.ExpertPolicy.try_load(path) is None  # and the other way round
    with pytest.raises(ValueError, match="not a file in the 'cusrl_amd.policy' format"):
        cusrl.DeployedPolicy.load(expert_file)
    with pytest.raises(FileNotFoundError):
        cusrl.DeployedPolicy.try_load(tmp_path / "missing.pt")
    data = torch.load(path, weights_only=True)
    data["spec"]["version"] = 2
    torch.save(data, wrong)
    with pytest.raises(ValueError, match="unsupported 'cusrl_amd.policy' version 2"):
        cusrl.DeployedPolicy.try_load(wrong)


def test_memory_is_readable_and_assignable(cusrl, g, exported):
    policy = cusrl.DeployedPolicy.load(exported["gru"][1])
    observation = torch.from_numpy(g["gru/observation"])
    first = policy(observation[0])
    kept = policy.memory.clone()
    second = policy(observation[1])
    policy.memory = kept
    assert torch.equal(policy(observation[1]), second)
    policy.memory = None
    assert torch.equal(policy(observation[0]), first)
    with pytest.raises(ValueError, match=r"\[B, 12\]"):
        policy.memory = torch.zeros(3, 5)
    with pytest.raises(TypeError, match="bool"):
        policy.reset(torch.zeros(3))
    with pytest.raises(ValueError, match="observation"):
        policy(torch.zeros(3, 4))


def test_stage_order_and_contents_are_checked(cusrl):
    head = ({"kind": "head"}, {"weight": torch.randn(2, 4), "bias": torch.randn(2)})
    clean = ({"kind": "nan_to_num", "nan": 0.0, "posinf": 1.0, "neginf": -1.0}, {})
    normalize = ({"kind": "normalize", "clamp": 5.0, "epsilon": 1e-8}, {"mean": torch.zeros(4), "std": torch.ones(4)})
    policy = cusrl.DeployedPolicy([clean, normalize, head], 4, 2)
    assert policy.memory_dim == 0
    with pytest.raises(ValueError, match="out of order"):
        cusrl.DeployedPolicy([normalize, clean, head], 4, 2)
    with pytest.raises(ValueError, match="Unknown stage kind 'conv'"):
        cusrl.DeployedPolicy([({"kind": "conv"}, {}), head], 4, 2)
    with pytest.raises(ValueError, match="needs a 'head' stage"):
        cusrl.DeployedPolicy([normalize], 4, 4)
    with pytest.raises(ValueError, match="action_dim = 3"):
        cusrl.DeployedPolicy([head], 4, 3)


# ------------------------------------------------------------------------------------------------ optional action stages
def test_action_affine_and_clip_follow_the_head(cusrl, g, tmp_path):
    agent = shared.build_agent(cusrl, g, "mlp")
    plain = cusrl.DeployedPolicy.load(agent.export(tmp_path, "plain"))
    agent.environment_spec.action_denormalization = (torch.tensor([2.0, 0.5, 1.5]), torch.tensor([0.25, -1.0, 0.0]))
    shaped = cusrl.DeployedPolicy.load(agent.export(tmp_path, "shaped", action_clip=(-0.75, torch.tensor([0.5, 0.6, 0.7]))))
    assert [stage["kind"] for stage in shaped.spec()["stages"]] == ["normalize", "mlp", "head", "action_affine", "action_clip"]
    observation = torch.from_numpy(g["mlp/observation"])[0]
    expected = plain(observation) * torch.tensor([2.0, 0.5, 1.5]) + torch.tensor([0.25, -1.0, 0.0])
    expected = torch.clamp(expected, torch.full((3,), -0.75), torch.tensor([0.5, 0.6, 0.7]))
    assert torch.equal(shaped(observation), expected)
    unshaped = cusrl.DeployedPolicy.load(agent.export(tmp_path, "unshaped", with_environment_normalization=False))
    assert torch.equal(unshaped(observation), plain(observation))


# ------------------------------------------------------------------------------------------------ refusals
def _actor(cusrl, backbone, distribution=None):
    distribution = distribution or cusrl.nn.NormalDist(backbone.output_dim, 3)
    return cusrl.nn.Actor(backbone, distribution)


def test_actors_outside_the_stage_set_are_refused_by_name(cusrl):
    from cusrl_amd.hook.auxiliary.symmetry import MirrorDef, SymmetricActor
    from cusrl_amd.template.export import actor_stages

    Mlp = cusrl.nn.Mlp
    refused = {
        "backbone Simba": _actor(cusrl, cusrl.nn.Simba(7, 16, 1, 8)),
        "recurrent backbone _Recurrent": _actor(cusrl, _Recurrent(7, 8)),
        "Dropout": _actor(cusrl, Mlp(7, (16, 8), dropout=0.1, ends_with_activation=True)),
        "mixed activations": _actor(cusrl, _mixed(Mlp(7, (16, 8), ends_with_activation=True))),
        "ends_with_activation=False": _actor(cusrl, Mlp(7, (16, 8))),
        "must be one of": _actor(cusrl, Mlp(7, (16, 8), activation_fn="GELU", ends_with_activation=True)),
        "OneHotCategoricalDist": _actor(cusrl, Mlp(7, (16, 8), ends_with_activation=True), cusrl.nn.OneHotCategoricalDist(8, 3)),
        "SymmetricActor": SymmetricActor(_actor(cusrl, Mlp(7, (16, 8), ends_with_activation=True)),
                                         MirrorDef(list(range(7)), []), MirrorDef(list(range(3)), [])),
        "backbone Cnn": _actor(cusrl, _named(cusrl, "Cnn")),
        "backbone TransformerEncoderLayer": _actor(cusrl, _named(cusrl, "TransformerEncoderLayer")),
    }
    for cause, actor in refused.items():
        with pytest.raises(ValueError, match=f"ActorCritic.export: .*{cause}"):
            actor_stages(actor)
    stages = actor_stages(_actor(cusrl, cusrl.nn.Sequential([Mlp(7, (16,), ends_with_activation=True), cusrl.nn.Gru(16, 8)])))
    assert [meta["kind"] for meta, _ in stages] == ["mlp", "rnn", "head"]


class _Recurrent(nn.Module):
    """A recurrent backbone of a kind the stage set does not know."""

    def __new__(cls, input_dim, output_dim):
        from cusrl_amd.nn.module import Module

        class _Recurrent(Module):
            def forward(self, input, memory=None, **kwargs):
                return input[..., :self.output_dim], memory

        return _Recurrent(input_dim, output_dim, is_recurrent=True)


def _named(cusrl, name):
    """A feed-forward module whose class carries the name of a backbone the stage set does not express (building the real one
    adds nothing: the export looks at the type)."""
    from cusrl_amd.nn.module import Module

    kind = type(name, (Module,), {"forward": lambda self, input, **kwargs: input[..., :8]})
    assert name in dir(cusrl.nn)
    return kind(7, 8)


def _mixed(mlp):
    mlp.layers[3] = nn.Tanh()
    return mlp


class _Rewriting:
    """Built lazily so that the module imports without the package."""

    @staticmethod
    def hook(cusrl, declared: bool):
        class ObservationScaling(cusrl.template.Hook):
            def pre_act(self, transition):
                transition["observation"] = transition["observation"] * 2

        class Bystander(cusrl.template.Hook):
            def pre_act(self, transition):
                transition["seen"] = True

            def export_stages(self, which="actor"):
                return ()

        return Bystander() if declared else ObservationScaling()


def _agent_with(cusrl, g, *extra, **properties):
    factory = cusrl.preset.PpoAgentFactory(num_steps_per_update=8, actor_hidden_dims=(16, 8), critic_hidden_dims=(16, 8)).to_underlying()
    for hook in extra:
        factory.register_hook(hook, index=1)
    _, _, K, A = shared.shape(g)
    return factory(cusrl.template.environment.EnvironmentSpec(K, A, **properties))


def test_hooks_that_rewrite_observations_must_contribute_a_stage(cusrl, g, tmp_path):
    with pytest.raises(ValueError, match="hook 'observation_scaling' .*overrides 'pre_act'.*no export stage"):
        _agent_with(cusrl, g, _Rewriting.hook(cusrl, False)).export(tmp_path)
    with pytest.raises(ValueError, match="hook 'transition_mirroring' .*TransitionMirroring"):
        from cusrl_amd.hook.auxiliary.symmetry import MirrorDef

        _, _, K, A = shared.shape(g)
        mirrors = dict(mirror_observation=MirrorDef(list(range(K)), [0]), mirror_action=MirrorDef(list(range(A)), [0]))
        _agent_with(cusrl, g, cusrl.hook.TransitionMirroring(), **mirrors).export(tmp_path)
    assert not list(tmp_path.iterdir())  # a refused agent leaves no file
    agent = _agent_with(cusrl, g, _Rewriting.hook(cusrl, True), cusrl.hook.ObservationNanToNum(nan=0.5, posinf=9.0, neginf=-9.0))
    policy = cusrl.DeployedPolicy.load(agent.export(tmp_path, "clean"))
    stages = policy.spec()["stages"]
    assert stages[0] == {"kind": "nan_to_num", "nan": 0.5, "posinf": 9.0, "neginf": -9.0}
    observation = torch.randn(4, agent.observation_dim)
    dirty = observation.clone()
    dirty[0, 0], dirty[1, 1], dirty[2, 2] = float("nan"), float("inf"), float("-inf")
    observation[0, 0], observation[1, 1], observation[2, 2] = 0.5, 9.0, -9.0
    assert torch.equal(policy(dirty), policy(observation))
    # the spec's observation normalisation has no place in front of the hooks' stages
    agent.environment_spec.observation_normalization = (torch.ones(agent.observation_dim), torch.zeros(agent.observation_dim))
    with pytest.raises(ValueError, match="observation_normalization"):
        agent.export(tmp_path, "normalized")


def test_normalization_stage_carries_the_observation_statistics_not_the_states(cusrl):
    factory = cusrl.preset.PpoAgentFactory(num_steps_per_update=8, actor_hidden_dims=(16, 8), critic_hidden_dims=(16, 8),
                                           normalize_observation=True).to_underlying()
    agent = factory(cusrl.template.environment.EnvironmentSpec(5, 2, state_dim=9))
    hook = agent.hook["observation_normalization"]
    hook.observation_rms.mean.fill_(0.25)
    hook.state_rms.mean.fill_(-4.0)
    (meta, tensors), = hook.export_stages("actor")
    assert meta["kind"] == "normalize" and tensors["mean"].shape == (5,) and (tensors["mean"] == 0.25).all()
    assert cusrl.template.Hook().export_stages("actor") == ()


# ------------------------------------------------------------------------------------------------ the distillation hook
def test_policy_distillation_reads_an_exported_file_like_the_expert_of_the_same_actor(cusrl, g, exported, tmp_path):
    agent, path = exported["mlp"]
    rms = agent.hook["observation_normalization"].observation_rms
    expert = cusrl.ExpertPolicy.from_actor(agent.actor, rms)
    expert_file = tmp_path / "expert.pt"
    expert.save(expert_file)
    observation = torch.from_numpy(g["mlp/observation"]).flatten(0, 1)
    done = torch.rand(observation.shape[0], 1) < 0.3
    written = {}
    for name, file in (("exported", path), ("expert", str(expert_file))):
        hook = cusrl.hook.PolicyDistillation(file)
        hook.pre_init(SimpleNamespace(device=torch.device("cpu")))
        hook.init()
        transition = {"observation": observation.clone(), "done": done.clone()}
        hook.post_step(transition)
        written[name] = transition["expert_action"]
        assert isinstance(hook.expert, cusrl.DeployedPolicy if name == "exported" else cusrl.ExpertPolicy)
        assert hook.native_expert == (name == "expert")  # files in the expert format are handled exactly as before
    assert torch.equal(written["exported"], written["expert"])  # bit-identical on the CPU
    assert torch.equal(written["expert"], expert(observation))
