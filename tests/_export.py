"""Shared by tests/test_export.py and tests/test_export_gpu.py: the agents of ``export.npz`` rebuilt here from the recorded
parameters, and the replay of the recorded sequence through a ``DeployedPolicy``."""

from __future__ import annotations

import torch

CASES = ("mlp", "gru", "lstm")
# the project's fp32 parity bound, in units of the recorded tensor's largest entry
PARITY = 1e-5


def relative_to_largest(candidate: torch.Tensor, reference: torch.Tensor) -> float:
    reference = reference.to(candidate.device)
    return float((candidate.double() - reference.double()).abs().max() / reference.double().abs().max().clamp_min(1e-30))


def shape(g):
    sequence, rows, K, A = (int(v) for v in g["shape"])
    return sequence, rows, K, A


def build_agent(cusrl, g, case: str, device="cpu"):
    """The agent of ``case`` as the generator built it in the reference, with the recorded actor parameters and statistics."""
    _, _, K, A = shape(g)
    if case == "mlp":
        factory = cusrl.preset.PpoAgentFactory(num_steps_per_update=8, actor_hidden_dims=(16, 8), critic_hidden_dims=(16, 8),
                                               normalize_observation=True, device=device).to_underlying()
    elif case == "gru":
        factory = cusrl.preset.RecurrentPpoAgentFactory(
            num_steps_per_update=8, rnn_type="GRU", actor_num_layers=1, actor_hidden_size=12, critic_num_layers=1,
            critic_hidden_size=12, normalize_observation=True, empty_cuda_cache=False, device=device).to_underlying()
        factory.actor_factory.latent_dim = 8
    else:
        factory = cusrl.preset.RecurrentPpoAgentFactory(
            num_steps_per_update=8, rnn_type="LSTM", actor_num_layers=2, actor_hidden_size=8, critic_num_layers=2,
            critic_hidden_size=8, empty_cuda_cache=False, device=device).to_underlying()
    agent = factory(cusrl.template.environment.EnvironmentSpec(K, A, device=device))
    names = [str(name) for name in g[f"{case}/param_names"]]
    parameters = dict(agent.actor.named_parameters())
    assert sorted(names) == sorted(parameters), (names, sorted(parameters))
    with torch.no_grad():
        for name in names:
            parameters[name].copy_(torch.from_numpy(g[f"{case}/param/{name}"]))
        if bool(g[f"{case}/normalized"]):
            rms = agent.hook["observation_normalization"].observation_rms
            assert rms.clamp == float(g[f"{case}/clamp"]) and rms.epsilon == float(g[f"{case}/epsilon"])
            rms.mean.copy_(torch.from_numpy(g[f"{case}/mean"]))
            rms.std.copy_(torch.from_numpy(g[f"{case}/std"]))
            rms.var.copy_(rms.std.square() - rms.epsilon)
    return agent


def replay(policy, g, case: str, device="cpu", fused_done: bool = False):
    """``(actions [T, B, A], memories behind each step, memories behind each reset)`` of the recorded sequence; ``fused_done``:
    ``policy(observation, done=...)`` instead of a call followed by ``reset(done)`` (then no memory in between is seen)."""
    observation = torch.from_numpy(g[f"{case}/observation"]).to(device)
    done = torch.from_numpy(g[f"{case}/done"]).to(device)
    actions, memories, resets = [], [], []
    policy.memory = None
    for t in range(observation.shape[0]):
        if fused_done:
            actions.append(policy(observation[t].contiguous(), done=done[t]).clone())
        else:
            actions.append(policy(observation[t].contiguous()).clone())
            if policy.is_recurrent:
                memories.append(policy.memory.clone())
            policy.reset(done[t] if t % 2 else done[t].unsqueeze(-1))  # [B] and [B, 1] alike
        if policy.is_recurrent:
            resets.append(policy.memory.clone())
    stack = lambda tensors: torch.stack(tensors) if tensors else None  # noqa: E731
    return torch.stack(actions), stack(memories), stack(resets)
