"""Regenerate ``export.npz`` by running the reference on the CPU.  Data only.

Three agents of the reference's ``ppo`` presets on its dummy environment (8 envs, observation 10, action 3), seeded, each
trained for two updates of 8 steps so that parameters and statistics are non-trivial:

* ``mlp``   an MLP actor (hidden (16, 8), ReLU) with ``ObservationNormalization``;
* ``gru``   a one-layer GRU actor (hidden 12) with an ``output_proj`` (latent 8) and observation normalisation;
* ``lstm``  a two-layer LSTM actor (hidden 8), no normaliser.

Per case: every actor parameter, the normaliser's mean / std / clamp / epsilon, 6 observations for 3 envs (scaled and shifted
so that the normaliser and its clamp matter), a ``done`` pattern (env 0 finishes at step 0, env 1 at two consecutive steps, env 2
never) and, step by step, what ``actor.act(..., deterministic=True)`` returns for the normalised observation — the action, the
memory behind the step (for the LSTM: hidden then cell, side by side) and the memory behind ``actor.reset_memory(memory, done)``.
When the reference's own TorchScript export runs (it needs ``yaml``), the exported stateful module is replayed over the same
sequence and asserted to agree with the step-by-step record; ``exported_checked`` says whether that happened.

    python tests/golden/make_export_golden.py
"""

from __future__ import annotations

import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from make_golden import META, REFERENCE, import_reference, np_  # noqa: E402

HERE = Path(__file__).resolve().parent
ENVS, K, A, STEPS, UPDATES = 8, 10, 3, 8, 2
SEQUENCE, ROWS = 6, 3
CASES = ("mlp", "gru", "lstm")


def done_pattern() -> torch.Tensor:
    done = torch.zeros(SEQUENCE, ROWS, dtype=torch.bool)
    done[0, 0] = True  # a done at step 0
    done[2, 1] = done[3, 1] = True  # two consecutive dones
    done[4, 0] = True  # (env 2 never finishes)
    return done


def make_agent(cusrl, case: str, env):
    if case == "mlp":
        factory = cusrl.preset.PpoAgentFactory(num_steps_per_update=STEPS, actor_hidden_dims=(16, 8), critic_hidden_dims=(16, 8),
                                               normalize_observation=True).to_underlying()
    elif case == "gru":
        factory = cusrl.preset.RecurrentPpoAgentFactory(
            num_steps_per_update=STEPS, rnn_type="GRU", actor_num_layers=1, actor_hidden_size=12, critic_num_layers=1,
            critic_hidden_size=12, normalize_observation=True, empty_cuda_cache=False).to_underlying()
        factory.actor_factory.latent_dim = 8  # -> Rnn(output_dim=8): an output_proj behind the core
    else:
        factory = cusrl.preset.RecurrentPpoAgentFactory(
            num_steps_per_update=STEPS, rnn_type="LSTM", actor_num_layers=2, actor_hidden_size=8, critic_num_layers=2,
            critic_hidden_size=8, empty_cuda_cache=False).to_underlying()
    return factory(env.spec)


def flat_memory(memory) -> torch.Tensor:
    if isinstance(memory, dict):
        return torch.cat([memory["hidden"], memory["cell"]], dim=-1)
    return memory


def replay_exported(agent, observation, done):
    """The reference's own export (TorchScript), replayed: actions per step, or None when it does not run here."""
    try:
        import yaml  # noqa: F401, PLC0415
    except ModuleNotFoundError:
        return None
    with tempfile.TemporaryDirectory() as directory, torch.no_grad():  # (its memory buffers must not require a gradient)
        agent.export(directory, target_format="jit", batch_size=ROWS, verbose=False, optimize=False)
        module = torch.jit.load(str(Path(directory) / "actor.pt"))
    actions = []
    with torch.no_grad():
        if agent.actor.is_recurrent:
            # tracing ran `forward` and a random `reset` on the module's own memory buffers: start from a clean memory
            module.reset(torch.ones(ROWS, dtype=torch.bool))
        for t in range(SEQUENCE):
            result = module(observation[t].unsqueeze(0))
            actions.append((result[0] if isinstance(result, (tuple, list)) else result).reshape(ROWS, A).clone())
            if agent.actor.is_recurrent:
                module.reset(done[t])
    return torch.stack(actions)


def make_case(cusrl, out, index: int, case: str) -> bool:
    from cusrl.testing.environment import DummyTorchEnvironment  # noqa: PLC0415

    torch.manual_seed(5200 + index)
    env = DummyTorchEnvironment(num_instances=ENVS, observation_dim=K, action_dim=A, reward_dim=1)
    agent = make_agent(cusrl, case, env)
    observation, state, _ = env.reset()
    scale, shift = torch.rand(K) * 2.0 + 0.5, torch.randn(K)  # the statistics see channels of different location and scale
    for _ in range(UPDATES):
        while True:
            action = agent.act(observation * scale + shift, state)
            observation, state, reward, terminated, truncated, _ = env.step(action)
            if agent.step(observation * scale + shift, reward, terminated, truncated, state):
                break
        agent.update()
    actor = agent.actor.eval()
    p = case + "/"
    names = [name for name, _ in actor.named_parameters()]
    out[p + "param_names"] = np.array(names)
    for name, parameter in actor.named_parameters():
        out[p + "param/" + name] = np_(parameter)
    hooks = {hook.name: hook for hook in agent.hook}
    rms = hooks["observation_normalization"].observation_rms if "observation_normalization" in hooks else None
    assert (rms is not None) == (case != "lstm")
    out[p + "normalized"] = np.array(rms is not None)
    if rms is not None:
        out[p + "mean"], out[p + "std"] = np_(rms.mean), np_(rms.std)
        out[p + "clamp"], out[p + "epsilon"] = np.array(rms.clamp, dtype=np.float64), np.array(rms.epsilon, dtype=np.float64)
    gen = torch.Generator().manual_seed(6200 + index)
    sequence = (torch.randn(SEQUENCE, ROWS, K, generator=gen) * 1.5) * scale + shift
    sequence[1, 2, 0] = 60.0  # beyond the normaliser's clamp, where there is one
    done = done_pattern()
    actions, memories, memories_reset = [], [], []
    memory = None
    with torch.no_grad():
        for t in range(SEQUENCE):
            x = sequence[t] if rms is None else rms.normalize(sequence[t])
            action, memory = actor.act(x, memory=memory, deterministic=True)
            actions.append(action.clone())
            if actor.is_recurrent:
                memories.append(flat_memory(memory).clone())
                actor.reset_memory(memory, done[t])
                memories_reset.append(flat_memory(memory).clone())
    actions = torch.stack(actions)
    out[p + "observation"], out[p + "done"], out[p + "action"] = np_(sequence), np_(done), np_(actions)
    out[p + "recurrent"] = np.array(bool(actor.is_recurrent))
    if actor.is_recurrent:
        out[p + "memory"], out[p + "memory_reset"] = np_(torch.stack(memories)), np_(torch.stack(memories_reset))
    exported = replay_exported(agent, sequence, done)
    if exported is not None:
        error = float((exported.detach() - actions).abs().max())
        assert error <= 1e-5 * max(1.0, float(actions.abs().max())), f"{case}: the exported module differs by {error:.3e}"
    print(f"{case}: {len(names)} actor parameters, largest action {float(actions.abs().max()):.4f}, "
          f"exported module {'agrees' if exported is not None else 'not run'}")
    return exported is not None


def main():
    cusrl = import_reference()
    cusrl.config.set_device("cpu")
    out = dict(META)
    out["cases"] = np.array(CASES)
    out["shape"] = np.array([SEQUENCE, ROWS, K, A])
    checked = [make_case(cusrl, out, index, case) for index, case in enumerate(CASES)]
    out["exported_checked"] = np.array(checked)
    np.savez_compressed(HERE / "export.npz", **out)
    leaked = list(REFERENCE.rglob("__pycache__"))
    assert not leaked, f"bytecode leaked into the reference tree: {leaked[:3]}"
    print("export.npz:", len(out), "arrays,", (HERE / "export.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
