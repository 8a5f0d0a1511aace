"""Regenerate ``symmetric_actor.npz``: the reference's ``SymmetricActor`` / ``SymmetricArchitecture`` on CPU
(cusrl/hook/auxiliary/symmetry.py:359-508), with the mirror definitions of ``make_symmetry_golden.py``.

    python tests/golden/make_symmetric_actor_golden.py
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from make_golden import META, REFERENCE, import_reference, np_  # noqa: E402
from make_symmetry_golden import ACTION, OBSERVATION  # noqa: E402

HERE = Path(__file__).resolve().parent
DISTRIBUTIONS = {"normal": "NormalDist", "adaptive": "AdaptiveNormalDist"}
B = 5


def seeded_weights(actor, gen):
    """Fixed weights with every output alive: a std that depends on the state (adaptive) and stays inside its bijector's range."""
    with torch.no_grad():
        for name, param in actor.named_parameters():
            if name.endswith("std.param"):  # NormalDist: the std itself (identity bijector)
                param.copy_(0.5 + torch.rand(param.shape, generator=gen))
            elif "std_head" in name:  # AdaptiveNormalDist: log std, clamped to [log 0.01, 0]
                param.copy_(torch.randn(param.shape, generator=gen) * 0.1 - (1.0 if name.endswith("bias") else 0.0))
            else:
                param.copy_(torch.randn(param.shape, generator=gen) * 0.3)


def make_actor(cusrl, out):
    symmetry = cusrl.hook.auxiliary.symmetry
    gen = torch.Generator().manual_seed(17)
    for tag, dist_name in DISTRIBUTIONS.items():
        factory = symmetry.SymmetricActorFactory(
            cusrl.Mlp.Factory(hidden_dims=(32, 16), activation_fn="ReLU", ends_with_activation=True),
            getattr(cusrl, dist_name).Factory(),
            mirror_observation=symmetry.MirrorDef(*OBSERVATION), mirror_action=symmetry.MirrorDef(*ACTION))
        actor = factory(16, 8)
        seeded_weights(actor, gen)
        names = [name for name, _ in actor.named_parameters()]
        observation = torch.randn(B, 16, generator=gen)
        recorded_action = torch.randn(B, 8, generator=gen)
        c1, c2 = torch.randn(B, 8, generator=gen), torch.randn(B, 8, generator=gen)
        p = tag + "_"
        out[p + "param_names"] = np.array(names)
        for name, param in actor.named_parameters():
            out[p + "param/" + name] = np_(param)
        out[p + "observation"], out[p + "action"], out[p + "c1"], out[p + "c2"] = map(np_, (observation, recorded_action, c1, c2))

        action_dist, _ = actor(observation)
        out[p + "mean"], out[p + "std"] = np_(action_dist["mean"]), np_(action_dist["std"])
        out[p + "compute_logp"] = np_(actor.compute_logp(action_dist, recorded_action))
        loss = (action_dist["mean"] * c1).sum() + (action_dist["std"] * c2).sum()
        grads = torch.autograd.grad(loss, [param for _, param in actor.named_parameters()])
        for name, grad in zip(names, grads):
            out[p + "grad/" + name] = np_(grad)
        with torch.no_grad():
            _, (action, logp), _ = actor.explore(observation, deterministic=True)
        out[p + "deterministic_action"], out[p + "deterministic_logp"] = np_(action), np_(logp)
        print(f"symmetric actor {tag}: parameters {names}, std in [{action_dist['std'].min():.3f}, {action_dist['std'].max():.3f}]")


FACTORY_KWARGS = dict(num_steps_per_update=6, sampler_epochs=2, sampler_mini_batches=3)
ITERATIONS = 2


def make_update_trace(cusrl, out):
    """Two rollouts and two ``agent.update()`` of the `ppo` preset with ``SymmetricArchitecture`` on the dummy environment, in the
    format of make_golden.make_update_trace: the initial parameters, every iteration's buffer as its update finds it, the
    minibatch indices and the parameters after that update."""
    from cusrl.testing.environment import DummyTorchEnvironment  # noqa: PLC0415

    symmetry = cusrl.hook.auxiliary.symmetry
    torch.manual_seed(11)
    env = DummyTorchEnvironment(num_instances=8, observation_dim=16, action_dim=8, reward_dim=1)
    env.spec.mirror_observation = symmetry.MirrorDef(*OBSERVATION)
    env.spec.mirror_action = symmetry.MirrorDef(*ACTION)
    factory = cusrl.preset.PpoAgentFactory(actor_hidden_dims=(32, 16), critic_hidden_dims=(32, 16), **FACTORY_KWARGS)
    underlying = factory.to_underlying()
    trace = {"indices": [], "params_after": []}

    class Capture(cusrl.Hook):
        def post_optim(self):
            trace["params_after"].append(np_(torch.cat([p.detach().reshape(-1) for _, p in self.agent.named_parameters()])))

        def objective(self, metadata, batch):
            trace["indices"].append(np_(batch["flat_index"].squeeze(-1)))

    underlying.register_hook(symmetry.SymmetricArchitecture())
    underlying.register_hook(Capture().name_("capture_post"), after="gradient_clipping")
    agent = underlying(env.spec)
    assert isinstance(agent.actor, symmetry.SymmetricActor)
    p = "trace_"
    state0 = {n: np_(param) for n, param in agent.named_parameters()}
    out[p + "param_names"] = np.array(list(state0))
    for k, v in state0.items():
        out[p + "param0/" + k] = v
    out[p + "factory_keys"] = np.array(list(FACTORY_KWARGS))
    out[p + "factory_vals"] = np.array([float(v) for v in FACTORY_KWARGS.values()])
    out[p + "iterations"] = np.array(ITERATIONS)

    observation, state, _ = env.reset()
    step = 0
    for iteration in range(ITERATIONS):
        while True:
            action = agent.act(observation, state)
            observation, state, reward, terminated, truncated, _ = env.step(action)
            flat_index = (torch.arange(8) + step * 8).reshape(8, 1)
            ready = agent.step(observation, reward, terminated, truncated, state, flat_index=flat_index)
            step += 1
            if ready:
                break
        # (next_value / advantage / return are what the update writes: stale leftovers of the previous one are not inputs)
        buffer_in = {k: np_(v) for k, v in agent.buffer.storage.items() if k not in ("next_value", "advantage", "return")}
        seen = len(trace["params_after"])
        torch.manual_seed(99 + iteration)  # generator state at the update boundary
        metrics = agent.update()
        q = f"{p}{iteration}_"
        out[q + "buffer_keys"] = np.array(list(buffer_in))
        for k, v in buffer_in.items():
            out[q + "buffer_in/" + k] = v
        for k in ("next_value", "advantage", "return"):
            out[q + "buffer_out/" + k] = np_(agent.buffer.storage[k])
        out[q + "indices"] = np.stack(trace["indices"][seen:])
        out[q + "params_after"] = trace["params_after"][-1]
        out[q + "metric_keys"] = np.array(list(metrics.keys()))
        out[q + "metric_vals"] = np.array(list(metrics.values()), dtype=np.float64)
        print(f"update trace, iteration {iteration}: {len(trace['params_after']) - seen} train steps, buffer leaves {list(buffer_in)}")


def main():
    cusrl = import_reference()
    cusrl.config.set_device("cpu")
    out = dict(META)
    out["observation_dest"], out["observation_flipped"] = np.array(OBSERVATION[0]), np.array(OBSERVATION[1])
    out["action_dest"], out["action_flipped"] = np.array(ACTION[0]), np.array(ACTION[1])
    make_actor(cusrl, out)
    make_update_trace(cusrl, out)
    np.savez_compressed(HERE / "symmetric_actor.npz", **out)
    leaked = list(REFERENCE.rglob("__pycache__"))
    assert not leaked, f"bytecode leaked into the reference tree: {leaked[:3]}"
    print("symmetric_actor.npz:", len(out), "arrays")


if __name__ == "__main__":
    main()
