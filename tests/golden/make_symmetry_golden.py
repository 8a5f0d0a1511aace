"""Regenerate ``symmetry.npz``: the reference's mirror symmetry on CPU (cusrl/hook/auxiliary/symmetry.py,
cusrl/hook/mdp/observation.py:213-217), with fixed mirror definitions.

    python tests/golden/make_symmetry_golden.py
"""

from __future__ import annotations

import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from make_golden import META, REFERENCE, import_reference, np_  # noqa: E402

HERE = Path(__file__).resolve().parent

# (destination_indices, flipped_indices): a permutation with flips for a 16-wide observation, an 8-wide action and a
# 7-wide state, and a non-bijective one (5 -> 9 columns: some inputs read twice, one never)
OBSERVATION = ([1, 0, 3, 2, 4, 5, 7, 6, 9, 8, 10, 12, 11, 13, 15, 14], [4, 5, 10, 13])
ACTION = ([1, 0, 3, 2, 5, 4, 6, 7], [6, 7])
STATE = ([2, 1, 0, 3, 5, 4, 6], [1, 3, 6])
NON_BIJECTIVE = ([4, 0, 0, 2, 3, 3, 3, 1, 4], [1, 5, 8])
DEFS = {"observation": (OBSERVATION, 16), "action": (ACTION, 8), "state": (STATE, 7), "non_bijective": (NON_BIJECTIVE, 5)}


def make_mirror_def(cusrl, out):
    gen = torch.Generator().manual_seed(5)
    for name, ((dest, flipped), width) in DEFS.items():
        mirror = cusrl.hook.auxiliary.symmetry.MirrorDef(dest, flipped)
        x = torch.randn(37, width, generator=gen)
        x[0, 0], x[1, 0] = 0.0, -0.0
        out[f"mirror_{name}_dest"] = np.array(dest)
        out[f"mirror_{name}_flipped"] = np.array(flipped)
        out[f"mirror_{name}_repr"] = np.array(repr(mirror))
        out[f"mirror_{name}_in"] = np_(x)
        out[f"mirror_{name}_out"] = np_(mirror(x))


def make_transition_mirroring(cusrl, out):
    symmetry = cusrl.hook.auxiliary.symmetry
    gen = torch.Generator().manual_seed(6)
    spec = cusrl.EnvironmentSpec(16, 8, state_dim=7, num_instances=4,
                                 mirror_observation=symmetry.MirrorDef(*OBSERVATION), mirror_action=symmetry.MirrorDef(*ACTION),
                                 mirror_state=symmetry.MirrorDef(*STATE))
    agent = SimpleNamespace(environment_spec=spec, has_state=True)
    hook = symmetry.TransitionMirroring()
    hook.agent = agent
    hook.init()
    transition = {"observation": torch.randn(4, 16, generator=gen), "state": torch.randn(4, 7, generator=gen)}
    for key, value in transition.items():
        out[f"tm_in_{key}"] = np_(value)
    hook.pre_act(transition)
    transition["action"] = torch.randn(4, 8, generator=gen)
    out["tm_in_action"] = np_(transition["action"])
    hook.post_act(transition)
    transition["next_observation"] = torch.randn(4, 16, generator=gen)
    transition["next_state"] = torch.randn(4, 7, generator=gen)
    out["tm_in_next_observation"], out["tm_in_next_state"] = np_(transition["next_observation"]), np_(transition["next_state"])
    hook.post_step(transition)
    for key in ("observation", "state", "action", "next_observation", "next_state"):
        out[f"tm_out_{key}"] = np_(transition[key])


def make_obs_norm(cusrl, out):
    """ObservationNormalization with mirrors over several steps (with a state, and the observation alone)."""
    symmetry = cusrl.hook.auxiliary.symmetry
    gen = torch.Generator().manual_seed(7)
    for case, with_state in (("s", True), ("o", False)):
        N, C, S = 32, 16, 7
        spec = cusrl.EnvironmentSpec(C, 8, state_dim=S if with_state else None, num_instances=N,
                                     mirror_observation=symmetry.MirrorDef(*OBSERVATION),
                                     mirror_state=symmetry.MirrorDef(*STATE) if with_state else None)
        agent = SimpleNamespace(environment_spec=spec, observation_dim=C, state_dim=S if with_state else C, has_state=with_state,
                                inference_mode=False, setup_module=lambda m: m, to_tensor=torch.as_tensor)
        hook = cusrl.hook.ObservationNormalization()
        hook.pre_init(agent)
        hook.init()
        steps = 5
        observation = torch.randn(N, C, generator=gen) * 2 + torch.linspace(-3, 3, C)
        state = torch.randn(N, S, generator=gen) * 0.5 - 1 if with_state else None
        p = f"on_{case}_"
        out[p + "steps"] = np.array(steps)
        for t in range(steps):
            tr = {"observation": observation.clone()}
            if with_state:
                tr["state"] = state.clone()
            hook.pre_act(tr)
            out[p + f"obs_in_{t}"] = np_(observation)
            if with_state:
                out[p + f"state_in_{t}"] = np_(state)
            next_observation = torch.randn(N, C, generator=gen) * (2 + t) + torch.linspace(-3, 3, C)
            next_state = torch.randn(N, S, generator=gen) * 0.5 - 1 if with_state else None
            done = torch.rand(N, 1, generator=gen) < 0.3
            tr.update(next_observation=next_observation.clone(), done=done)
            if with_state:
                tr["next_state"] = next_state.clone()
            hook.post_step(tr)
            out[p + f"next_in_{t}"] = np_(next_observation)
            out[p + f"done_{t}"] = np_(done)
            out[p + f"mean_{t}"] = np_(hook.observation_rms.mean)
            out[p + f"var_{t}"] = np_(hook.observation_rms.var)
            out[p + f"count_{t}"] = np.array(float(hook.observation_rms.count))
            if with_state:
                out[p + f"next_state_in_{t}"] = np_(next_state)
                out[p + f"state_mean_{t}"] = np_(hook.state_rms.mean)
                out[p + f"state_var_{t}"] = np_(hook.state_rms.var)
            observation = torch.where(done, torch.randn(N, C, generator=gen) * 0.1, next_observation)
            if with_state:
                state = torch.where(done, torch.randn(N, S, generator=gen), next_state)


AUGMENTED_KEYS = ("observation", "next_observation", "action", "state", "next_state", "action_logp", "advantage", "value", "return")
TRACES = {  # tag: (symmetry hooks, privileged state width)
    "ta": ("loss", None),
    "tb": ("augmentation", None),
    "tc": ("both", 7),
}


def make_update_traces(cusrl, out):
    """Update traces in the format of make_golden.make_update_trace (8 envs x 16 obs x 8 act, hidden (32, 16)) with
    (a) MirrorSymmetryLoss(0.5, symmetrize_action_std=True) after ppo_surrogate_loss, (b) SymmetricDataAugmentation()
    before value_loss, (c) both with a privileged state; plus the first minibatch's batch fields after augmentation."""
    from cusrl.testing.environment import DummyTorchEnvironment  # noqa: PLC0415

    symmetry = cusrl.hook.auxiliary.symmetry
    factory_kwargs = dict(num_steps_per_update=6, sampler_epochs=2, sampler_mini_batches=3)
    for tag, (which, state_dim) in TRACES.items():
        torch.manual_seed(11)
        env = DummyTorchEnvironment(num_instances=8, observation_dim=16, action_dim=8, reward_dim=1, state_dim=state_dim)
        env.spec.mirror_observation = symmetry.MirrorDef(*OBSERVATION)
        env.spec.mirror_action = symmetry.MirrorDef(*ACTION)
        if state_dim is not None:
            env.spec.mirror_state = symmetry.MirrorDef(*STATE)
        factory = cusrl.preset.PpoAgentFactory(actor_hidden_dims=(32, 16), critic_hidden_dims=(32, 16), **factory_kwargs)
        underlying = factory.to_underlying()
        trace = {"objectives": [], "symmetry": [], "indices": [], "grads_unclipped": [], "grads": [], "params_after": [],
                 "lrs": [], "batch0": {}}

        class Capture(cusrl.Hook):
            def __init__(self, where):
                super().__init__()
                self.where = where
                self.name_(f"capture_{where}")

            def pre_optim(self, optimizer):
                flat = torch.cat([p.grad.reshape(-1) for g in optimizer.param_groups for p in g["params"]])
                trace["grads_unclipped" if self.where == "pre" else "grads"].append(np_(flat))
                if self.where == "pre":
                    trace["lrs"].append([group["lr"] for group in optimizer.param_groups])

            def post_optim(self):
                if self.where == "post":
                    flat = torch.cat([p.detach().reshape(-1) for _, p in self.agent.named_parameters()])
                    trace["params_after"].append(np_(flat))

            def objective(self, metadata, batch):
                if self.where == "post":
                    trace["indices"].append(np_(batch["flat_index"].squeeze(-1)))
                    if not trace["batch0"]:
                        trace["batch0"] = {k: np_(batch[k]) for k in AUGMENTED_KEYS if batch.get(k) is not None}

        if which in ("augmentation", "both"):
            underlying.register_hook(symmetry.SymmetricDataAugmentation(), before="value_loss")
        if which in ("loss", "both"):
            underlying.register_hook(symmetry.MirrorSymmetryLoss(0.5, symmetrize_action_std=True), after="ppo_surrogate_loss")
        underlying.register_hook(Capture("pre"), before="gradient_clipping")
        underlying.register_hook(Capture("post"), after="gradient_clipping")
        agent = underlying(env.spec)

        state0 = {n: np_(p) for n, p in agent.named_parameters()}
        orig_objective = agent.hook.objective

        def wrapped(metadata, batch, _o=orig_objective):
            res = _o(metadata, batch)
            trace["objectives"].append(np.array([res["value_loss"].item(), res["surrogate_loss"].item(),
                                                 res["entropy_loss"].item()], dtype=np.float32))
            if "action_mean_symmetry_loss" in res:
                trace["symmetry"].append(np.array([res["action_mean_symmetry_loss"].item(),
                                                   res["action_std_symmetry_loss"].item()], dtype=np.float32))
            return res

        agent.hook.objective = wrapped
        observation, state, _ = env.reset()
        step = 0
        while True:
            action = agent.act(observation, state)
            observation, state, reward, terminated, truncated, _ = env.step(action)
            flat_index = (torch.arange(8) + step * 8).reshape(8, 1)
            ready = agent.step(observation, reward, terminated, truncated, state, flat_index=flat_index)
            step += 1
            if ready:
                break
        # the reference stores doubled `augmented_*` leaves at every step; they are recorded as the batch fields below
        buffer_in = {k: np_(v) for k, v in agent.buffer.storage.items() if not k.startswith("augmented_")}
        torch.manual_seed(99)
        metrics = agent.update()

        p = tag + "_"
        out[p + "factory_keys"] = np.array(list(factory_kwargs.keys()))
        out[p + "factory_vals"] = np.array([float(v) for v in factory_kwargs.values()])
        out[p + "state_dim"] = np.array(-1 if state_dim is None else state_dim)
        for k, v in state0.items():
            out[p + "param0/" + k] = v
        out[p + "param_names"] = np.array(list(state0.keys()))
        for k, v in buffer_in.items():
            out[p + "buffer_in/" + k] = v
        out[p + "buffer_keys"] = np.array(list(buffer_in.keys()))
        for k, v in trace["batch0"].items():
            out[p + "batch0/" + k] = v
        out[p + "batch0_keys"] = np.array(list(trace["batch0"].keys()))
        out[p + "objectives"] = np.stack(trace["objectives"])
        if trace["symmetry"]:
            out[p + "symmetry"] = np.stack(trace["symmetry"])
        out[p + "indices"] = np.stack(trace["indices"])
        out[p + "grads_unclipped"] = np.stack(trace["grads_unclipped"])
        out[p + "grads"] = np.stack(trace["grads"])
        out[p + "params_after"] = np.stack(trace["params_after"])
        out[p + "lrs"] = np.asarray(trace["lrs"], dtype=np.float64)
        out[p + "metric_keys"] = np.array(list(metrics.keys()))
        out[p + "metric_vals"] = np.array(list(metrics.values()), dtype=np.float64)
        print(f"update trace {tag}: {len(trace['objectives'])} train steps, buffer leaves {list(buffer_in)}, "
              f"batch fields {[(k, v.shape) for k, v in trace['batch0'].items()]}")


def main():
    cusrl = import_reference()
    cusrl.config.set_device("cpu")
    out = dict(META)
    make_mirror_def(cusrl, out)
    make_transition_mirroring(cusrl, out)
    make_obs_norm(cusrl, out)
    make_update_traces(cusrl, out)
    np.savez_compressed(HERE / "symmetry.npz", **out)
    leaked = list(REFERENCE.rglob("__pycache__"))
    assert not leaked, f"bytecode leaked into the reference tree: {leaked[:3]}"
    print("symmetry.npz:", len(out), "arrays")


if __name__ == "__main__":
    main()
