"""Regenerate ``privileged.npz``: the reference's privileged-information hooks on CPU (cusrl/hook/auxiliary/estimation.py,
representation.py, distillation.py) — stand-alone objectives on seeded inputs and three update traces.

    python tests/golden/make_privileged_golden.py
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

ROWS, OBS, ACT, STATE, LATENT, VALUE = 37, 16, 8, 7, 16, 1
# the three index forms of a `Slice`: a strided slice, a list with a repeat out of order, the reversed leaf.  torch refuses
# slice(None, None, -1), so the reference is given the columns that slice means as a list; the port takes the slice itself.
INDEX_FORMS = {"slice": slice(1, 6, 2), "list": [5, 0, 5], "reversed": list(range(STATE - 1, -1, -1))}


class LatentActor:
    """What the representation hooks see of an actor outside an agent: a call leaves a latent behind."""

    def __init__(self):
        self.intermediate_repr = {}

    def __call__(self, observation, **kwargs):
        self.intermediate_repr["backbone.output"] = torch.zeros(observation.shape[0], LATENT)


def stub_agent():
    return SimpleNamespace(observation_dim=OBS, state_dim=STATE, action_dim=ACT, value_dim=VALUE, has_state=True,
                           device=torch.device("cpu"), setup_module=lambda m: m, to_tensor=torch.as_tensor, actor=LatentActor())


def record_objective(out, prefix, hook, module, batch, differentiated, key):
    """One ``objective`` call: the module's parameters, the loss, its gradient wrt every parameter (flat, in order) and
    wrt the tensors in ``differentiated``."""
    for name, value in module.state_dict().items():
        out[f"{prefix}param/{name}"] = np_(value)
    out[f"{prefix}param_names"] = np.array(list(module.state_dict().keys()))
    loss = hook.objective({}, batch)[key]
    loss.backward()
    out[prefix + "loss"] = np_(loss)
    out[prefix + "grad"] = np_(torch.cat([p.grad.reshape(-1) for p in module.parameters()]))
    for name, tensor in differentiated.items():
        out[f"{prefix}d_{name}"] = np_(tensor.grad)


def make_objectives(cusrl, out):
    gen = torch.Generator().manual_seed(21)
    auxiliary = cusrl.hook.auxiliary
    observation = torch.randn(ROWS, OBS, generator=gen)
    state = torch.randn(ROWS, STATE, generator=gen) * 1.5 + 0.25
    next_state = torch.randn(ROWS, STATE, generator=gen) - 0.5
    action = torch.randn(ROWS, ACT, generator=gen)
    expert_action = torch.randn(ROWS, ACT, generator=gen)
    ret, value = torch.randn(ROWS, VALUE, generator=gen) * 3, torch.randn(ROWS, VALUE, generator=gen)
    done = torch.rand(ROWS, 1, generator=gen) < 0.1
    for name, tensor in (("observation", observation), ("state", state), ("next_state", next_state), ("action", action),
                         ("expert_action", expert_action), ("return", ret), ("value", value), ("done", done)):
        out["obj_" + name] = np_(tensor)
    out["obj_index_forms"] = np.array(list(INDEX_FORMS))

    def latent():
        return (torch.randn(ROWS, LATENT, generator=gen) * 0.7).requires_grad_()

    for form, indices in INDEX_FORMS.items():
        torch.manual_seed(31)
        hook = auxiliary.estimation.StateEstimation(cusrl.Mlp.Factory([12]), source_indices=slice(2, 14), target_indices=indices,
                                                    weight=0.7)
        hook.pre_init(stub_agent())
        hook.init()
        batch = {"observation": observation, "state": state, "done": done, "estimator_memory": None}
        record_objective(out, f"obj_estimation_{form}_", hook, hook.estimator, batch, {}, "state_estimation_loss")

        torch.manual_seed(32)
        hook = auxiliary.representation.StatePrediction(indices, weight=0.3)
        hook.pre_init(stub_agent())
        hook.init()
        hook.agent.actor.intermediate_repr["backbone.output"] = z = latent()
        out[f"obj_state_prediction_{form}_latent"] = np_(z)
        record_objective(out, f"obj_state_prediction_{form}_", hook, hook.predictor, {"state": state}, {"latent": z},
                         "state_prediction_loss")

        torch.manual_seed(33)
        hook = auxiliary.representation.NextStatePrediction(indices, weight=0.2)
        hook.pre_init(stub_agent())
        hook.init()
        hook.agent.actor.intermediate_repr["backbone.output"] = z = latent()
        out[f"obj_next_state_prediction_{form}_latent"] = np_(z)
        record_objective(out, f"obj_next_state_prediction_{form}_", hook, hook.predictor, {"next_state": next_state, "action": action},
                         {"latent": z}, "next_state_prediction_loss")

    for which, predicts_value in (("return", False), ("value", True)):
        torch.manual_seed(34)
        hook = auxiliary.representation.ReturnPrediction(weight=0.05, predicts_value_instead_of_return=predicts_value)
        hook.pre_init(stub_agent())
        hook.init()
        hook.agent.actor.intermediate_repr["backbone.output"] = z = latent()
        out[f"obj_return_prediction_{which}_latent"] = np_(z)
        record_objective(out, f"obj_return_prediction_{which}_", hook, hook.predictor, {"return": ret, "value": value}, {"latent": z},
                         "return_prediction_loss")

    hook = auxiliary.distillation.PolicyDistillationLoss(weight=1.5)
    hook.pre_init(stub_agent())
    hook.init()
    mean = torch.randn(ROWS, ACT, generator=gen).requires_grad_()
    out["obj_distillation_mean"] = np_(mean)
    loss = hook.objective({}, {"curr_action_dist": {"mean": mean}, "expert_action": expert_action})["distillation_loss"]
    loss.backward()
    out["obj_distillation_loss"], out["obj_distillation_d_mean"] = np_(loss), np_(mean.grad)


TRACES = ("pa", "pb", "pc")
AUX_KEYS = {"pa": ("state_estimation_loss",), "pb": ("state_prediction_loss", "return_prediction_loss"),
            "pc": ("next_state_prediction_loss", "distillation_loss")}
STATE_INDICES = [5, 0, 5, 2]
NEXT_STATE_INDICES = slice(1, None, 2)


def privileged_hooks(cusrl, hook_module, tag):
    """The composition of trace ``tag``; shared with the tests, which pass their own package as ``cusrl``."""
    auxiliary = hook_module
    if tag == "pa":  # (a) StateEstimation, observation -> state
        class StateEstimation(auxiliary.StateEstimation):
            """The reference stores no ``estimator_memory`` leaf for a feed-forward estimator (the value is None) and then
            looks it up with ``batch["estimator_memory"]``: the lookup is given its None, nothing else changes."""

            def objective(self, metadata, batch):
                batch.setdefault("estimator_memory", None)
                return super().objective(metadata, batch)

        return [StateEstimation(cusrl.Mlp.Factory([12]), weight=0.5).name_("state_estimation")]
    if tag == "pb":  # (b) StatePrediction + ReturnPrediction
        return [auxiliary.StatePrediction(STATE_INDICES, weight=0.1), auxiliary.ReturnPrediction(weight=0.05)]

    class ExpertAction(cusrl.Hook):  # (c) NextStatePrediction + PolicyDistillationLoss on a leaf a small hook pushes
        def post_step(self, transition):
            transition["expert_action"] = torch.tanh(transition["observation"][..., :ACT])

    return [ExpertAction(), auxiliary.NextStatePrediction(NEXT_STATE_INDICES, weight=0.1), auxiliary.PolicyDistillationLoss(weight=0.25)]


def make_update_traces(cusrl, out):
    """Update traces in the format of make_golden.make_update_trace (8 envs x 16 obs x 8 act, state 7, hidden (32, 16)) with
    the privileged hooks behind ``entropy_loss``, plus their loss values per train step."""
    from cusrl.testing.environment import DummyTorchEnvironment  # noqa: PLC0415

    factory_kwargs = dict(num_steps_per_update=6, sampler_epochs=2, sampler_mini_batches=3)
    for tag in TRACES:
        torch.manual_seed(13)
        env = DummyTorchEnvironment(num_instances=8, observation_dim=OBS, action_dim=ACT, reward_dim=1, state_dim=STATE)
        factory = cusrl.preset.PpoAgentFactory(actor_hidden_dims=(32, 16), critic_hidden_dims=(32, 16), **factory_kwargs)
        underlying = factory.to_underlying()
        trace = {"objectives": [], "aux": [], "indices": [], "grads_unclipped": [], "grads": [], "params_after": [], "lrs": []}

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

        after = "entropy_loss"
        for hook in privileged_hooks(cusrl, cusrl.hook.auxiliary, tag):
            underlying.register_hook(hook, after=after)
            after = hook.name
        underlying.register_hook(Capture("pre"), before="gradient_clipping")
        underlying.register_hook(Capture("post"), after="gradient_clipping")
        agent = underlying(env.spec)

        state0 = {n: np_(p) for n, p in agent.named_parameters()}
        orig_objective = agent.hook.objective

        def wrapped(metadata, batch, _o=orig_objective, _tag=tag):
            res = _o(metadata, batch)
            trace["objectives"].append(np.array([res["value_loss"].item(), res["surrogate_loss"].item(),
                                                 res["entropy_loss"].item()], dtype=np.float32))
            trace["aux"].append(np.array([res[key].item() for key in AUX_KEYS[_tag]], dtype=np.float32))
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
        buffer_in = {k: np_(v) for k, v in agent.buffer.storage.items()}
        torch.manual_seed(99)
        metrics = agent.update()

        p = tag + "_"
        out[p + "factory_keys"] = np.array(list(factory_kwargs.keys()))
        out[p + "factory_vals"] = np.array([float(v) for v in factory_kwargs.values()])
        out[p + "state_dim"] = np.array(STATE)
        for k, v in state0.items():
            out[p + "param0/" + k] = v
        out[p + "param_names"] = np.array(list(state0.keys()))
        for k, v in buffer_in.items():
            out[p + "buffer_in/" + k] = v
        out[p + "buffer_keys"] = np.array(list(buffer_in.keys()))
        out[p + "objectives"] = np.stack(trace["objectives"])
        out[p + "aux"] = np.stack(trace["aux"])
        out[p + "aux_keys"] = np.array(list(AUX_KEYS[tag]))
        out[p + "indices"] = np.stack(trace["indices"])
        out[p + "grads_unclipped"] = np.stack(trace["grads_unclipped"])
        out[p + "grads"] = np.stack(trace["grads"])
        out[p + "params_after"] = np.stack(trace["params_after"])
        out[p + "lrs"] = np.asarray(trace["lrs"], dtype=np.float64)
        out[p + "metric_keys"] = np.array(list(metrics.keys()))
        out[p + "metric_vals"] = np.array(list(metrics.values()), dtype=np.float64)
        print(f"update trace {tag}: {len(trace['objectives'])} train steps, buffer leaves {list(buffer_in)}, "
              f"{len(state0)} parameters")


def main():
    cusrl = import_reference()
    cusrl.config.set_device("cpu")
    out = dict(META)
    make_objectives(cusrl, out)
    make_update_traces(cusrl, out)
    np.savez_compressed(HERE / "privileged.npz", **out)
    leaked = list(REFERENCE.rglob("__pycache__"))
    assert not leaked, f"bytecode leaked into the reference tree: {leaked[:3]}"
    print("privileged.npz:", len(out), "arrays,", (HERE / "privileged.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
