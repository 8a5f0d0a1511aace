"""Regenerate ``distillation.npz`` by running the reference on the CPU.  Data only:

* for each of ReLU, ELU and Tanh a small expert (K = 11, hidden (32, 16), A = 3): its weights, a normaliser's mean and std,
  observations, and what the reference's ``Normalization`` + ``Mlp`` make of them in float32 and in float64;
* what ``StubModule`` and ``Identity`` (cusrl/nn/module/stub.py) return;
* a three-update trace of the reference's ``DistillationAgentFactory`` (cusrl/preset/distillation.py) on the dummy
  environment, 16 envs x 8 steps per update, whose expert is a TorchScript module scripted from the ELU expert's weights into a
  temporary directory: the initial parameters, every update's buffer as the update finds it, the ``distillation_loss`` of every
  minibatch step and the parameters after every update.  The ``.pt`` archive is not kept; the tests script their own.

    python tests/golden/make_distillation_golden.py
"""

from __future__ import annotations

import sys
import tempfile
from pathlib import Path

import numpy as np
import torch
from torch import nn

sys.path.insert(0, str(Path(__file__).resolve().parent))
from make_golden import META, REFERENCE, import_reference, np_  # noqa: E402

HERE = Path(__file__).resolve().parent
ACTIVATIONS = ("ReLU", "ELU", "Tanh")
K, HIDDEN, A = 11, (32, 16), 3
ROWS = 37
ENVS, STEPS, UPDATES = 16, 8, 3
TRACE_ACTIVATION = "ELU"
STUDENT_HIDDEN = (32, 16)


class Teacher(nn.Module):
    """``net((x - mean) / std)`` as a plain torch module (restated in tests/_distillation.py): what gets scripted."""

    def __init__(self, weights, biases, activation, mean, std):
        super().__init__()
        layers = []
        for i, (weight, bias) in enumerate(zip(weights, biases)):
            linear = nn.Linear(weight.shape[1], weight.shape[0])
            with torch.no_grad():
                linear.weight.copy_(weight)
                linear.bias.copy_(bias)
            layers.append(linear)
            if i + 1 < len(weights):
                layers.append(getattr(nn, activation)())
        self.net = nn.Sequential(*layers)
        self.register_buffer("mean", mean.clone())
        self.register_buffer("std", std.clone())

    def forward(self, observation: torch.Tensor) -> torch.Tensor:
        return self.net((observation - self.mean) / self.std)


def expert_tensors(index: int):
    gen = torch.Generator().manual_seed(4100 + index)
    widths = (K, *HIDDEN, A)
    weights = [torch.randn(o, i, generator=gen) * (1.5 / i**0.5) for i, o in zip(widths[:-1], widths[1:])]
    biases = [torch.randn(o, generator=gen) * 0.3 for o in widths[1:]]
    mean = torch.randn(K, generator=gen)
    std = torch.rand(K, generator=gen) * 1.5 + 0.25
    observation = torch.randn(ROWS, K, generator=gen) * 2.0 + mean
    return weights, biases, mean, std, observation


def make_experts(cusrl, out):
    out["activations"] = np.array(ACTIVATIONS)
    out["expert_shape"] = np.array([K, *HIDDEN, A])
    for index, activation in enumerate(ACTIVATIONS):
        weights, biases, mean, std, observation = expert_tensors(index)
        mlp = cusrl.Mlp(K, HIDDEN, A, activation_fn=activation)
        linears = [layer for layer in mlp.layers if isinstance(layer, nn.Linear)]
        assert len(linears) == len(weights)
        with torch.no_grad():
            for linear, weight, bias in zip(linears, weights, biases):
                linear.weight.copy_(weight)
                linear.bias.copy_(bias)
        norm = cusrl.nn.Normalization(mean, std)
        with torch.no_grad():
            out32 = mlp(norm(observation))
            out64 = mlp.double()(norm.double()(observation.double()))
        p = f"expert/{activation}/"
        for i, (weight, bias) in enumerate(zip(weights, biases)):
            out[f"{p}weight_{i}"] = np_(weight)
            out[f"{p}bias_{i}"] = np_(bias)
        out[p + "mean"], out[p + "std"], out[p + "observation"] = np_(mean), np_(std), np_(observation)
        out[p + "output32"], out[p + "output64"] = np_(out32), np_(out64)
        print(f"{activation}: |float32 - float64| max {float((out32.double() - out64).abs().max()):.3e}, "
              f"largest entry {float(out64.abs().max()):.3f}")


def make_stubs(cusrl, out):
    gen = torch.Generator().manual_seed(77)
    x = torch.randn(2, 5, 7, generator=gen)
    out["stub/input"] = np_(x)
    out["stub/default"] = np_(cusrl.nn.StubModule.Factory()(7, None)(x))
    out["stub/four"] = np_(cusrl.nn.StubModule(7, 4)(x))
    out["stub/identity"] = np_(cusrl.nn.Identity.Factory()(7, None)(x))


def make_trace(cusrl, out):
    from cusrl.testing.environment import DummyTorchEnvironment  # noqa: PLC0415

    weights, biases, mean, std, _ = expert_tensors(ACTIVATIONS.index(TRACE_ACTIVATION))
    with tempfile.TemporaryDirectory() as directory:
        path = str(Path(directory) / "expert.pt")
        torch.jit.script(Teacher(weights, biases, TRACE_ACTIVATION, mean, std)).save(path)
        torch.manual_seed(31)
        env = DummyTorchEnvironment(num_instances=ENVS, observation_dim=K, action_dim=A, reward_dim=1)
        factory = cusrl.preset.DistillationAgentFactory(num_steps_per_update=STEPS, actor_hidden_dims=STUDENT_HIDDEN, expert_path=path)
        agent = factory(env.spec)
    out["trace_shape"] = np.array([ENVS, STEPS, UPDATES])
    out["trace_student_hidden"] = np.array(STUDENT_HIDDEN)
    out["trace_activation"] = np.array(TRACE_ACTIVATION)
    out["trace_hooks"] = np.array([hook.name for hook in agent.hook])
    losses = []
    outer = agent.hook.objective

    def wrapped(metadata, batch):
        result = outer(metadata, batch)
        assert list(result) == ["distillation_loss"]
        losses.append(np.float32(result["distillation_loss"].item()))
        return result

    agent.hook.objective = wrapped
    state0 = {name: np_(param) for name, param in agent.named_parameters()}
    out["param_names"] = np.array(list(state0))
    for name, value in state0.items():
        out["param0/" + name] = value
    observation, state, _ = env.reset()
    for update in range(UPDATES):
        while True:
            action = agent.act(observation, state)
            observation, state, reward, terminated, truncated, _ = env.step(action)
            if agent.step(observation, reward, terminated, truncated, state):
                break
        buffer_in = {k: np_(v) for k, v in agent.buffer.storage.items()}
        seen = len(losses)
        torch.manual_seed(99 + update)  # generator state at the update boundary
        metrics = agent.update()
        q = f"{update}_"
        out[q + "buffer_keys"] = np.array(list(buffer_in))
        for k, v in buffer_in.items():
            out[q + "buffer_in/" + k] = v
        out[q + "distillation_loss"] = np.array(losses[seen:], dtype=np.float32)
        out[q + "params_after"] = np_(torch.cat([param.detach().reshape(-1) for _, param in agent.named_parameters()]))
        out[q + "metric_keys"] = np.array(list(metrics.keys()))
        out[q + "metric_vals"] = np.array(list(metrics.values()), dtype=np.float64)
        print(f"update {update}: {len(losses) - seen} train steps, distillation_loss {losses[seen]:.5f} .. {losses[-1]:.5f}, "
              f"leaves {list(buffer_in)}")


def main():
    cusrl = import_reference()
    cusrl.config.set_device("cpu")
    out = dict(META)
    make_experts(cusrl, out)
    make_stubs(cusrl, out)
    make_trace(cusrl, out)
    np.savez_compressed(HERE / "distillation.npz", **out)
    leaked = list(REFERENCE.rglob("__pycache__"))
    assert not leaked, f"bytecode leaked into the reference tree: {leaked[:3]}"
    print("distillation.npz:", len(out), "arrays,", (HERE / "distillation.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
