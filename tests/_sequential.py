"""What the Sequential tests of both kinds share: the golden module and its recorded calls (golden ``sequential.npz``), the
operands of the column-affine kernel cases and torch's own fp32 expressions for them."""

from __future__ import annotations

import numpy as np
import torch

ROW_STRIDE, DY_OFFSET = 7919, 2503  # (primes: rows and the two tensors start at unrelated places of the pool)
OBS, HIDDEN, ACT = 6, 8, 4
# recorded call -> the keyword arguments it was made with (``done`` is filled in from the file)
CALLS = {"seq_": {"done": True}, "packed_": {"done": True, "pack_sequence": True}, "plain_": {}, "step_": {"sequential": False}}


def golden_state(g) -> dict[str, torch.Tensor]:
    return {str(key): torch.from_numpy(g["state/" + str(key)].copy()) for key in g["state_keys"]}


def build_module(cusrl):
    """The recorded architecture with this project's classes (weights not loaded yet)."""
    zeros, ones = torch.zeros, torch.ones
    return cusrl.nn.Sequential(
        cusrl.nn.Normalization(zeros(OBS), ones(OBS)), cusrl.nn.Mlp(OBS, [HIDDEN], activation_fn="ReLU", ends_with_activation=True),
        cusrl.nn.Gru(HIDDEN, HIDDEN, num_layers=1), cusrl.nn.Mlp(HIDDEN, [], ACT), cusrl.nn.Denormalization(zeros(ACT), ones(ACT)))


def golden_module(cusrl, g, device="cpu"):
    module = build_module(cusrl)
    module.load_state_dict(golden_state(g), strict=True)
    return module.to(device)


def run_call(module, g, prefix: str, device="cpu"):
    """(output, final memory dict, intermediate_repr keys, gradient of ``output.sum()`` w.r.t. the input) of a recorded call."""
    kwargs = dict(CALLS[prefix])
    if kwargs.pop("done", False):
        kwargs["done"] = torch.from_numpy(g["done"].copy()).to(device)
    observation = torch.from_numpy(g["input"].copy()).to(device)
    if prefix == "step_":
        observation = observation[0].contiguous()
    observation.requires_grad_(True)
    memory = {"2": torch.from_numpy(g["initial_memory/2"].copy()).to(device)}
    module.clear_intermediate_repr()
    output, final_memory = module(observation, memory=memory, **kwargs)
    (grad,) = torch.autograd.grad(output.sum(), observation)
    return output.detach(), final_memory, list(module.intermediate_repr), grad


def recorded_memory(g, prefix: str) -> dict[str, np.ndarray]:
    return {str(key): g[f"{prefix}memory/{key}"] for key in g[prefix + "memory_keys"]}


# ------------------------------------------------------------------------------------------------ column-affine kernel cases
def kernel_case(g, rows: int, C: int) -> dict[str, torch.Tensor]:
    """fp32 operands of one kernel case: entry (r, c) of ``x`` is ``1 + 3 * pool[(7919 r + c) % P]``, of ``dy``
    ``pool[(7919 r + c + 2503) % P]``; ``mean`` / ``std`` are the first ``C`` recorded statistics (``std`` in [1e-3, 3])."""
    pool = g["kernel_pool"]
    index = (np.arange(rows)[:, None] * ROW_STRIDE + np.arange(C)[None, :]) % pool.size
    x = np.float32(1.0) + np.float32(3.0) * pool[index]
    dy = pool[(index + DY_OFFSET) % pool.size]
    return {"x": torch.from_numpy(x), "dy": torch.from_numpy(np.ascontiguousarray(dy)),
            "mean": torch.from_numpy(g["kernel_mean"][:C].copy()), "std": torch.from_numpy(g["kernel_std"][:C].copy())}


def torch_expression(x, mean, std, inverse: bool):
    """The reference's expressions, normalization.py:52 and :89, as torch evaluates them."""
    return x * std + mean if inverse else (x - mean) / std


def torch_forward_backward(x, mean, std, dy, inverse: bool):
    """(out, dx) of torch's own fp32 expression and autograd, on the device the operands live on."""
    x = x.detach().clone().requires_grad_(True)
    out = torch_expression(x, mean, std, inverse)
    (dx,) = torch.autograd.grad(out, x, grad_outputs=dy)
    return out.detach(), dx


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """``torch.equal`` with NaNs in the same places counted as equal."""
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.isclose(a, b, rtol=0.0, atol=0.0, equal_nan=True).all())
