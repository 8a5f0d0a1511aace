"""What the Simba tests of both kinds share: the golden modules, the operands of the LayerNorm-level cases and a float64
restatement of residual add + LayerNorm, written from the formulas:

    s = x + r        mean, var = the row's mean and biased variance        xhat = (s - mean) / sqrt(var + eps)
    y = xhat * gamma + beta
    d_s = (g - mean_H(g) - xhat * mean_H(g * xhat)) / sqrt(var + eps) + ds   with g = dy * gamma
    d_gamma = sum_rows dy * xhat        d_beta = sum_rows dy
"""

from __future__ import annotations

import functools

import numpy as np
import torch

WEIGHT_STEP = np.float32(2.0**-10)
ROW_STRIDE, TENSOR_STRIDE = 7919, 2503  # (primes: rows and tensors start at unrelated places of the pool)


# ------------------------------------------------------------------------------------------------ module-level golden cases
def configs(g):
    """[(input_dim, hidden_dim | None, num_blocks, output_dim | None, activation)] of the golden file."""
    return [(int(i), int(h) or None, int(n), int(o) or None, str(a)) for (i, h, n, o), a in zip(g["configs"], g["activations"])]


def golden_state(g, c: int) -> dict[str, torch.Tensor]:
    state = {}
    for key in (str(k) for k in g[f"m{c}_state_keys"]):
        if f"m{c}_state/{key}" in g.files:
            state[key] = torch.from_numpy(g[f"m{c}_state/{key}"])
        else:  # a matrix, recorded as int8 multiples of 2^-10
            state[key] = torch.from_numpy(g[f"m{c}_state8/{key}"].astype(np.float32) * WEIGHT_STEP)
    return state


def golden_module(cusrl, g, c: int, device="cpu"):
    input_dim, hidden_dim, num_blocks, output_dim, activation = configs(g)[c]
    module = cusrl.nn.Simba(input_dim, hidden_dim, num_blocks, output_dim, activation)
    module.load_state_dict(golden_state(g, c), strict=True)
    return module.to(device)


def run_case(module, g, c: int, batch: int, device="cpu"):
    """(output, grad_input, {parameter: gradient}) of ``sum(module(input) * w)`` on the recorded input and ``w``."""
    p = f"m{c}_{batch}_"
    observation = torch.from_numpy(g[p + "input"].astype(np.float32)).to(device).requires_grad_(True)
    weight = torch.from_numpy(g[p + "w"].astype(np.float32)).to(device)
    output = module(observation)
    names = [name for name, _ in module.named_parameters()]
    grads = torch.autograd.grad((output * weight).sum(), [observation, *module.parameters()])
    return output, grads[0], dict(zip(names, grads[1:]))


def recorded_gradient(g, c: int, batch: int, name: str, candidate):
    """(candidate entries, recorded entries): a large matrix is recorded at every ``stride``-th flat entry."""
    p = f"m{c}_{batch}_"
    stride = int(g[p + "grad_stride/" + name])
    candidate = candidate.detach().cpu().numpy()
    return (candidate.reshape(-1)[::stride] if stride > 1 else candidate), g[p + "grad/" + name]


# ------------------------------------------------------------------------------------------------ LayerNorm-level cases
@functools.lru_cache(maxsize=None)
def _pool_rows(pool_bytes: bytes, tensor: int, rows: int, H: int) -> np.ndarray:
    pool = np.frombuffer(pool_bytes, dtype=np.float16).astype(np.float32)
    index = (np.arange(rows)[:, None] * ROW_STRIDE + np.arange(H)[None, :] + tensor * TENSOR_STRIDE) % pool.size
    return pool[index]


def kernel_case(g, B: int, H: int) -> dict[str, np.ndarray]:
    """fp32 operands of one LayerNorm-level case, read from the recorded pool: entry (b, h) of tensor t is
    ``pool[(7919 b + h + 2503 t) % P]``; x = 1.5 + 3 * that (a one-pass variance would show), gamma = 1 + 0.3 *, beta = 0.3 *."""
    pool = g["kernel_pool"].tobytes()
    rows = max(B, *(int(r) for r in g["kernel_rows"]))
    x, r, dy, ds = (_pool_rows(pool, t, rows, H)[:B] for t in range(4))
    gamma, beta = _pool_rows(pool, 4, 1, H)[0], _pool_rows(pool, 5, 1, H)[0]
    three, one_and_half, one, scale = np.float32(3.0), np.float32(1.5), np.float32(1.0), np.float32(0.3)
    return {"x": one_and_half + three * x, "r": r.copy(), "dy": dy.copy(), "ds": ds.copy(), "gamma": one + scale * gamma,
            "beta": scale * beta}


def add_layer_norm64(x, r, gamma, beta, eps: float):
    """(s, y, xhat, rstd) in float64 from fp32-valued operands; ``s`` is formed from the fp32 sum, as the kernel's rows are."""
    s = np.asarray(x, np.float32) + np.asarray(r, np.float32) if r is not None else np.asarray(x, np.float32)
    s = s.astype(np.float64)
    mean = s.mean(axis=-1, keepdims=True)
    var = ((s - mean) ** 2).mean(axis=-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = (s - mean) * rstd
    return s, xhat * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64), xhat, rstd


def add_layer_norm_bwd64(dy, ds, xhat, rstd, gamma):
    """(d_s, d_gamma, d_beta) in float64."""
    dy = np.asarray(dy, np.float64)
    g = dy * np.asarray(gamma, np.float64)
    d_s = (g - g.mean(axis=-1, keepdims=True) - xhat * (g * xhat).mean(axis=-1, keepdims=True)) * rstd
    if ds is not None:
        d_s = d_s + np.asarray(ds, np.float64)
    return d_s, (dy * xhat).sum(axis=0), dy.sum(axis=0)
