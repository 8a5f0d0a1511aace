"""Float64 restatement of the symmetric actor's head (cusrl_symmetric_head_fwd / _bwd / _sample), written from the formulas:

    mean[b] = (mean_o[b] + M(mean_m[b])) / 2          std[b] = (std_o[b] + |M(std_m[b])|) / 2
    d_o = g / 2      d_m[i] = sum over the outputs j reading i, increasing j, of sign_j * g[j] / 2   (std: * sgn(M(std_m)[j]))

with M(x)[j] = x[dest[j]] * mult[j], plus what the tests of both kinds share: mirror tables and the golden actors.
"""

from __future__ import annotations

import math

import numpy as np
import torch

LOG_SQRT_2PI = math.log(math.sqrt(2 * math.pi))


def multiplier(dest, flipped) -> np.ndarray:
    mult = np.ones(len(dest))
    mult[list(flipped)] = -1.0
    return mult


def combine64(mean2, std2, dest, flipped):
    """(mean, std) [B, A] in float64 from the stacked [2B, A] operands; ``std2`` may be the [A] vector (one row, both halves)."""
    mean2, std2 = np.asarray(mean2, dtype=np.float64), np.asarray(std2, dtype=np.float64)
    dest, mult = np.asarray(dest), multiplier(dest, flipped)
    B = mean2.shape[0] // 2
    std_o, std_m = (std2[None, :], std2[None, :]) if std2.ndim == 1 else (std2[:B], std2[B:])
    mean = (mean2[:B] + mean2[B:][:, dest] * mult) / 2
    std = np.broadcast_to((std_o + np.abs(std_m[:, dest] * mult)) / 2, mean.shape)
    return mean, std


def combine_backward64(g, operand_m, dest, flipped, through_abs: bool):
    """(d_o, d_m, magnitudes, counts) [B, A]: the gradients of both halves for an incoming ``g [B, A]``, the summed magnitudes of
    each d_m entry's terms and the number of terms.  ``through_abs``: the std's form, every term times sgn(M(operand_m)[j])."""
    g = np.asarray(g, dtype=np.float64)
    dest, mult = np.asarray(dest), multiplier(dest, flipped)
    B, A = g.shape
    d_m, magnitudes, counts = np.zeros((B, A)), np.zeros((B, A)), np.zeros(A, dtype=np.int64)
    for j in range(A):  # increasing output column
        term = mult[j] * g[:, j] / 2
        if through_abs:
            term = term * np.sign(np.asarray(operand_m, dtype=np.float64)[:, dest[j]] * mult[j])
        d_m[:, dest[j]] += term
        magnitudes[:, dest[j]] += np.abs(term)
        counts[dest[j]] += 1
    return g / 2, d_m, magnitudes, counts


def sample64(mean, std, eps):
    """(action, logp [B, 1]) in float64 from fp32-valued mean / std / eps: action = mean + std * eps, Normal log-prob over A."""
    mean, std = np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64)
    action = mean + std * np.asarray(eps, dtype=np.float64)
    return action, normal_logp64(mean, std, action)


def normal_logp64(mean, std, action):
    mean, std, action = (np.asarray(t, dtype=np.float64) for t in (mean, std, action))
    return (-((action - mean) ** 2) / (2 * std**2) - np.log(std) - LOG_SQRT_2PI).sum(axis=-1, keepdims=True)


def normal_logp_magnitude64(mean, std, action):
    """The summed magnitudes of the log-prob's terms [B, 1]: what a relative bound on that sum refers to (the terms cancel)."""
    mean, std, action = (np.asarray(t, dtype=np.float64) for t in (mean, std, action))
    terms = np.abs((action - mean) ** 2 / (2 * std**2)) + np.abs(np.log(std)) + LOG_SQRT_2PI
    return terms.sum(axis=-1, keepdims=True)


def mirror_case(rng, A: int, bijective: bool):
    """(dest, flipped) over A columns: a permutation with flips, or a map where some inputs are read twice and one never."""
    dest = rng.permutation(A)
    if not bijective:
        assert A >= 3
        dest[1] = dest[0]  # one input read twice, the one column 1 read is read by nobody
        if A >= 12:
            dest[5], dest[7] = dest[4], dest[4]  # another read three times
    flipped = sorted(rng.choice(A, size=max(1, A // 3), replace=False).tolist())
    return dest.tolist(), flipped


def golden_actor(cusrl, g, tag: str, device="cpu"):
    """The ``SymmetricActor`` of the golden file's case ``tag`` ("normal" / "adaptive") with its recorded weights."""
    from cusrl_amd.hook import MirrorDef, SymmetricActorFactory
    from cusrl_amd.nn.distribution import AdaptiveNormalDist, NormalDist
    from cusrl_amd.nn.module import Mlp

    distribution = {"normal": NormalDist, "adaptive": AdaptiveNormalDist}[tag]
    factory = SymmetricActorFactory(
        Mlp.Factory(hidden_dims=(32, 16), activation_fn="ReLU", ends_with_activation=True), distribution.Factory(),
        mirror_observation=MirrorDef(g["observation_dest"].tolist(), g["observation_flipped"].tolist()),
        mirror_action=MirrorDef(g["action_dest"].tolist(), g["action_flipped"].tolist()))
    actor = factory(16, 8).to(device)
    names = [name for name, _ in actor.named_parameters()]
    assert names == [str(n) for n in g[tag + "_param_names"]]
    with torch.no_grad():
        for name, param in actor.named_parameters():
            param.copy_(torch.from_numpy(g[f"{tag}_param/{name}"]))
    return actor
