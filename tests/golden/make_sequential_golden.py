"""Regenerate ``sequential.npz``: the reference's ``Sequential`` on CPU (cusrl/nn/module/sequential.py:15-78) around its
``Normalization`` / ``Denormalization`` layers (normalization.py:13-89), plus the operands of the column-affine kernel cases.

    python tests/golden/make_sequential_golden.py

The recorded module is ``Sequential(Normalization(mean6, std6), Mlp(6, [8], ReLU, ends_with_activation=True), Gru(8 -> 8, one
layer), Mlp(8, [], 4), Denormalization(mean4, std4))`` with seeded weights, stored as the reference's state dict.  Four calls
on those weights, each with the output, the final memory dict, the ``intermediate_repr`` keys and the gradient of
``output.sum()`` with respect to the input:

  * ``seq_``     a temporal batch ``[T=5, B=3, 6]`` from an initial memory, with a ``done`` pattern that ends env 1's episode after
                 step 2 (the reference returns no memory from this form: the RNN also consumed padded steps);
  * ``packed_``  the same call with ``pack_sequence=True``, which does return every env's true final state;
  * ``plain_``   the temporal batch without ``done`` (the one temporal form that needs no done-split layout, which this project
                 only has on the device: the CPU test replays this call and the next one);
  * ``step_``    a single step ``[B=3, 6]``, ``sequential=False``, from the same initial memory.

The kernel cases are inputs only (``x`` and ``dy`` read from one recorded pool, ``mean`` and ``std`` in [1e-3, 3] at the largest
width): their expectations are torch's own fp32 expressions, evaluated by the test on the device it runs on.
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from make_golden import META, REFERENCE, import_reference, np_  # noqa: E402

HERE = Path(__file__).resolve().parent
T, B, OBS, HIDDEN, ACT = 5, 3, 6, 8, 4
KERNEL_ROWS = (1, 3, 257, 2049)
KERNEL_WIDTHS = (1, 3, 4, 48, 50, 260)
POOL = 4099  # (prime)


def call(module, observation, memory, **kwargs):
    module.clear_intermediate_repr()
    observation = observation.clone().requires_grad_(True)
    output, final_memory = module(observation, memory={key: value.clone() for key, value in memory.items()}, **kwargs)
    (grad,) = torch.autograd.grad(output.sum(), observation)
    return output.detach(), final_memory, list(module.intermediate_repr), grad


def record(out, prefix, output, final_memory, keys, grad):
    out[prefix + "output"], out[prefix + "grad_input"] = np_(output), np_(grad)
    out[prefix + "memory_keys"] = np.array(sorted(final_memory), dtype=np.str_)
    for key, value in final_memory.items():
        out[prefix + "memory/" + key] = np_(value)
    out[prefix + "repr_keys"] = np.array(keys)


def make_module(cusrl, out):
    from cusrl.nn.module.mlp import Mlp  # noqa: PLC0415
    from cusrl.nn.module.normalization import Denormalization, Normalization  # noqa: PLC0415
    from cusrl.nn.module.rnn import Gru  # noqa: PLC0415
    from cusrl.nn.module.sequential import Sequential  # noqa: PLC0415

    torch.manual_seed(2024)
    gen = torch.Generator().manual_seed(2024)
    mean6, std6 = torch.randn(OBS, generator=gen), torch.rand(OBS, generator=gen) * 2 + 0.5
    mean4, std4 = torch.randn(ACT, generator=gen), torch.rand(ACT, generator=gen) * 2 + 0.5
    module = Sequential(Normalization(mean6, std6), Mlp(OBS, [HIDDEN], activation_fn="ReLU", ends_with_activation=True),
                        Gru(HIDDEN, HIDDEN, num_layers=1), Mlp(HIDDEN, [], ACT), Denormalization(mean4, std4))
    assert module.is_recurrent and (module.input_dim, module.output_dim) == (OBS, ACT)
    out["state_keys"] = np.array(list(module.state_dict()))
    for key, value in module.state_dict().items():
        out["state/" + key] = np_(value)

    observation = torch.randn(T, B, OBS, generator=gen) * 2 + 1
    memory = {"2": torch.randn(B, HIDDEN, generator=gen)}
    done = torch.zeros(T, B, 1, dtype=torch.bool)
    done[2, 1] = True  # env 1's episode ends after step 2: steps 3 and 4 restart from a zero memory
    out["input"], out["initial_memory/2"], out["done"] = np_(observation), np_(memory["2"]), np_(done)
    record(out, "seq_", *call(module, observation, memory, done=done))
    record(out, "packed_", *call(module, observation, memory, done=done, pack_sequence=True))
    record(out, "plain_", *call(module, observation, memory))
    record(out, "step_", *call(module, observation[0], memory, sequential=False))
    for prefix in ("seq_", "packed_", "plain_", "step_"):
        print(prefix, "memory keys", list(out[prefix + "memory_keys"]), "repr keys", list(out[prefix + "repr_keys"]))


def make_kernel_cases(out):
    """One pool of normal draws (tests/_sequential.py ``kernel_case`` reads ``x`` and ``dy`` from it by an index rule: full copies
    of the largest case would be megabytes) and the statistics at the largest width, sliced for the narrower cases."""
    gen = torch.Generator().manual_seed(777)
    width = max(KERNEL_WIDTHS)
    out["kernel_pool"] = np_(torch.randn(POOL, generator=gen))
    out["kernel_mean"] = np_(torch.randn(width, generator=gen))
    out["kernel_std"] = np_(torch.rand(width, generator=gen) * (3 - 1e-3) + 1e-3)
    out["kernel_rows"], out["kernel_widths"] = np.array(KERNEL_ROWS), np.array(KERNEL_WIDTHS)
    for name in ("kernel_pool", "kernel_mean", "kernel_std"):  # finite, in normal range: no denormal decides a case
        assert np.isfinite(out[name]).all() and (np.abs(out[name]) > 1e-30).all(), name
    assert out["kernel_std"].min() >= 1e-3 and out["kernel_std"].max() <= 3


def main():
    cusrl = import_reference()
    cusrl.config.set_device("cpu")
    out = dict(META)
    make_module(cusrl, out)
    make_kernel_cases(out)
    np.savez_compressed(HERE / "sequential.npz", **out)
    leaked = list(REFERENCE.rglob("__pycache__"))
    assert not leaked, f"bytecode leaked into the reference tree: {leaked[:3]}"
    print("sequential.npz:", len(out), "arrays,", (HERE / "sequential.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
