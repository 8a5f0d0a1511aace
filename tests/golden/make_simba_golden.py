"""Regenerate ``simba.npz``: the reference's ``Simba`` backbone on CPU (cusrl/nn/module/simba.py:11-73) — state dict, input,
output and the gradients of ``sum(output * w)`` for a recorded ``w`` — plus the operands of the LayerNorm-level kernel cases
(inputs only: their expectations are a float64 restatement, tests/_simba.py).

    python tests/golden/make_simba_golden.py

What the file has to hold against the 1 MiB limit on a committed file: the four configurations have 160 000 parameters, so
a state dict and two full gradient sets in fp32 alone would be 1.9 MB.  Nothing is stored lossily; instead
  * one state dict per configuration (both batches use it), its matrices set to multiples of 2^-10 before the reference runs
    and stored as those int8 multiples (``state8/``), its vectors in fp32 (``state/``);
  * inputs and ``w`` drawn as float16-exact values and stored as float16;
  * the gradient of a parameter with more than 4096 entries recorded at every ``stride``-th flat entry (``grad_stride/``, an odd
    stride, so the kept entries walk every row and column); every other gradient in full;
  * the kernel-level operands as ONE pool of float16-exact values plus the index rule of tests/_simba.py ``kernel_case``.

Every module-level case also records the reference's OWN fp32 distance from a float64 evaluation of the same module (the
output relative to its largest entry, each gradient in ``oracle.gradient_error`` units).  The standing bounds are 1e-5; a case
whose recorded distance exceeds half of that would have its seed replaced here — none of the seeds below needed it.
"""

from __future__ import annotations

import copy
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
from make_golden import META, REFERENCE, import_reference, np_  # noqa: E402

HERE = Path(__file__).resolve().parent
# (input_dim, hidden_dim, num_blocks, output_dim, activation)
CONFIGS = [(7, 64, 2, 5, "ReLU"), (48, 100, 1, None, "ReLU"), (12, None, 2, 3, "Tanh"), (9, 260, 0, 4, "ReLU")]
BATCHES = (3, 257)
SEEDS = {(c, b): 1000 + 10 * c + b for c in range(len(CONFIGS)) for b in BATCHES}
BOUND = 1e-5
WEIGHT_STEP = 2.0**-10
FULL_GRADIENT = 4096
POOL = 20011  # (prime)
KERNEL_ROWS = (1, 3, 257, 2049)
KERNEL_WIDTHS = (5, 63, 64, 100, 256, 260, 1024)


def evaluate(module, observation, weight):
    observation = observation.clone().requires_grad_(True)
    output = module(observation)
    params = list(module.parameters())
    grads = torch.autograd.grad((output * weight).sum(), [observation, *params])
    return output.detach(), grads


def gradient_stride(numel: int) -> int:
    stride = -(-numel // FULL_GRADIENT)
    return stride + 1 - stride % 2


def half_exact(shape, gen):
    return torch.randn(shape, generator=gen).half().float()


def make_modules(cusrl, out):
    import oracle

    from cusrl.nn.module.simba import Simba  # noqa: PLC0415

    for c, (input_dim, hidden_dim, num_blocks, output_dim, activation) in enumerate(CONFIGS):
        torch.manual_seed(SEEDS[c, BATCHES[0]])
        gen = torch.Generator().manual_seed(SEEDS[c, BATCHES[0]])
        module = Simba(input_dim, hidden_dim, num_blocks, output_dim, activation)
        with torch.no_grad():
            for name, param in module.named_parameters():
                if param.dim() == 1:  # (LayerNorm starts at weight 1, bias 0: moved off that point so their gradients matter)
                    param.add_(torch.randn(param.shape, generator=gen) * 0.1)
                else:
                    param.copy_((param / WEIGHT_STEP).round().clamp(-127, 127) * WEIGHT_STEP)
        names = [name for name, _ in module.named_parameters()]
        q = f"m{c}_"
        out[q + "state_keys"] = np.array(list(module.state_dict()))
        out[q + "param_names"] = np.array(names)
        for key, value in module.state_dict().items():
            if value.dim() == 1:
                out[q + "state/" + key] = np_(value)
            else:
                out[q + "state8/" + key] = np_((value / WEIGHT_STEP).round()).astype(np.int8)
                assert np.array_equal(out[q + "state8/" + key].astype(np.float32) * np.float32(WEIGHT_STEP), np_(value))
        for batch in BATCHES:
            gen = torch.Generator().manual_seed(SEEDS[c, batch])
            observation = half_exact((batch, input_dim), gen)
            weight = half_exact((batch, module.output_dim), gen)
            output, grads = evaluate(module, observation, weight)
            output64, grads64 = evaluate(copy.deepcopy(module).double(), observation.double(), weight.double())
            p = f"m{c}_{batch}_"
            out[p + "input"], out[p + "w"] = np_(observation).astype(np.float16), np_(weight).astype(np.float16)
            out[p + "output"] = np_(output)
            out[p + "grad_input"] = np_(grads[0])
            for name, grad in zip(names, grads[1:]):
                stride = gradient_stride(grad.numel()) if grad.numel() > FULL_GRADIENT else 1
                out[p + "grad/" + name] = np_(grad).reshape(-1)[::stride].copy() if stride > 1 else np_(grad)
                out[p + "grad_stride/" + name] = np.array(stride)
            distance = [float((output.double() - output64).abs().max() / output64.abs().max())]
            distance += [oracle.gradient_error(np_(g), np_(g64)) for g, g64 in zip(grads, grads64)]
            out[p + "reference_distance"] = np.array(distance)  # output, grad_input, then the parameters in order
            assert max(distance) <= BOUND / 2, f"case {p}: reference distance {max(distance):.2e} > half the bound: replace its seed"
            print(f"simba {CONFIGS[c]} B={batch}: {len(names)} parameters, reference distance from float64 "
                  f"output {distance[0]:.2e}, gradients <= {max(distance[1:]):.2e}")
    out["configs"] = np.array([[i, h or 0, n, o or 0] for i, h, n, o, _ in CONFIGS])
    out["activations"] = np.array([a for *_, a in CONFIGS])
    out["batches"] = np.array(BATCHES)


def make_kernel_cases(out):
    """The pool the LayerNorm-level operands are read from (tests/_simba.py ``kernel_case``: x has mean 1.5 and scale 3, so a
    one-pass variance would show)."""
    out["kernel_pool"] = np_(half_exact((POOL,), torch.Generator().manual_seed(4242))).astype(np.float16)
    out["kernel_rows"], out["kernel_widths"] = np.array(KERNEL_ROWS), np.array(KERNEL_WIDTHS)


def main():
    cusrl = import_reference()
    cusrl.config.set_device("cpu")
    out = dict(META)
    make_modules(cusrl, out)
    make_kernel_cases(out)
    np.savez_compressed(HERE / "simba.npz", **out)
    leaked = list(REFERENCE.rglob("__pycache__"))
    assert not leaked, f"bytecode leaked into the reference tree: {leaked[:3]}"
    print("simba.npz:", len(out), "arrays,", (HERE / "simba.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
