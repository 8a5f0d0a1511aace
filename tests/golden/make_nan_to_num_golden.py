"""Regenerate ``nan_to_num.npz``: the reference's ``ObservationNanToNum`` hook on CPU (cusrl/hook/mdp/observation.py:17-56) —
the four fields it touches, before and after ``pre_act`` / ``post_step``.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_nan_to_num_golden.py

``cases`` lists ``<parameter set>|<state or nostate>``; ``params/<parameter set>`` holds ``(nan, posinf, neginf)`` as float64.
Every tensor is stored as its ``uint32`` bit pattern (NaN payloads and the sign of zero survive): the inputs of a case under
``in/<case>/<field>``, what the hook left there under ``out/<case>/<field>``.  ``special_bits`` are the ten special patterns every
input field contains: at its first element, at its last, and at scattered interior positions.
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from make_golden import META, import_reference  # noqa: E402

HERE = Path(__file__).resolve().parent

PARAMETER_SETS = {"defaults": (0.0, 0.0, 0.0), "finite": (1.5, 1e6, -1e6), "keep_inf": (0.0, float("inf"), float("-inf"))}
# quiet NaN, a NaN with another payload, a negative NaN, +-Inf, -0.0, the smallest denormal (1e-45), -1e-40 (a denormal),
# +-FLT_MAX
SPECIAL_BITS = np.array([0x7FC00000, 0x7FA00000, 0xFFC00000, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001,
                         np.float32(-1e-40).view(np.uint32), 0x7F7FFFFF, 0xFF7FFFFF], dtype=np.uint32)
FIELDS = {"observation": (8, 16), "state": (8, 5), "next_observation": (8, 16), "next_state": (8, 5)}
PHASES = {"pre_act": ("observation", "state"), "post_step": ("next_observation", "next_state")}


def draw_field(gen, shape, rotation: int) -> np.ndarray:
    """Ordinary N(0, 3) values with the ten specials written over the first element, the last one and eight interior positions
    (a seeded choice); ``rotation`` changes which special lands where."""
    bits = (3.0 * torch.randn(*shape, generator=gen)).numpy().view(np.uint32).reshape(-1).copy()
    interior = 1 + torch.randperm(bits.size - 2, generator=gen)[: len(SPECIAL_BITS) - 2].numpy()
    positions = np.concatenate(([0, bits.size - 1], np.sort(interior)))
    bits[positions] = np.roll(SPECIAL_BITS, rotation)
    return bits.reshape(shape)


def main():
    cusrl = import_reference()
    gen = torch.Generator().manual_seed(1756)
    out = dict(META)
    out["special_bits"] = SPECIAL_BITS
    cases = []
    for set_name, params in PARAMETER_SETS.items():
        out[f"params/{set_name}"] = np.array(params, dtype=np.float64)
        for with_state in (True, False) if set_name == "defaults" else (True,):
            case = f"{set_name}|{'state' if with_state else 'nostate'}"
            cases.append(case)
            hook = cusrl.hook.ObservationNanToNum(*params)
            transition = {}
            for rotation, (field, shape) in enumerate(FIELDS.items()):
                if not with_state and field.endswith("state"):
                    continue
                bits = draw_field(gen, shape, rotation)
                out[f"in/{case}/{field}"] = bits
                transition[field] = torch.from_numpy(bits.copy()).view(torch.float32)
            for phase, fields in PHASES.items():
                untouched = {f: t.clone() for f, t in transition.items() if f not in fields}
                getattr(hook, phase)(transition)
                for field, before in untouched.items():  # a phase leaves the other phase's fields alone
                    assert torch.equal(before.view(torch.int32), transition[field].view(torch.int32)), (case, phase, field)
            for field, tensor in transition.items():
                result = tensor.numpy().view(np.uint32).copy()
                source = out[f"in/{case}/{field}"]
                finite = (source & 0x7F800000) != 0x7F800000
                assert np.array_equal(result[finite], source[finite]), (case, field)  # the reference passes finite bits through
                assert (~finite).sum() == 5
                out[f"out/{case}/{field}"] = result
    out["cases"] = np.array(cases)
    np.savez_compressed(HERE / "nan_to_num.npz", **out)
    print(f"wrote nan_to_num.npz: {len(cases)} cases, {(HERE / 'nan_to_num.npz').stat().st_size} bytes")


if __name__ == "__main__":
    main()
