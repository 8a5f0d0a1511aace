"""What the gate / GLU / FeedForward tests of both kinds share: the recorded modules (golden ``gates.npz``), the operands of the
kernel cases, the kernel formulas evaluated in any dtype on the CPU (float64: the expectation; float32: a restatement that shows
without a GPU that the bounds are reachable) and the assertions."""

from __future__ import annotations

import numpy as np
import torch

BOUND = 1e-5  # the standing bound, relative to the largest entry
FWD_RTOL, FWD_ATOL = 1e-5, 2e-6  # the standing forward bound (tests/test_recurrent_gates_gpu.py)
ROWS = (1, 3, 257, 2049)  # a single row, one block, a ragged last block, more lanes than one block holds
WIDTHS = (1, 3, 4, 48, 50, 260)  # the scalar path (C % 4 != 0), the vector path, a width beyond one wave's lanes
GATE_KINDS = ("input", "output", "highway", "sigmoid_tanh", "gru_reset", "gru_out")
GLU_KINDS = ("geglu", "swiglu")
# what each gate kind takes besides x and p, and what its backward produces (include/cusrl_hip.h's table)
TAKES_Y = {"input": True, "output": True, "highway": True, "sigmoid_tanh": False, "gru_reset": False, "gru_out": False}
TAKES_Q = {"input": False, "output": False, "highway": False, "sigmoid_tanh": True, "gru_reset": False, "gru_out": True}
GRADIENTS = {"input": ("dx", "dp"), "output": ("dy", "dp"), "highway": ("dx", "dy", "dp"), "sigmoid_tanh": ("dp", "dq"),
             "gru_reset": ("dx", "dp"), "gru_out": ("dx", "dp", "dq")}
ROW_STRIDE = 7919  # (prime: rows start at unrelated places of the pool)
# (primes: the operands start at unrelated places of the pool); pre-activations are scaled to N(0, 2^2)
OFFSETS = {"x": 0, "y": 1201, "p": 2503, "p2": 3001, "q": 3571, "q2": 523, "dout": 1777}
SCALES = {"x": 1.0, "y": 1.0, "p": 2.0, "p2": 2.0, "q": 2.0, "q2": 2.0, "dout": 1.0}
MODULE_GATES = ("passthrough", "residual", "input", "output", "highway", "sigmoid_tanh", "gru")
GATE_TYPES = {"passthrough": None, "residual": "residual", "input": "input", "output": "output", "highway": "highway",
              "sigmoid_tanh": "sigmoid_tanh", "gru": "gru"}
GATE_DIMS = (8, 6)
GLU_WIDTHS = (12, 16)
FEEDFORWARDS = ("geglu", "swiglu", "gelu")
MODULE_CASES = [*(("gate", name, dim) for name in MODULE_GATES for dim in GATE_DIMS),
                *(("glu", name, width) for name in GLU_KINDS for width in GLU_WIDTHS), *(("ff", name, None) for name in FEEDFORWARDS)]


# ------------------------------------------------------------------------------------------------ kernel operands
def cut(g, name: str, rows: int, C: int) -> torch.Tensor:
    """fp32 operand ``name`` of a ``[rows, C]`` case: entry (r, c) is ``scale * pool[(7919 r + c + offset) % P]``."""
    pool = g["kernel_pool"]
    index = (np.arange(rows)[:, None] * ROW_STRIDE + np.arange(C)[None, :] + OFFSETS[name]) % pool.size
    return torch.from_numpy(np.ascontiguousarray(np.float32(SCALES[name]) * pool[index]))


def gate_case(g, kind: str, rows: int, C: int, second: bool | None = None) -> dict:
    """Operands of one gate case (None for what the kind does not take).  ``second``: with the second addends ``p2`` / ``q2``
    (default: for the two GRU kinds, which is how ``GruGate`` calls them)."""
    second = kind.startswith("gru") if second is None else second
    case = {name: cut(g, name, rows, C) for name in ("x", "p", "dout")}
    case["y"] = cut(g, "y", rows, C) if TAKES_Y[kind] else None
    case["q"] = cut(g, "q", rows, C) if TAKES_Q[kind] else None
    case["p2"] = cut(g, "p2", rows, C) if second else None
    case["q2"] = cut(g, "q2", rows, C) if second and TAKES_Q[kind] else None
    return case


def saturated_gate_case(g, kind: str) -> dict:
    """``[4, 4]``: every combination of p and q in +-{20, 100}; x, y, dout from the pool."""
    case = gate_case(g, kind, 4, 4, second=False)
    case["p"] = torch.from_numpy(g["saturated_p"].reshape(4, 4).copy())
    if TAKES_Q[kind]:
        case["q"] = torch.from_numpy(g["saturated_q"].reshape(4, 4).copy())
    return case


def glu_case(g, rows: int, H: int) -> dict:
    """``input`` ``[rows, 2 H]`` scaled to N(0, 2^2) and ``dout`` ``[rows, H]``."""
    return {"input": cut(g, "p", rows, 2 * H), "dout": cut(g, "dout", rows, H)}


def saturated_glu_case(g) -> dict:
    """``[4, 8]``: the gated half holds +-{20, 100}."""
    case = glu_case(g, 4, 4)
    case["input"][:, 4:] = torch.from_numpy(g["saturated_p"].reshape(4, 4).copy())
    return case


# ------------------------------------------------------------------------------------------------ the formulas, in any dtype
def _sigmoid(v):
    return 1 / (1 + torch.exp(-v))


def _sigmoid_terms(P, kernel_order: bool):
    """``(g, 1 - g, g (1 - g))``; ``kernel_order``: the last two as csrc/gate.hip evaluates them, through ``e = exp(-|P|)`` and
    exactly zero where ``g`` has rounded to 0 or 1."""
    g = _sigmoid(P)
    if not kernel_order:
        return g, 1 - g, g * (1 - g)
    e = torch.exp(-P.abs())
    large = 1 / (1 + e)
    small = e * large
    return g, torch.where(P >= 0, small, large), torch.where((g == 0) | (g == 1), torch.zeros_like(g), large * small)


def _tanh_slope(Q, h, kernel_order: bool):
    """``1 - h h``; ``kernel_order``: ``4 u / (1 + u)^2`` with ``u = exp(-2 |Q|)``, exactly zero where ``h`` has rounded to +-1."""
    if not kernel_order:
        return 1 - h * h
    u = torch.exp(-2 * Q.abs())
    w = 1 / (1 + u)
    return torch.where(h.abs() == 1, torch.zeros_like(h), 4 * u * w * w)


def gate_formulas(kind: str, case: dict, dtype, kernel_order: bool = False) -> dict:
    """``out`` and the gradients the kind's backward writes, each step in ``dtype``: the formulas of include/cusrl_hip.h's table as
    they stand (float64: the expectation), or with ``kernel_order`` the kernel's way of evaluating the same quantities (float32:
    the restatement a CPU can check)."""
    t = {name: None if value is None else value.cpu().to(dtype) for name, value in case.items()}
    x, y, d = t["x"], t["y"], t["dout"]
    P = t["p"] if t["p2"] is None else t["p"] + t["p2"]
    g, complement, slope = _sigmoid_terms(P, kernel_order)
    if TAKES_Q[kind]:
        Q = t["q"] if t["q2"] is None else t["q"] + t["q2"]
        h = torch.tanh(Q)
        h_slope = _tanh_slope(Q, h, kernel_order)
    if kind == "input":
        return {"out": g * x + y, "dx": d * g, "dp": d * x * slope}
    if kind == "output":
        return {"out": x + g * y, "dy": d * g, "dp": d * y * slope}
    if kind == "highway":
        return {"out": g * x + (1 - g) * y, "dx": d * g, "dy": d * complement, "dp": d * (x - y) * slope}
    if kind == "sigmoid_tanh":
        return {"out": x + g * h, "dp": d * h * slope, "dq": d * g * h_slope}
    if kind == "gru_reset":
        return {"out": g * x, "dx": d * g, "dp": d * x * slope}
    return {"out": (1 - g) * x + g * h, "dx": d * complement, "dp": d * (h - x) * slope, "dq": d * g * h_slope}


def saturation_masks(kind: str, case: dict) -> dict:
    """Where fp32 has saturated: ``{"dp": sigmoid is exactly 0 or 1, "dq": tanh is exactly +-1}`` by the kernel's fp32 formulas."""
    p = case["p"].detach().cpu().float()
    g = _sigmoid(p if case["p2"] is None else p + case["p2"].detach().cpu().float())
    masks = {"dp": (g == 0) | (g == 1)}
    if TAKES_Q[kind]:
        masks["dq"] = torch.tanh(case["q"].detach().cpu().float()).abs() == 1
    return masks


def glu_formulas(kind: str, case: dict, dtype) -> dict:
    """``out`` and ``dinput`` (both halves), each step in ``dtype`` in the kernel's order of operations."""
    input, d = case["input"].cpu().to(dtype), case["dout"].cpu().to(dtype)
    H = input.shape[-1] // 2
    a, b = input[..., :H], input[..., H:]
    if kind == "geglu":
        cdf = 0.5 * torch.special.erfc(-b * 0.70710678118654752440)
        pdf = torch.exp(-0.5 * b * b) * 0.39894228040143267794
        act, slope = b * cdf, cdf + b * pdf
    else:
        s = _sigmoid(b)
        act, slope = b * s, s + b * s * (1 - s)
    return {"out": a * act, "dinput": torch.cat([d * act, d * a * slope], dim=-1)}


# ------------------------------------------------------------------------------------------------ assertions
def relative_to_largest(candidate, reference) -> float:
    reference = np.asarray(reference, dtype=np.float64)
    candidate = candidate.detach().cpu().numpy().astype(np.float64) if isinstance(candidate, torch.Tensor) else np.asarray(candidate, np.float64)
    assert candidate.shape == reference.shape, (candidate.shape, reference.shape)
    largest = np.abs(reference).max()
    if largest == 0:  # (a gradient the recorded output does not depend on)
        return float(np.abs(candidate).max())
    return float(np.abs(candidate - reference).max() / largest)


def assert_kernel_matches(label: str, got: dict, want: dict) -> dict:
    """The standing bounds: ``out`` within 1e-5 relative + 2e-6, every gradient tensor within 1e-5 of its largest entry.  Prints
    and returns what was measured: ``out`` as the largest |got - want| / (2e-6 + 1e-5 |want|) (at most 1), gradients relative to
    the largest entry."""
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    errors = {}
    for name, reference in want.items():
        reference = reference.detach().numpy().astype(np.float64)
        candidate = got[name].detach().cpu().numpy()
        assert candidate.dtype == np.float32 and candidate.shape == reference.shape, f"{label} {name}"
        assert np.isfinite(candidate).all(), f"{label} {name}: not finite"
        if name == "out":
            errors[name] = float((np.abs(candidate - reference) / (FWD_ATOL + FWD_RTOL * np.abs(reference))).max())
        else:
            errors[name] = relative_to_largest(candidate, reference)
    print(f"{label}: " + ", ".join(f"{name} {error:.3e}" for name, error in errors.items()) + "  (out: fraction of its bound)")
    for name, error in errors.items():
        if name == "out":
            np.testing.assert_allclose(got[name].detach().cpu().numpy(), want[name].numpy(), rtol=FWD_RTOL, atol=FWD_ATOL, err_msg=f"{label} out")
        else:
            assert error <= BOUND, f"{label} {name}: {error:.3e} of the largest entry exceeds {BOUND:.0e}"
    return errors


def assert_saturated(label: str, got: dict, want: dict, masks: dict | None = None):
    """A saturated case: finite, within 1e-5 of max(1, the tensor's largest entry) — absolute, because whole tensors are ~0
    there — and exactly zero where ``masks`` says that fp32 has saturated."""
    assert sorted(got) == sorted(want)
    for name, reference in want.items():
        reference = reference.numpy().astype(np.float64)
        candidate = got[name].detach().cpu().numpy()
        assert np.isfinite(candidate).all(), f"{label} {name}: not finite"
        error, scale = float(np.abs(candidate - reference).max()), max(1.0, float(np.abs(reference).max()))
        print(f"{label} {name}: |got - want| = {error:.3e}, bound {BOUND * scale:.3e}")
        assert error <= BOUND * scale, f"{label} {name}: |got - want| = {error:.3e} exceeds 1e-5 * {scale:.3e}"
        if masks is not None and name in masks:
            mask = masks[name].numpy()
            assert mask.any(), f"{label} {name}: the case saturates nowhere"
            assert not candidate[mask].any(), f"{label} {name}: not exactly zero where fp32 has saturated"


# ------------------------------------------------------------------------------------------------ recorded modules
def module_prefix(family: str, name: str, size) -> str:
    return f"{family}/{name}/" if size is None else f"{family}/{name}/{size}/"


def build_module(cusrl, family: str, name: str, size):
    """The recorded module with this project's classes (weights not loaded yet)."""
    if family == "gate":
        return cusrl.nn.get_gate_cls(GATE_TYPES[name])(size)
    if family == "glu":
        return {"geglu": cusrl.nn.GeGlu, "swiglu": cusrl.nn.SwiGlu}[name]()
    return {"geglu": lambda: cusrl.nn.FeedForward(6, 16, cusrl.nn.GeGlu), "swiglu": lambda: cusrl.nn.FeedForward(8, 16, cusrl.nn.SwiGlu, output_dim=4),
            "gelu": lambda: cusrl.nn.FeedForward(6)}[name]()


def recorded_state(g, prefix: str) -> dict[str, torch.Tensor]:
    return {str(key): torch.from_numpy(g[prefix + "state/" + str(key)].copy()) for key in g[prefix + "state_keys"]}


def module_inputs(g, family: str, name: str, size) -> tuple[dict, torch.Tensor]:
    """(the recorded inputs by name, the weight ``w`` of the recorded objective ``(out * w).sum()``)."""
    tensor = lambda key: torch.from_numpy(g[key].copy())  # noqa: E731
    if family == "gate":
        return {"x": tensor(f"gate_x/{size}"), "y": tensor(f"gate_y/{size}")}, tensor(f"gate_w/{size}")
    if family == "glu":
        return {"input": tensor(f"glu_input/{size}")}, tensor(f"glu_w/{size}")
    return {"input": tensor(f"ff_input/{name}")}, tensor(f"ff_w/{name}")


def run_module(module, inputs: dict, w: torch.Tensor, device="cpu") -> dict:
    """``{"out", "grad_<input>", "grad/<parameter>"}`` of ``(module(*inputs) * w).sum()`` (zeros where nothing depends on a leaf)."""
    leaves = {name: value.to(device).requires_grad_(True) for name, value in inputs.items()}
    output = module(*leaves.values())
    params = dict(module.named_parameters())
    wanted = [*leaves.values(), *params.values()]
    grads = torch.autograd.grad((output * w.to(device)).sum(), wanted, allow_unused=True)
    result = {"out": output.detach()}
    for key, leaf, grad in zip([*("grad_" + n for n in leaves), *("grad/" + n for n in params)], wanted, grads):
        result[key] = torch.zeros_like(leaf) if grad is None else grad
    return result


def assert_module_matches(label: str, got: dict, g, prefix: str) -> dict:
    """Every recorded tensor within 1e-5 of its largest entry (exactly zero where the recorded tensor is)."""
    recorded = {key[len(prefix):]: g[key] for key in g.files if key.startswith(prefix) and not key[len(prefix):].startswith("state")}
    assert sorted(got) == sorted(recorded), (sorted(got), sorted(recorded))
    errors = {key: relative_to_largest(got[key], value) for key, value in recorded.items()}
    print(f"{label}: worst {max(errors.values()):.3e} of the largest entry over {len(errors)} tensors")
    for key, error in errors.items():
        assert error <= BOUND, f"{label} {key}: {error:.3e} of the largest entry exceeds {BOUND:.0e}"
    return errors
