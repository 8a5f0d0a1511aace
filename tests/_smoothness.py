"""Shared by the action-smoothness tests (CPU and GPU): the cases of golden ``smoothness.npz``
(tests/golden/make_smoothness_golden.py), one way to run a case through the public hook, and the closed form of the loss in
float64 numpy."""

from __future__ import annotations

from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

GOLDEN = np.load(Path(__file__).resolve().parent / "golden" / "smoothness.npz", allow_pickle=False)
INPUTS = [str(name) for name in GOLDEN["inputs"]]
CASES = [str(case) for case in GOLDEN["cases"]]
EMPTY_INPUTS = {str(name) for name in GOLDEN["empty_inputs"]}
KEY_1ST, KEY_2ND = "action_smoothness_1st_order_loss", "action_smoothness_2nd_order_loss"


def parse(case: str):
    name, terms, form = case.split("|")
    return name, terms, form


def case_inputs(case: str, device="cpu"):
    """``(mean, done)`` of a case's input set."""
    name = parse(case)[0]
    return tuple(torch.from_numpy(GOLDEN[f"in/{name}/{leaf}"]).to(device) for leaf in ("mean", "done"))


def case_weights(case: str):
    """``(weight_1st_order, weight_2nd_order)`` as the constructor takes them: a float, a list, or None."""

    def weight(key):
        if key not in GOLDEN.files:
            return None
        value = GOLDEN[key]
        return float(value) if value.ndim == 0 else [float(v) for v in value]

    return weight(f"out/{case}/w1"), weight(f"out/{case}/w2")


def expected(case: str, name: str) -> np.ndarray:
    return GOLDEN[f"out/{case}/{name}"]


def make_hook(cusrl, w1, w2, device="cpu", action_dim=None):
    hook = cusrl.hook.ActionSmoothnessLoss(weight_1st_order=w1, weight_2nd_order=w2)
    hook.agent = SimpleNamespace(device=torch.device(device), action_dim=action_dim,
                                 to_tensor=lambda value: torch.as_tensor(value, device=device))
    hook.init()
    return hook


def run_case(cusrl, case: str, device="cpu", scale: float | None = None):
    """``(losses, d_mean)`` of the public hook on a case: the sum of its terms (times ``scale``) differentiated wrt the mean."""
    mean, done = case_inputs(case, device)
    hook = make_hook(cusrl, *case_weights(case), device=device, action_dim=mean.shape[-1])
    mean.requires_grad_()
    losses = hook.objective({}, {"curr_action_dist": {"mean": mean}, "done": done})
    total = sum(losses.values())
    (total if scale is None else scale * total).backward()
    return losses, mean.grad


def closed_form_f64(mean, done, w1, w2):
    """The issue's closed form in float64: ``{"loss1", "loss2", "n1", "n2", "d_mean"}`` (a loss absent with its weight;
    ``d_mean`` the gradient of the sum of the given terms).  An empty selection gives NaN and adds nothing to the gradient."""
    mean = np.asarray(mean, dtype=np.float64)
    T, B, A = mean.shape
    open_step = ~np.asarray(done).reshape(T, B).astype(bool)
    valid1 = open_step[:-1]                       # pair (t-1, t), indexed by t-1
    valid2 = open_step[:-2] & open_step[1:-1]     # triple (t-2, t-1, t), indexed by t-2
    n1, n2 = int(valid1.sum()), int(valid2.sum())
    result = {"n1": n1, "n2": n2, "d_mean": np.zeros_like(mean)}
    with np.errstate(invalid="ignore", divide="ignore"):
        if w1 is not None:
            w = np.broadcast_to(np.asarray(w1, dtype=np.float32).astype(np.float64), (A,))
            d1 = (mean[1:] - mean[:-1]) * valid1[:, :, None]
            result["loss1"] = np.float64((w * np.abs(d1)).sum()) / (n1 * A) if n1 else np.float64("nan")
            if n1:
                g = w * np.sign(d1) / (n1 * A)
                result["d_mean"][1:] += g
                result["d_mean"][:-1] -= g
        if w2 is not None:
            w = np.broadcast_to(np.asarray(w2, dtype=np.float32).astype(np.float64), (A,))
            d2 = (-mean[:-2] + 2.0 * mean[1:-1] - mean[2:]) * valid2[:, :, None]
            result["loss2"] = np.float64((w * np.abs(d2)).sum()) / (n2 * A) if n2 else np.float64("nan")
            if n2:
                g = w * np.sign(d2) / (n2 * A)
                result["d_mean"][:-2] -= g
                result["d_mean"][1:-1] += 2.0 * g
                result["d_mean"][2:] -= g
    return result


def check_case(case, losses, d_mean, counts, gradient_parity, label, scale=1.0):
    """Losses to 1e-5 relative (an empty selection: NaN, as recorded), the gradient to 1e-5 of its largest entry (an all-zero
    recorded gradient: exactly zeros), counts exact.  Prints what was achieved before it asserts."""
    _, terms, _ = parse(case)
    assert set(losses) == {key for key, term in ((KEY_1ST, "1"), (KEY_2ND, "2")) if term in terms}
    for key, term in ((KEY_1ST, "1"), (KEY_2ND, "2")):
        if term not in terms:
            continue
        value = losses[key]
        reference, value = float(expected(case, f"loss{term}")), float(value.detach() if isinstance(value, torch.Tensor) else value)
        print(f"{label}: loss{term} {value:.9g} vs {reference:.9g}"
              + ("" if np.isnan(reference) else f" (rel {abs(value - reference) / abs(reference):.2e})"))
        if np.isnan(reference):
            assert np.isnan(value), f"{label}: loss{term} of an empty selection is recorded as NaN, got {value}"
        else:
            np.testing.assert_allclose(value, reference, rtol=1e-5)
    if counts is not None:
        assert (int(counts[0]), int(counts[1])) == (int(expected(case, "n1")), int(expected(case, "n2")))
    reference = scale * expected(case, "d_mean")
    candidate = d_mean.detach().cpu().numpy() if isinstance(d_mean, torch.Tensor) else np.asarray(d_mean)
    assert candidate.shape == reference.shape
    if not reference.any():
        assert not candidate.any(), f"{label}: the recorded gradient is all zeros"
        return 0.0
    achieved = gradient_parity(f"smoothness.d_mean[{label}]", candidate, reference, 1e-5)
    print(f"{label}: d_mean {achieved:.2e} of the largest entry")
    return achieved
