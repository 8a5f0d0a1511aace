"""Shared by the loss-layer tests (CPU and GPU): the cases of golden ``loss_layers.npz``
(tests/golden/make_loss_layers_golden.py) and one way to run a case through the public ``NormalNllLoss``."""

from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

GOLDEN = np.load(Path(__file__).resolve().parent / "golden" / "loss_layers.npz", allow_pickle=False)
EPS = float(GOLDEN["nll_eps"])
LEAF_OFFSET = int(GOLDEN["nll_leaf_offset"])
CASES = [str(case) for case in GOLDEN["nll_cases"]]
REDUCED = [case for case in CASES if not case.endswith("|none")]
UNREDUCED = [case for case in CASES if case.endswith("|none")]
FORMS = ("tuple", "chunked")
MODES = ("log_var", "log_std", "var", "std")


def parse(case: str):
    shape, mode, full, reduction = case.split("|")
    return shape, mode, bool(int(full)), reduction


def case_inputs(case: str, device="cpu"):
    """``(mean, dist, target)`` of a case; the target of an ``@leaf`` shape is the column view of its wider leaf."""
    shape, mode, _, _ = parse(case)
    prefix = f"nll_in/{shape}/{mode}/"
    mean, dist = (torch.from_numpy(GOLDEN[prefix + name]).to(device) for name in ("mean", "dist"))
    if shape.endswith("@leaf"):
        leaf = torch.from_numpy(GOLDEN[prefix + "leaf"]).to(device)
        target = leaf[..., LEAF_OFFSET:LEAF_OFFSET + mean.shape[-1]]
        assert not target.is_contiguous()
    else:
        target = torch.from_numpy(GOLDEN[prefix + "target"]).to(device)
    return mean, dist, target


def expected(case: str, name: str) -> np.ndarray:
    return GOLDEN[f"nll_out/{case}/{name}"]


def run_case(cusrl, case: str, form: str, device="cpu", target_grad: bool = False, scale: float | None = None):
    """``(loss, {name: gradient})`` of the public layer on a case's inputs: ``loss.backward`` with ones (times ``scale``)."""
    _, mode, full, reduction = parse(case)
    mean, dist, target = case_inputs(case, device)
    if target_grad:
        target = target.clone().requires_grad_()
    layer = cusrl.nn.NormalNllLoss(mode=mode, full=full, eps=EPS, reduction=reduction)
    if form == "tuple":
        mean, dist = mean.requires_grad_(), dist.requires_grad_()
        loss = layer((mean, dist), target)
    else:
        joint = torch.cat([mean, dist], dim=-1).requires_grad_()
        loss = layer(joint, target)
    (loss if scale is None else scale * loss).backward(torch.ones_like(loss))
    if form == "tuple":
        grads = {"d_mean": mean.grad, "d_dist": dist.grad}
    else:
        K = joint.shape[-1] // 2
        grads = {"d_mean": joint.grad[..., :K], "d_dist": joint.grad[..., K:]}
    if target_grad:
        grads["d_target"] = target.grad
    return loss, grads


def check_loss(loss, reference, gradient_parity, label):
    """A reduced loss: 1e-5 relative.  An unreduced one is a tensor whose elements 0.5 (log_var + ratio) [+ c] are sums of O(1)
    terms that may cancel (an fp32 rounding of a term, 6e-8 of it, is then any fraction of the element): like a gradient it is
    held to 1e-5 of its largest entry."""
    loss, reference = loss.detach().cpu().numpy(), np.asarray(reference)
    assert loss.shape == reference.shape
    if reference.ndim == 0:
        np.testing.assert_allclose(loss, reference, rtol=1e-5)
    else:
        gradient_parity(label, loss, reference, 1e-5)
