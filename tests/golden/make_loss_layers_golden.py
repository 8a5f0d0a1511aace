"""Regenerate ``loss_layers.npz``: the reference's ``NormalNllLoss`` and ``L2RegularizationLoss`` on CPU
(cusrl/nn/layer/loss.py) — losses and autograd gradients on seeded inputs.

    python tests/golden/make_loss_layers_golden.py

``nll_cases`` lists ``shape|mode|full|reduction``; the inputs of a case are ``nll_in/<shape>/<mode>/{mean,dist,target}`` (or
``leaf`` for the shape whose target is the column view ``leaf[..., LEAF_OFFSET:LEAF_OFFSET + K]``), its results
``nll_out/<case>/{loss,d_mean,d_dist,d_target}``.  The reference's results do not depend on whether it is handed the tuple
``(mean, dist)`` or the chunked ``cat([mean, dist], -1)`` (asserted here, bit for bit), so one record serves both input forms.
"""

from __future__ import annotations

import math
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from make_golden import META, REFERENCE, import_reference, np_  # noqa: E402

HERE = Path(__file__).resolve().parent

EPS = 1e-2  # the clamp bound within reach of ordinary values
MODES = ("log_var", "log_std", "var", "std")
LEAF_WIDTH, LEAF_OFFSET = 11, 2
# rows x K, the smallest at which each path of the kernel can go wrong: one element; a scalar-path shape whose chunked `dist` is
# misaligned; two float4 shapes (pitch 2K when chunked); a leading shape of rank 2; the first shape past one self-finalising
# block (17 527 > 16 384 elements: partials + finalize); a target that is a column view of a wider leaf (pitch != width)
SHAPES = {"1x1": (1, 1), "37x7": (37, 7), "5x12": (5, 12), "6x4": (6, 4), "3x5x8": (3, 5, 8), "1031x17": (1031, 17),
          "9x6@leaf": (9, 6)}
FULL_GRID = "37x7"  # every mode x full x reduction
LARGE = {"1031x17": ("log_var", True, "mean")}  # ~70 KB per array: one mode and reduction
ROTATION = ((False, "mean"), (True, "sum"), (True, "mean"), (False, "sum"))
MARGIN = 1e-3  # no variance parameter lies this close to the clamp bound: the clamp's tie rule never decides a case


def bound_of(mode: str) -> float:
    return {"log_var": math.log(EPS), "log_std": math.log(EPS) / 2, "var": EPS, "std": math.sqrt(EPS)}[mode]


def case_table():
    cases = []
    for index, shape in enumerate(SHAPES):
        for m, mode in enumerate(MODES):
            if shape == FULL_GRID:
                cases += [(shape, mode, full, reduction) for full in (False, True) for reduction in ("mean", "sum")]
                cases.append((shape, mode, bool(m % 2), "none"))
            elif shape in LARGE:
                if mode == LARGE[shape][0]:
                    cases.append((shape, *LARGE[shape]))
            else:
                cases.append((shape, mode, *ROTATION[(index + m) % 4]))
    return cases


def case_name(shape, mode, full, reduction) -> str:
    return f"{shape}|{mode}|{int(full)}|{reduction}"


def draw_inputs(gen, shape, mode):
    """mean, the variance parameter of ``mode`` and the target.  The log-variance is log(EPS) + N(1, 1.5): about a quarter of
    the entries below the bound; entries closer to it than 2 MARGIN are pushed away from it."""
    mean = torch.randn(*shape, generator=gen) * 0.8
    target = mean + torch.randn(*shape, generator=gen) * 0.4 + 0.05
    log_var = math.log(EPS) + 1.0 + 1.5 * torch.randn(*shape, generator=gen, dtype=torch.float64)
    dist = {"log_var": log_var, "log_std": log_var / 2, "var": log_var.exp(), "std": (log_var / 2).exp()}[mode]
    gap = dist - bound_of(mode)
    dist = torch.where(gap.abs() < 2 * MARGIN, bound_of(mode) + torch.where(gap < 0, -1.0, 1.0) * (2 * MARGIN + gap.abs()), dist)
    dist = dist.float()
    assert (dist.double() - bound_of(mode)).abs().min() >= MARGIN, (shape, mode)
    return mean, dist, target


def make_normal_nll(cusrl, out):
    gen = torch.Generator().manual_seed(41)
    inputs, below = {}, []
    for shape_name, shape in SHAPES.items():
        for mode in MODES:
            if shape_name in LARGE and mode != LARGE[shape_name][0]:
                continue
            mean, dist, target = draw_inputs(gen, shape, mode)
            prefix = f"nll_in/{shape_name}/{mode}/"
            out[prefix + "mean"], out[prefix + "dist"] = np_(mean), np_(dist)
            if shape_name.endswith("@leaf"):
                leaf = torch.randn(*shape[:-1], LEAF_WIDTH, generator=gen)
                leaf[..., LEAF_OFFSET:LEAF_OFFSET + shape[-1]] = target
                out[prefix + "leaf"] = np_(leaf)
            else:
                out[prefix + "target"] = np_(target)
            inputs[shape_name, mode] = (mean, dist, target)
            if dist.numel() >= 200:
                below.append((dist.double() < bound_of(mode)).double().mean().item())
    assert all(0.15 < fraction < 0.35 for fraction in below), below

    def evaluate(layer, form, mean, dist, target):
        mean, dist, target = (t.clone().requires_grad_() for t in (mean, dist, target))
        if form == "tuple":
            loss = layer((mean, dist), target)
        else:
            joint = torch.cat([mean, dist], dim=-1)
            loss = layer(joint, target)
        loss.backward(torch.ones_like(loss))
        return loss, mean.grad, dist.grad, target.grad

    cases = case_table()
    for shape_name, mode, full, reduction in cases:
        layer = cusrl.nn.NormalNllLoss(mode=mode, full=full, eps=EPS, reduction=reduction)
        results = {form: evaluate(layer, form, *inputs[shape_name, mode]) for form in ("tuple", "chunked")}
        for a, b in zip(results["tuple"], results["chunked"]):
            assert torch.equal(a, b), f"{case_name(shape_name, mode, full, reduction)}: the two input forms differ"
        loss, d_mean, d_dist, d_target = results["tuple"]
        prefix = f"nll_out/{case_name(shape_name, mode, full, reduction)}/"
        out[prefix + "loss"], out[prefix + "d_mean"], out[prefix + "d_dist"] = np_(loss), np_(d_mean), np_(d_dist)
        if shape_name not in LARGE:
            out[prefix + "d_target"] = np_(d_target)
    out["nll_cases"] = np.array([case_name(*case) for case in cases])
    out["nll_eps"] = np.array(EPS)
    out["nll_leaf_offset"] = np.array(LEAF_OFFSET)
    print(f"NormalNllLoss: {len(cases)} cases, fraction below the bound {min(below):.2f}..{max(below):.2f}")


def make_l2(cusrl, out):
    gen = torch.Generator().manual_seed(42)
    value = torch.randn(37, 7, generator=gen) * 1.3 + 0.2
    out["l2_input"] = np_(value)
    for reduction in ("none", "mean", "sum"):
        x = value.clone().requires_grad_()
        loss = cusrl.nn.L2RegularizationLoss(reduction=reduction)(x)
        loss.backward(torch.ones_like(loss))
        out[f"l2_{reduction}_loss"], out[f"l2_{reduction}_d_input"] = np_(loss), np_(x.grad)


def main():
    cusrl = import_reference()
    cusrl.config.set_device("cpu")
    out = dict(META)
    make_normal_nll(cusrl, out)
    make_l2(cusrl, out)
    np.savez_compressed(HERE / "loss_layers.npz", **out)
    leaked = list(REFERENCE.rglob("__pycache__"))
    assert not leaked, f"bytecode leaked into the reference tree: {leaked[:3]}"
    print("loss_layers.npz:", len(out), "arrays,", (HERE / "loss_layers.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
