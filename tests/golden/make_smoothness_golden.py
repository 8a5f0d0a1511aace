"""Regenerate ``smoothness.npz``: the reference's ``ActionSmoothnessLoss.objective`` on CPU
(cusrl/hook/auxiliary/smoothness.py:59-102) — both losses, the numbers of valid pairs and triples, and the autograd gradient
with respect to the action mean, on seeded temporal minibatches.

    python tests/golden/make_smoothness_golden.py

``inputs`` lists the input sets ``<shape>[@variant]``; ``in/<input>/{mean,done}`` hold one.  ``cases`` lists
``<input>|<terms>|<form>`` with terms ``1`` / ``2`` / ``12`` (which weights are given) and form ``scalar`` / ``sequence``;
``out/<case>/{w1,w2,loss1,loss2,n1,n2,d_mean}`` hold a case's weights (absent: not given) and results.  ``n1`` / ``n2`` are
counted from the reference's own padded mask (``mask[1:]`` / ``mask[2:]``), not from a formula.  Every input has valid pairs
and triples except those named in ``empty_inputs``.
"""

from __future__ import annotations

import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from make_golden import META, REFERENCE, import_reference, np_  # noqa: E402

HERE = Path(__file__).resolve().parent
DONE_RATE = 0.1
EMPTY = ("T3,B2,A1@all_done_at_0",)  # no triple at all: the second-order term is the mean of an empty selection


def draw_inputs():
    gen = torch.Generator().manual_seed(59)

    def randn(*shape):
        return torch.randn(*shape, generator=gen) * 0.7

    def random_done(T, B):
        return torch.rand(T, B, 1, generator=gen) < DONE_RATE

    inputs = {}
    inputs["T3,B1,A1"] = (randn(3, 1, 1), torch.zeros(3, 1, 1, dtype=torch.bool))
    # column 0 has one pair and no triple, column 1 is unbroken
    done = torch.zeros(3, 2, 1, dtype=torch.bool)
    done[0, 0] = True
    inputs["T3,B2,A1@done_at_0_0"] = (randn(3, 2, 1), done)
    done = torch.zeros(3, 2, 1, dtype=torch.bool)
    done[0] = True
    inputs["T3,B2,A1@all_done_at_0"] = (randn(3, 2, 1), done)
    # one column never done, one done at t = 0 and t = 1 (back to back), one done only at T - 1
    done = torch.zeros(5, 3, 1, dtype=torch.bool)
    done[0, 1] = done[1, 1] = done[4, 2] = True
    inputs["T5,B3,A2"] = (randn(5, 3, 2), done)
    inputs["T8,B300,A7"] = (randn(8, 300, 7), random_done(8, 300))    # 2100 columns: nine blocks, the last one ragged
    inputs["T24,B37,A12"] = (randn(24, 37, 12), random_done(24, 37))  # per-column weight lists of length 12
    # action column 1 is constant in time: both of its differences are exactly 0 (sign(0) = 0)
    mean, done = randn(6, 4, 3), random_done(6, 4)
    mean[:, :, 1] = mean[0, :, 1]
    inputs["T6,B4,A3@constant_column"] = (mean, done)
    return inputs, gen


def weights_for(gen, action_dim: int, form: str):
    if form == "scalar":
        return 0.03, 0.011
    w1 = (0.01 + 0.05 * torch.rand(action_dim, generator=gen)).tolist()
    w2 = (0.005 + 0.02 * torch.rand(action_dim, generator=gen)).tolist()
    return w1, w2


def main():
    cusrl = import_reference()
    cusrl.config.set_device("cpu")
    from cusrl.nn.utils.recurrent import split_and_pad_sequences  # noqa: PLC0415

    agent = SimpleNamespace(device=torch.device("cpu"), to_tensor=torch.as_tensor)
    inputs, gen = draw_inputs()
    out = dict(META)
    cases = []
    for name, (mean, done) in inputs.items():
        out[f"in/{name}/mean"], out[f"in/{name}/done"] = np_(mean), np_(done)
        _, mask = split_and_pad_sequences(mean, done)
        n1, n2 = int(mask[1:].sum()), int(mask[2:].sum())
        if name in EMPTY:
            assert n2 == 0 and n1 > 0, (name, n1, n2)
        else:
            assert n1 > 0 and n2 > 0, (name, n1, n2)
        action_dim = mean.shape[-1]
        for form in ("scalar", "sequence"):
            w1, w2 = weights_for(gen, action_dim, form)
            for terms in ("1", "2", "12"):
                hook = cusrl.hook.ActionSmoothnessLoss(weight_1st_order=w1 if "1" in terms else None,
                                                       weight_2nd_order=w2 if "2" in terms else None)
                hook.agent = agent
                hook.init()
                leaf = mean.clone().requires_grad_()
                losses = hook.objective({}, {"curr_action_dist": {"mean": leaf}, "done": done})
                assert set(losses) == {f"action_smoothness_{'1st' if k == '1' else '2nd'}_order_loss" for k in terms}
                # (an empty selection's NaN does not stop autograd: its gradient is recorded as it comes)
                sum(losses.values()).backward()
                case = f"{name}|{terms}|{form}"
                prefix = f"out/{case}/"
                if "1" in terms:
                    out[prefix + "w1"] = np.asarray(w1, dtype=np.float32)
                    out[prefix + "loss1"] = np_(losses["action_smoothness_1st_order_loss"])
                if "2" in terms:
                    out[prefix + "w2"] = np.asarray(w2, dtype=np.float32)
                    out[prefix + "loss2"] = np_(losses["action_smoothness_2nd_order_loss"])
                out[prefix + "n1"], out[prefix + "n2"] = np.array(n1, dtype=np.int64), np.array(n2, dtype=np.int64)
                out[prefix + "d_mean"] = np_(leaf.grad)
                cases.append(case)
    out["inputs"] = np.array(list(inputs))
    out["cases"] = np.array(cases)
    out["empty_inputs"] = np.array(list(EMPTY))
    np.savez_compressed(HERE / "smoothness.npz", **out)
    leaked = list(REFERENCE.rglob("__pycache__"))
    assert not leaked, f"bytecode leaked into the reference tree: {leaked[:3]}"
    print("smoothness.npz:", len(cases), "cases,", (HERE / "smoothness.npz").stat().st_size, "bytes")
    for name in EMPTY:
        for case in cases:
            if case.startswith(name + "|") and "2" in case.split("|")[1]:
                print(case, "loss2", out[f"out/{case}/loss2"], "d_mean", out[f"out/{case}/d_mean"].reshape(-1))


if __name__ == "__main__":
    main()
