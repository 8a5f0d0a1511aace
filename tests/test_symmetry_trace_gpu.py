"""Replays of the reference's updates with the symmetry hooks (golden ``symmetry.npz``, make_symmetry_golden.py):
(a) MirrorSymmetryLoss after ppo_surrogate_loss, (b) SymmetricDataAugmentation before value_loss, (c) both with a privileged
state.  The augmented batch is compared bit for bit, the losses, gradients and parameters of every step against the
reference; the stock terms must stay one fused launch per step and the augmentation one ``cusrl_mirror_rows``."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from test_agent_gpu import build_agent_from_golden, host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAGS = {"ta": ("loss",), "tb": ("augmentation",), "tc": ("loss", "augmentation")}
# "hipgraph_branch": compile=True with the critic forced onto its own stream — the augmented rows are written on the main
# stream and read by the critic on the branch
MODES = ["fused", "hook_by_hook", "hipgraph", "hipgraph_branch", "flat_adam"]


@pytest.fixture(scope="module")
def cusrl():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    import cusrl_amd

    cusrl_amd.config.set_device(DEV)
    return cusrl_amd


class _WithMirrors:
    """The package as ``build_agent_from_golden`` sees it, but its environment spec carries the trace's mirrors (and state)."""

    def __init__(self, module, g, tag):
        from cusrl_amd.hook import MirrorDef

        self._module = module
        state_dim = int(g[tag + "_state_dim"])
        mirrors = {"mirror_observation": MirrorDef(g["mirror_observation_dest"].tolist(), g["mirror_observation_flipped"].tolist()),
                   "mirror_action": MirrorDef(g["mirror_action_dest"].tolist(), g["mirror_action_flipped"].tolist())}
        if state_dim > 0:
            mirrors["mirror_state"] = MirrorDef(g["mirror_state_dest"].tolist(), g["mirror_state_flipped"].tolist())

        def spec(observation_dim, action_dim, **kwargs):
            return module.EnvironmentSpec(observation_dim, action_dim, state_dim=state_dim if state_dim > 0 else None,
                                          **mirrors, **kwargs)

        self.EnvironmentSpec = spec

    def __getattr__(self, name):
        return getattr(self._module, name)


def _count(name):
    from cusrl_amd import _native

    return _native.launch_counts.get(name, 0)


@pytest.mark.parametrize("tag", list(TAGS))
@pytest.mark.parametrize("mode", MODES)
def test_symmetry_update_replays_reference_trace(cusrl, golden, tag, mode, gradient_parity):
    from cusrl_amd.hook import MirrorSymmetryLoss, SymmetricDataAugmentation
    from cusrl_amd.hook.on_policy.fused import FusedPpoObjective

    g = golden("symmetry")
    hooks = []
    if "augmentation" in TAGS[tag]:
        hooks.append((SymmetricDataAugmentation(), {"before": "value_loss"}))
    if "loss" in TAGS[tag]:
        hooks.append((MirrorSymmetryLoss(0.5, symmetrize_action_std=True), {"after": "ppo_surrogate_loss"}))
    batch0: dict[str, torch.Tensor] = {}
    keys = [str(k) for k in g[tag + "_batch0_keys"]]

    class Tap(cusrl.Hook):
        def post_objective(self, metadata, batch):
            if not batch0:
                batch0.update({k: batch[k].detach().clone() for k in keys})

    hooks.append((Tap(), {}))
    compiled = mode.startswith("hipgraph")
    overrides = {"compile": True} if compiled else {"optimizer_kwargs": {"fused": True}} if mode == "flat_adam" else {}
    agent, trace = build_agent_from_golden(_WithMirrors(cusrl, g, tag), g, tag, extra_hooks=hooks, **overrides)
    agent.fuse_objective = mode != "hook_by_hook"
    if mode == "hipgraph_branch":
        agent.concurrent_critic = True
    if mode != "hook_by_hook":
        assert FusedPpoObjective.mode(agent.hook) == ("fused" if tag == "tb" else "split")

    # per objective evaluation (eager step, capture warm-up or capture): launches of the fused objective and of the mirror
    per_step, symmetry_losses = [], []
    inner = agent.hook.objective

    def counted(metadata, batch):
        before = _count("cusrl_ppo_loss_fwd_bwd"), _count("cusrl_mirror_rows")
        result = inner(metadata, batch)
        per_step.append((_count("cusrl_ppo_loss_fwd_bwd") - before[0], _count("cusrl_mirror_rows") - before[1]))
        if "loss" in TAGS[tag] and result["value_loss"] is not None:
            symmetry_losses.append(torch.stack([result["action_mean_symmetry_loss"], result["action_std_symmetry_loss"]]).detach().clone())
        return result

    agent.hook.objective = counted
    torch.manual_seed(99)
    metrics = agent.update()

    assert np.array_equal(host(torch.stack(trace["indices"])), g[tag + "_indices"]), "minibatch permutations differ"
    for k in keys:  # the [B, 2, ...] batch the other hooks see: bit-identical to the reference's
        if k in ("advantage", "return"):  # computed on the device (GAE, normalisation): the buffer_out tolerance of the PPO traces
            np.testing.assert_allclose(host(batch0[k]), g[f"{tag}_batch0/{k}"], rtol=1e-5, atol=2e-6, err_msg=k)
            if batch0[k].dim() == 3:  # ... and repeated exactly
                assert torch.equal(batch0[k][:, 0], batch0[k][:, 1]), k
        else:
            assert np.array_equal(host(batch0[k]), g[f"{tag}_batch0/{k}"]), k
    mirrors_per_step = len(TAGS[tag])  # the augmentation's one launch + the mirrored observations of the symmetry loss
    assert per_step and all(m == mirrors_per_step for _, m in per_step), per_step
    if mode != "hook_by_hook":
        assert all(p == 1 for p, _ in per_step), per_step
    else:
        assert all(p == 0 for p, _ in per_step), per_step

    seen = len(trace["objectives"])
    assert seen == (len(g[tag + "_objectives"]) if not agent._graphed_steps else sum(1 for s in agent._graphed_steps.values()))
    np.testing.assert_allclose(host(torch.stack(trace["objectives"])), g[tag + "_objectives"][:seen], rtol=2e-5, atol=1e-6)
    if "loss" in TAGS[tag]:
        assert len(symmetry_losses) == seen
        np.testing.assert_allclose(host(torch.stack(symmetry_losses)), g[tag + "_symmetry"][:seen], rtol=2e-5, atol=1e-6)
    clipped = g[tag + ("_grads_unclipped" if agent.flat_optimizer is not None else "_grads")]
    assert len(trace["grads_unclipped"]) == len(g[tag + "_grads_unclipped"])
    for step, (raw, after) in enumerate(zip(trace["grads_unclipped"], trace["grads"])):
        gradient_parity(f"symmetry.grads_unclipped[{tag},{mode},{step}]", host(raw), g[tag + "_grads_unclipped"][step], 1e-5)
        gradient_parity(f"symmetry.grads[{tag},{mode},{step}]", host(after), clipped[step], 1e-5)
    np.testing.assert_allclose(host(torch.stack(trace["params_after"])), g[tag + "_params_after"], rtol=1e-4, atol=2e-6)
    ref = dict(zip((str(k) for k in g[tag + "_metric_keys"]), g[tag + "_metric_vals"]))
    for key in ("Agent/value_loss", "Agent/surrogate_loss", "Agent/entropy_loss", "Agent/action_mean_symmetry_loss",
                "Agent/action_std_symmetry_loss"):
        if key in ref:
            np.testing.assert_allclose(metrics[key], ref[key], rtol=1e-3, atol=1e-5, err_msg=key)
