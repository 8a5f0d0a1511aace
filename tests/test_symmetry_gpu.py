"""Mirror symmetry on an MI355X: the four HIP entries against torch / float64 restatements, the symmetric statistics against
the reference's golden run, and training runs with the symmetry hooks under compile=True."""

from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def cusrl():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    import cusrl_amd

    cusrl_amd.config.set_device(DEV)
    return cusrl_amd


def _count(name):
    from cusrl_amd import _native

    return _native.launch_counts.get(name, 0)


def _random_def(rng, c_in, c_out, bijective):
    dest = rng.permutation(c_in)[:c_out].tolist() if bijective else rng.integers(0, c_in, c_out).tolist()
    flipped = sorted(rng.choice(c_out, size=c_out // 3, replace=False).tolist())
    return dest, flipped


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _assert_bit_exact(out, expected):
    a, b = out.detach().cpu(), expected.detach().cpu()
    assert a.shape == b.shape
    nan = torch.isnan(b)
    assert torch.equal(torch.isnan(a), nan)
    assert np.array_equal(_bits(a.masked_fill(nan, 0)), _bits(b.masked_fill(nan, 0)))


def _special(x):
    """NaN, +-0 and +-inf down the first column and along the first row."""
    values = torch.tensor([float("nan"), 0.0, -0.0, float("inf"), -float("inf"), 1.5], device=x.device)
    n, k = min(x.shape[0], 6), min(x.shape[1], 6)
    x[:n, 0] = values[:n]
    x[0, :k] = values[:k]
    return x


@pytest.mark.parametrize("c_in", [1, 3, 12, 48, 129, 300])
@pytest.mark.parametrize("rows", [0, 1, 63, 65, 24576])
def test_mirror_rows_is_bit_exact(cusrl, c_in, rows):
    from cusrl_amd.hook import MirrorDef

    rng = np.random.default_rng(c_in * 7 + rows)
    for c_out, bijective in ((c_in, True), (max(1, c_in // 2), True), (c_in + 5, False), (c_in, False)):
        mirror = MirrorDef(*_random_def(rng, c_in, c_out, bijective and c_out <= c_in))
        x = torch.randn(rows, c_in + 3, device=DEV)[:, 2:2 + c_in]  # strided rows
        if rows:
            _special(x)
        before = _count("cusrl_mirror_rows")
        out = mirror(x)
        assert _count("cusrl_mirror_rows") == before + 1
        _assert_bit_exact(out, mirror(x.cpu()))


def test_mirror_rows_million_rows(cusrl):
    from cusrl_amd.hook import MirrorDef

    rng = np.random.default_rng(1)
    mirror = MirrorDef(*_random_def(rng, 48, 48, True))
    x = _special(torch.randn(1_000_000, 48, device=DEV))
    _assert_bit_exact(mirror(x), mirror(x.cpu()))


def test_one_launch_writes_the_augmented_layout(cusrl):
    from cusrl_amd import ops
    from cusrl_amd.hook import MirrorDef

    rng = np.random.default_rng(2)
    R = 24576
    obs_def, act_def = MirrorDef(*_random_def(rng, 48, 48, True)), MirrorDef(*_random_def(rng, 12, 12, True))
    obs, act, adv = _special(torch.randn(R, 48, device=DEV)), torch.randn(R, 12, device=DEV), torch.randn(R, 1, device=DEV)
    out_obs, out_act, out_adv = (torch.empty(R, 2, t.shape[1], device=DEV) for t in (obs, act, adv))
    fields = []
    for src, dst, mirror in ((obs, out_obs, obs_def), (act, out_act, act_def), (adv, out_adv, None)):
        flat, w = dst.view(R, -1), src.shape[1]
        fields += [(src, flat, 0, None), (src, flat, w, None if mirror is None else mirror.device_form(DEV, w))]
    before = _count("cusrl_mirror_rows")
    ops.mirror_rows(fields, R)
    assert _count("cusrl_mirror_rows") == before + 1
    for src, dst, mirror in ((obs, out_obs, obs_def), (act, out_act, act_def)):
        host = src.cpu()
        _assert_bit_exact(dst, torch.cat([host.unsqueeze(1), mirror(host).unsqueeze(1)], dim=1))
    _assert_bit_exact(out_adv, adv.cpu().unsqueeze(1).repeat_interleave(2, dim=1))


@pytest.mark.parametrize("bijective", [True, False])
@pytest.mark.parametrize("c_in", [3, 48, 300])
def test_mirror_backward_matches_autograd(cusrl, bijective, c_in):
    from cusrl_amd.hook import MirrorDef

    rng = np.random.default_rng(c_in)
    c_out = c_in if bijective else 2 * c_in
    mirror = MirrorDef(*_random_def(rng, c_in, c_out, bijective))
    x = torch.randn(1000, c_in, device=DEV, requires_grad=True)
    g = torch.randn(1000, c_out, device=DEV)
    before = _count("cusrl_mirror_rows_bwd")
    (grad,) = torch.autograd.grad(mirror(x), x, g)
    assert _count("cusrl_mirror_rows_bwd") == before + 1
    xh = x.detach().cpu().requires_grad_(True)
    (expected,) = torch.autograd.grad(mirror(xh), xh, g.cpu())
    if bijective:
        _assert_bit_exact(grad, expected)
    else:
        torch.testing.assert_close(grad.cpu(), expected, rtol=1e-6, atol=1e-6)


def _mirror_loss64(mean, mirrored_mean, std, mirrored_std, dest, mult, weight):
    """float64 restatement of MirrorSymmetryLoss and its gradients."""
    leaves = [t.detach().cpu().double().requires_grad_(True) for t in (mean, mirrored_mean)]
    mult64, index = torch.tensor(mult, dtype=torch.float64), torch.tensor(dest)
    loss_mean = ((leaves[0] - leaves[1][..., index] * mult64) ** 2).mean() * weight
    total, loss_std = loss_mean, None
    if std is not None:
        leaves += [t.detach().cpu().double().requires_grad_(True) for t in (std, mirrored_std)]
        loss_std = ((leaves[2] - (leaves[3][..., index] * mult64).abs()) ** 2).mean() * weight
        total = total + loss_std
    grads = torch.autograd.grad(total, leaves)
    return loss_mean, loss_std, grads


@pytest.mark.parametrize("B", [5, 300, 24576])
@pytest.mark.parametrize("std_form", [None, "matrix", "vector"])
@pytest.mark.parametrize("bijective", [True, False])
def test_mirror_mse_matches_float64(cusrl, B, std_form, bijective):
    from cusrl_amd import ops
    from cusrl_amd.hook import MirrorDef

    A, weight = 12, 0.5
    rng = np.random.default_rng(B + A)
    dest, flipped = _random_def(rng, A, A, bijective)
    mirror = MirrorDef(dest, flipped)
    mean, mirrored_mean = torch.randn(B, A, device=DEV), torch.randn(B, A, device=DEV)
    std = mirrored_std = None
    if std_form == "matrix":
        std, mirrored_std = torch.rand(B, A, device=DEV) + 0.1, torch.randn(B, A, device=DEV)
        mirrored_std[0, :3] = 0.0  # abs at 0
    elif std_form == "vector":
        std, mirrored_std = torch.rand(A, device=DEV) + 0.1, torch.randn(A, device=DEV)
        mirrored_std[0] = 0.0
    before = _count("cusrl_mirror_mse_fwd_bwd")
    losses, *grads = ops.mirror_mse_fwd_bwd(mean, mirrored_mean, mirror.device_table(DEV, A), weight, std, mirrored_std)
    assert _count("cusrl_mirror_mse_fwd_bwd") == before + 1
    mult = mirror.multiplier.tolist()
    if std_form == "vector":  # the vector is what every row repeats: the matrix form of the same numbers
        loss_mean, loss_std, ref = _mirror_loss64(mean, mirrored_mean, std.expand(B, A), mirrored_std.expand(B, A), dest, mult, weight)
        ref = (ref[0], ref[1], ref[2].sum(0), ref[3].sum(0))
    else:
        loss_mean, loss_std, ref = _mirror_loss64(mean, mirrored_mean, std, mirrored_std, dest, mult, weight)
    host = losses.cpu().double()
    assert abs(host[0] - loss_mean.item()) <= 1e-6 * abs(loss_mean.item())
    if loss_std is not None:
        assert abs(host[1] - loss_std.item()) <= 1e-6 * abs(loss_std.item())
    for got, expected in zip(grads, ref):
        if expected is None:
            continue
        scale = expected.abs().max().item()
        assert (got.cpu().double() - expected).abs().max().item() <= 1e-6 * scale


@pytest.mark.parametrize("C", [1, 7, 48, 300, 4096])
def test_symmetrize_mean_var_is_bit_exact(cusrl, C):
    from cusrl_amd import ops
    from cusrl_amd.hook import MirrorDef

    rng = np.random.default_rng(C)
    mirror = MirrorDef(*_random_def(rng, C, C, True))
    mean, var = torch.randn(C, device=DEV) * 3, torch.rand(C, device=DEV) * 2
    m, v = mean.cpu(), var.cpu()
    mirrored_mean, mirrored_var = mirror(m), abs(mirror(v))
    expected_var = (v + mirrored_var) / 2 + (m - mirrored_mean) ** 2 / 4
    expected_mean = (m + mirrored_mean) / 2
    before = _count("cusrl_symmetrize_mean_var")
    ops.symmetrize_mean_var_(mean, var, mirror.device_table(DEV, C))
    assert _count("cusrl_symmetrize_mean_var") == before + 1
    _assert_bit_exact(mean, expected_mean)
    _assert_bit_exact(var, expected_var)


def test_symmetric_observation_statistics_match_the_reference(cusrl, golden):
    from types import SimpleNamespace

    from cusrl_amd.hook import MirrorDef, ObservationNormalization

    g = golden("symmetry")
    defs = {name: MirrorDef(g[f"mirror_{name}_dest"].tolist(), g[f"mirror_{name}_flipped"].tolist()) for name in ("observation", "state")}
    for case, with_state in (("s", True), ("o", False)):
        spec = cusrl.EnvironmentSpec(16, 8, state_dim=7 if with_state else None, num_instances=32,
                                     mirror_observation=defs["observation"], mirror_state=defs["state"] if with_state else None)
        agent = SimpleNamespace(environment_spec=spec, observation_dim=16, state_dim=7 if with_state else 16, has_state=with_state,
                                device=torch.device(DEV), inference_mode=False, setup_module=lambda m: m.to(DEV),
                                to_tensor=lambda x: torch.as_tensor(x, device=DEV))
        hook = ObservationNormalization()
        hook.agent = agent
        hook.init()
        before = _count("cusrl_symmetrize_mean_var")
        p = f"on_{case}_"
        steps = int(g[p + "steps"])
        for t in range(steps):
            tr = {"observation": torch.from_numpy(g[p + f"obs_in_{t}"]).to(DEV)}
            if with_state:
                tr["state"] = torch.from_numpy(g[p + f"state_in_{t}"]).to(DEV)
            hook.pre_act(tr)
            tr.update(next_observation=torch.from_numpy(g[p + f"next_in_{t}"]).to(DEV), done=torch.from_numpy(g[p + f"done_{t}"]).to(DEV))
            if with_state:
                tr["next_state"] = torch.from_numpy(g[p + f"next_state_in_{t}"]).to(DEV)
            hook.post_step(tr)
            rms = hook.observation_rms
            np.testing.assert_allclose(rms.mean.cpu().numpy(), g[p + f"mean_{t}"], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(rms.var.cpu().numpy(), g[p + f"var_{t}"], rtol=1e-5, atol=1e-6)
            assert float(rms.count) == float(g[p + f"count_{t}"])
            # the reference's invariance: symmetric statistics stay symmetric
            mirror = defs["observation"]
            assert torch.equal(rms.mean, mirror(rms.mean.unsqueeze(0)).squeeze(0))
            assert torch.equal(rms.var, mirror(rms.var.unsqueeze(0)).squeeze(0).abs())
            if with_state:
                np.testing.assert_allclose(hook.state_rms.mean.cpu().numpy(), g[p + f"state_mean_{t}"], rtol=1e-5, atol=1e-6)
                np.testing.assert_allclose(hook.state_rms.var.cpu().numpy(), g[p + f"state_var_{t}"], rtol=1e-5, atol=1e-6)
        per_step = 2 * (2 if with_state else 1)  # pre_act + post_step, observation (+ state)
        assert _count("cusrl_symmetrize_mean_var") - before == steps * per_step


def _mirrored_env(cusrl, N=256):
    from cusrl_amd.hook import MirrorDef

    env = cusrl.testing.DummyTorchEnvironment(num_instances=N, observation_dim=12, action_dim=4, device=DEV)
    env.spec.mirror_observation = MirrorDef([1, 0, 3, 2, 4, 5, 7, 6, 8, 9, 11, 10], [4, 8, 9])
    env.spec.mirror_action = MirrorDef([1, 0, 2, 3], [2])
    return env


def _factory(cusrl, extra_hooks, compile=True):
    factory = cusrl.preset.PpoAgentFactory(num_steps_per_update=8, sampler_epochs=2, sampler_mini_batches=2, compile=compile,
                                           normalize_observation=True, optimizer_kwargs={"capturable": True, "fused": True})
    underlying = factory.to_underlying()
    for hook, where in extra_hooks:
        underlying.register_hook(hook, **where)
    return underlying


def test_training_with_symmetry_hooks_under_compile(cusrl):
    from cusrl_amd.hook import MirrorSymmetryLoss, SymmetricDataAugmentation

    cusrl.set_global_seed(3)
    env = _mirrored_env(cusrl)
    hooks = [(SymmetricDataAugmentation(), {"before": "value_loss"}),
             (MirrorSymmetryLoss(0.5, symmetrize_action_std=True), {"after": "ppo_surrogate_loss"})]
    counts = {k: _count(k) for k in ("cusrl_mirror_rows", "cusrl_mirror_mse_fwd_bwd", "cusrl_symmetrize_mean_var",
                                     "cusrl_ppo_loss_fwd_bwd")}
    trainer = cusrl.Trainer(env, _factory(cusrl, hooks), num_iterations=4, verbose=False)
    trainer.run_training_loop()
    for key, before in counts.items():
        assert _count(key) > before, key
    info = trainer.last_info
    for key in ("action_mean_symmetry_loss", "action_std_symmetry_loss", "value_loss", "surrogate_loss"):
        assert any(k.endswith(key) for k in info), key
    for key, value in info.items():
        if "loss" in key:
            assert np.isfinite(value), key
    for _, p in trainer.agent.named_parameters():
        assert torch.isfinite(p).all()


def test_transition_mirroring_keeps_the_captured_rollout(cusrl):
    from cusrl_amd.hook import TransitionMirroring

    cusrl.set_global_seed(5)
    env = _mirrored_env(cusrl, N=64)
    factory = _factory(cusrl, [(TransitionMirroring(), {"index": 0})])
    before = _count("cusrl_mirror_rows")
    trainer = cusrl.Trainer(env, factory, num_iterations=4, verbose=False)
    trainer.run_training_loop()
    graphed = trainer._graphed_rollout
    assert graphed is not None and graphed.captured > 0 and len(graphed.rollouts) == 1  # the whole rollout, one graph
    assert _count("cusrl_mirror_rows") > before
    for _, p in trainer.agent.named_parameters():
        assert torch.isfinite(p).all()


def test_a_table_of_another_shape_is_refused_on_the_host(cusrl):
    from cusrl_amd import ops
    from cusrl_amd.hook import MirrorDef

    mirror = MirrorDef([1, 0, 2], [0])
    x = torch.randn(4, 3, device=DEV)
    wrong = mirror.device_table(DEV, 5)  # built for 5-wide inputs
    before = _count("cusrl_mirror_rows")
    with pytest.raises(ValueError, match="mirror table"):
        ops.mirror_rows([(x, torch.empty(4, 3, device=DEV), 0, (wrong, 3, 3))], 4)
    with pytest.raises(ValueError, match="mirror table"):
        ops.mirror_rows_bwd(torch.randn(4, 3, device=DEV), wrong, 3)
    assert _count("cusrl_mirror_rows") == before  # nothing reached the device


def test_a_state_mirror_without_a_state_is_unused(cusrl):
    from types import SimpleNamespace

    from cusrl_amd.hook import MirrorDef, ObservationNormalization

    observation_mirror = MirrorDef([1, 0, 2, 3], [2])
    state_mirror = MirrorDef([6, 5, 4, 3, 2, 1, 0], [])  # reads 7 columns: no 4-wide input has them
    spec = cusrl.EnvironmentSpec(4, 2, num_instances=8, mirror_observation=observation_mirror, mirror_state=state_mirror)
    agent = SimpleNamespace(environment_spec=spec, observation_dim=4, state_dim=4, has_state=False, device=torch.device(DEV),
                            inference_mode=False, setup_module=lambda m: m.to(DEV), to_tensor=lambda x: torch.as_tensor(x, device=DEV))
    hook = ObservationNormalization()
    hook.agent = agent
    hook.init()
    transition = {"observation": torch.randn(8, 4, device=DEV)}
    hook.pre_act(transition)
    assert torch.equal(hook.observation_rms.mean, observation_mirror(hook.observation_rms.mean.unsqueeze(0)).squeeze(0))
