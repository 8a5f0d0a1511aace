"""The symmetric actor on an MI355X: the three head launches against torch's fp32 expression (bit for bit) and the float64
restatement (tests/_symmetric_actor.py), ``SymmetricActor`` against the reference's recorded run (golden ``symmetric_actor.npz``),
its equivariance, its launch counts, the replay of the reference's two updates and training under compile=True."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import _symmetric_actor as restated

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = [0, 1, 63, 65, 257]  # the edges of a 64-lane wave and of one 256-thread block
WIDTHS = [1, 3, 12, 16, 17]  # both sides of the narrow-head limit (16)
TABLES = [(A, bijective) for A in WIDTHS for bijective in (True, False) if bijective or A >= 3]
TAGS = ("normal", "adaptive")


@pytest.fixture(scope="module")
def cusrl():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    import cusrl_amd

    cusrl_amd.config.set_device(DEV)
    return cusrl_amd


def _count(name):
    from cusrl_amd import _native

    return _native.launch_counts.get(name, 0)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _assert_bit_exact(out, expected):
    a, b = out.detach().cpu(), expected.detach().cpu()
    assert a.shape == b.shape
    nan = torch.isnan(b)
    assert torch.equal(torch.isnan(a), nan)
    assert np.array_equal(_bits(a.masked_fill(nan, 0)), _bits(b.masked_fill(nan, 0)))


def _special(x):
    """NaN, +-0 and +-inf down the first column and along the first row (as in test_symmetry_gpu.py)."""
    values = torch.tensor([float("nan"), 0.0, -0.0, float("inf"), -float("inf"), 1.5])
    n, k = min(x.shape[0], 6), min(x.shape[1], 6)
    x[:n, 0] = values[:n]
    x[0, :k] = values[:k]
    return x


def _case(A, bijective, B, std_form, seed=0, special=True):
    """Host operands of one case: the mirror, mean2 [2B, A] and std2 ([2B, A] or [A]) whose mirrored half has negative entries
    (so M(std_m) is negative with and without a flip) and exact zeros of both signs."""
    from cusrl_amd.hook import MirrorDef

    rng = np.random.default_rng(1000 * A + 10 * B + bijective + seed)
    dest, flipped = restated.mirror_case(rng, A, bijective)
    gen = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    mean2 = torch.randn(2 * B, A, generator=gen)
    std2 = torch.rand(A if std_form == "vector" else (2 * B, A), generator=gen) + 0.1
    std2 = torch.where(torch.rand(std2.shape, generator=gen) < 0.3, -std2, std2)
    if std_form == "matrix":
        std2[:B] = std2[:B].abs()
        if special and B:
            _special(mean2[:B]), _special(mean2[B:]), _special(std2[B:])
            mean2[B:] = mean2[B:].roll(1, 0)  # (not the same rows as the original half's)
        if B > 2:
            std2[B + 1, -1], std2[B + 2, -1] = 0.0, -0.0
    elif A >= 3:
        std2[-1] = 0.0
    return MirrorDef(dest, flipped), dest, flipped, mean2, std2


def _torch_combine(mirror, mean2, std2, B):
    """The reference's fp32 expression (symmetry.py:450-453) on host tensors."""
    std_o, std_m = (std2.expand(B, -1),) * 2 if std2.dim() == 1 else (std2[:B], std2[B:])
    return (mean2[:B] + mirror(mean2[B:])) / 2, (std_o + mirror(std_m).abs()) / 2


@pytest.mark.parametrize("std_form", ["matrix", "vector"])
@pytest.mark.parametrize("B", ROWS)
@pytest.mark.parametrize("A,bijective", TABLES)
def test_forward_is_bit_exact(cusrl, A, bijective, B, std_form):
    from cusrl_amd import ops

    mirror, _, _, mean2, std2 = _case(A, bijective, B, std_form)
    table = mirror.device_table(DEV, A)
    before = _count("cusrl_symmetric_head_fwd")
    mean, std = ops.symmetric_head_fwd(mean2.to(DEV), std2.to(DEV), table)
    assert _count("cusrl_symmetric_head_fwd") == before + 1
    expected_mean, expected_std = _torch_combine(mirror, mean2, std2, B)
    assert mean.shape == std.shape == (B, A)
    _assert_bit_exact(mean, expected_mean)
    _assert_bit_exact(std, expected_std)
    if B >= 63 and std_form == "matrix":
        assert (mirror(std2[B:]) < 0).any()  # the case does hold a negative M(std_m)


def _check_half(got, g, operand_m, dest, flipped, through_abs, bijective, expected32):
    """One operand's stacked gradient [2B, A] against the formulas."""
    B = g.shape[0]
    d_o, d_m, magnitudes, counts = restated.combine_backward64(g.numpy(), operand_m, dest, flipped, through_abs)
    _assert_bit_exact(got[:B], g / 2)
    got_m = got[B:].cpu()
    if bijective:  # every sum has one term: the bits of torch's own backward
        _assert_bit_exact(got_m, expected32[B:])
    else:
        bound = (np.maximum(counts, 1) - 1)[None, :] * 2.0**-24 * magnitudes  # the fp32 bound of an n-term sum
        assert (np.abs(got_m.double().numpy() - d_m) <= bound).all()
        assert (counts == 0).any() and (counts > 1).any()
    assert torch.equal(got_m[:, counts == 0], torch.zeros(B, int((counts == 0).sum())))  # nobody reads them: exactly 0
    return d_o, d_m, magnitudes


@pytest.mark.parametrize("B", ROWS)
@pytest.mark.parametrize("A,bijective", TABLES)
def test_backward_of_the_matrix_form(cusrl, A, bijective, B):
    from cusrl_amd import ops

    mirror, dest, flipped, mean2, std2 = _case(A, bijective, B, "matrix", special=False)
    gen = torch.Generator().manual_seed(A + B)
    g_mean, g_std = torch.randn(B, A, generator=gen), torch.randn(B, A, generator=gen)
    table = mirror.device_table(DEV, A)
    before = _count("cusrl_symmetric_head_bwd")
    runs = [ops.symmetric_head_bwd(g_mean.to(DEV), g_std.to(DEV), std2.to(DEV), table, want_bias=True) for _ in range(2)]
    assert _count("cusrl_symmetric_head_bwd") == before + 2
    for first, second in zip(*runs):  # the same bits every time
        assert first.shape in ((2 * B, A), (A,)) and np.array_equal(_bits(first), _bits(second))
    d_mean2, d_std2, d_bias = runs[0]
    m, s = mean2.clone().requires_grad_(True), std2.clone().requires_grad_(True)
    expected = torch.autograd.grad(_torch_combine(mirror, m, s, B), (m, s), (g_mean, g_std))
    d_o, d_m, magnitudes = _check_half(d_mean2, g_mean, None, dest, flipped, False, bijective, expected[0])
    # the head bias's gradient: the column sums over B of both halves, within 1e-5 of the summed magnitudes of their terms
    summed = (np.abs(d_o) + magnitudes).sum(axis=0)
    assert (np.abs(d_bias.double().cpu().numpy() - (d_o + d_m).sum(axis=0)) <= 1e-5 * summed).all()
    _check_half(d_std2, g_std, std2[B:].numpy(), dest, flipped, True, bijective, expected[1])
    zero = (std2[B:] == 0)
    if B > 2:
        assert zero.any() and (d_std2[B:].cpu()[zero] == 0).all()  # sgn(0) = 0, for either zero
    only_mean, none, no_bias = ops.symmetric_head_bwd(g_mean.to(DEV), None, std2.to(DEV), table)
    assert none is None and no_bias is None and np.array_equal(_bits(only_mean), _bits(d_mean2))
    none, only_std, no_bias = ops.symmetric_head_bwd(None, g_std.to(DEV), std2.to(DEV), table, want_bias=True)
    assert none is None and no_bias is None and np.array_equal(_bits(only_std), _bits(d_std2))


@pytest.mark.parametrize("std_form", ["matrix", "vector"])
@pytest.mark.parametrize("B", [1, 65, 257, 20000])
def test_bias_gradient_of_a_self_flipped_column_is_exactly_zero(cusrl, B, std_form):
    """Columns 6 and 7 of the golden action mirror read themselves with a flip: d_o + d_m is g / 2 - g / 2 in every row, and the
    row-paired column sum is exactly 0 (the reference's two passes cancel exactly, too); the other columns are not."""
    from cusrl_amd import ops
    from cusrl_amd.hook import MirrorDef

    mirror = MirrorDef([1, 0, 3, 2, 5, 4, 6, 7], [6, 7])
    gen = torch.Generator().manual_seed(B)
    g_mean, g_std = torch.randn(B, 8, generator=gen), torch.randn(B, 8, generator=gen)
    std2 = torch.rand(8 if std_form == "vector" else (2 * B, 8), generator=gen) + 0.1
    _, d_std2, d_bias = ops.symmetric_head_bwd(g_mean.to(DEV), g_std.to(DEV), std2.to(DEV), mirror.device_table(DEV, 8), want_bias=True)
    d_bias = d_bias.cpu()
    assert d_bias.shape == (8,) and (d_bias[6:] == 0).all() and (d_bias[:6] != 0).all()
    pairs = (g_mean[:, [0, 2, 4]] + g_mean[:, [1, 3, 5]]).double().sum(0) / 2  # columns (0, 1), (2, 3), (4, 5) swap
    bound = 1e-5 * g_mean[:, :6].abs().double().sum(0).view(3, 2).sum(1) / 2
    assert ((d_bias[[0, 2, 4]].double() - pairs).abs() <= bound).all() and torch.equal(d_bias[[0, 2, 4]], d_bias[[1, 3, 5]])
    if std_form == "vector":  # (the std vector's column sums share the launch and its finalize)
        assert d_std2.shape == (8,) and torch.isfinite(d_std2).all()


# (20000 rows: more than one block of rows per column, so the column sums go through the finalize launch)
@pytest.mark.parametrize("A,bijective,B", [(*table, B) for table in TABLES for B in ROWS] + [(3, False, 20000), (17, True, 20000)])
def test_backward_of_the_vector_form(cusrl, A, bijective, B):
    from cusrl_amd import ops

    mirror, dest, flipped, _, std2 = _case(A, bijective, B, "vector")
    gen = torch.Generator().manual_seed(A + B)
    g_mean, g_std = torch.randn(B, A, generator=gen), torch.randn(B, A, generator=gen)
    table = mirror.device_table(DEV, A)
    runs = [ops.symmetric_head_bwd(g_mean.to(DEV), g_std.to(DEV), std2.to(DEV), table) for _ in range(2)]
    for first, second in zip(*runs):
        assert (first is None and second is None) or np.array_equal(_bits(first), _bits(second))
    d_mean2, d_std, _ = runs[0]
    assert d_mean2.shape == (2 * B, A) and d_std.shape == (A,)
    std_m = std2.expand(B, -1).numpy()
    d_o, d_m, magnitudes, counts = restated.combine_backward64(g_std.numpy(), std_m, dest, flipped, through_abs=True)
    expected = (d_o + d_m).sum(axis=0)
    summed = (np.abs(d_o) + magnitudes).sum(axis=0)
    # the column sums over B of both halves: within 1e-5 of the summed magnitudes of their terms (the soak's bias-gradient bound)
    assert (np.abs(d_std.double().cpu().numpy() - expected) <= 1e-5 * summed).all()
    if B and A >= 3:  # std2[-1] == 0: its readers contribute nothing, what is left of that column's sum is its own half
        assert std2[-1] == 0 and not magnitudes[:, A - 1].any()
        assert abs(float(d_std[A - 1]) - d_o[:, A - 1].sum()) <= 1e-5 * np.abs(d_o[:, A - 1]).sum()


@pytest.mark.parametrize("std_form", ["matrix", "vector"])
@pytest.mark.parametrize("B", ROWS)
@pytest.mark.parametrize("A,bijective", TABLES)
def test_sample_with_a_supplied_eps(cusrl, A, bijective, B, std_form):
    from cusrl_amd import ops

    mirror, _, _, mean2, std2 = _case(A, bijective, B, std_form, special=False)
    std2 = torch.where(std2 == 0, torch.full_like(std2, 0.25), std2)  # (a log-prob needs a positive std)
    if std_form == "vector":
        std2 = std2.abs()  # (the vector is the original half, too)
    eps = torch.randn(B, A, generator=torch.Generator().manual_seed(B + A))
    table = mirror.device_table(DEV, A)
    before = _count("cusrl_symmetric_head_sample")
    action, logp, mean, std = ops.symmetric_head_sample(mean2.to(DEV), std2.to(DEV), table, eps.to(DEV))
    assert _count("cusrl_symmetric_head_sample") == before + 1
    expected_mean, expected_std = ops.symmetric_head_fwd(mean2.to(DEV), std2.to(DEV), table)
    _assert_bit_exact(mean, expected_mean)
    _assert_bit_exact(std, expected_std)
    _assert_bit_exact(action, mean.cpu() + std.cpu() * eps)
    assert logp.shape == (B, 1)
    _, expected_logp = restated.sample64(mean.cpu().numpy(), std.cpu().numpy(), eps.numpy())
    # the project's bound for statistics; the action the kernel rounded to fp32 is the one whose log-prob it reports
    reported = restated.normal_logp64(mean.cpu().numpy(), std.cpu().numpy(), action.cpu().numpy())
    np.testing.assert_allclose(logp.cpu().numpy(), reported, rtol=1e-5)
    np.testing.assert_allclose(reported, expected_logp, rtol=1e-5, atol=1e-6 * np.abs(expected_logp).max(initial=0.0))


def test_shapes_outside_the_limits_are_unsupported(cusrl):
    from cusrl_amd import _native, ops
    from cusrl_amd.hook import MirrorDef

    A = _native.MAX_SYMMETRIC_HEAD_ACTIONS + 1
    mirror = MirrorDef(list(range(A)), [0])
    with pytest.raises(_native.NativeError, match="-3"):
        ops.symmetric_head_fwd(torch.randn(4, A, device=DEV), torch.rand(4, A, device=DEV), mirror.device_table(DEV, A))


# ------------------------------------------------------------------------------------------------ SymmetricActor
@pytest.mark.parametrize("tag", TAGS)
def test_actor_matches_the_reference(cusrl, golden, tag, gradient_parity):
    g = golden("symmetric_actor")
    actor = restated.golden_actor(cusrl, g, tag, DEV)
    observation = torch.from_numpy(g[tag + "_observation"]).to(DEV)
    counts = {k: _count(k) for k in ("cusrl_mirror_rows", "cusrl_symmetric_head_fwd", "cusrl_symmetric_head_bwd")}
    action_dist, memory = actor(observation)
    assert memory is None
    np.testing.assert_allclose(action_dist["mean"].detach().cpu().numpy(), g[tag + "_mean"], rtol=1e-5,
                               atol=1e-5 * np.abs(g[tag + "_mean"]).max())
    np.testing.assert_allclose(action_dist["std"].detach().cpu().numpy(), g[tag + "_std"], rtol=1e-5)
    recorded = torch.from_numpy(g[tag + "_action"]).to(DEV)
    logp = actor.compute_logp(action_dist, recorded).detach().cpu().numpy()
    bound = 1e-5 * restated.normal_logp_magnitude64(g[tag + "_mean"], g[tag + "_std"], g[tag + "_action"])
    assert (np.abs(logp - g[tag + "_compute_logp"]) <= bound).all()
    c1, c2 = (torch.from_numpy(g[tag + key]).to(DEV) for key in ("_c1", "_c2"))
    names = [name for name, _ in actor.named_parameters()]
    grads = torch.autograd.grad((action_dist["mean"] * c1).sum() + (action_dist["std"] * c2).sum(),
                                [param for _, param in actor.named_parameters()])
    for key, before in counts.items():
        assert _count(key) == before + 1, key
    for name, grad in zip(names, grads):
        gradient_parity(f"symmetric_actor.grad[{tag},{name}]", grad.cpu().numpy(), g[f"{tag}_grad/{name}"], 1e-5)
    views = actor.intermediate_repr
    assert sorted(views) == ["mirrored.action_dist", "mirrored.backbone.output", "mirrored.observation", "original.action_dist",
                             "original.backbone.output"]
    assert torch.equal(views["mirrored.observation"], actor.mirror_observation(observation))
    assert views["original.backbone.output"].shape == views["mirrored.backbone.output"].shape == (5, 16)
    with torch.no_grad():
        dist, (action, logp), _ = actor.explore(observation, deterministic=True)
    np.testing.assert_allclose(action.cpu().numpy(), g[tag + "_deterministic_action"], rtol=1e-5,
                               atol=1e-5 * np.abs(g[tag + "_mean"]).max())
    bound = 1e-5 * restated.normal_logp_magnitude64(g[tag + "_mean"], g[tag + "_std"], g[tag + "_deterministic_action"])
    assert (np.abs(logp.cpu().numpy() - g[tag + "_deterministic_logp"]) <= bound).all()


def _assert_equivariant(actor, observation, grad: bool):
    """actor(M_o(x)) is (M_a(mean(x)), |M_a(std(x))|), for the self-inverse bijective pair."""
    with torch.set_grad_enabled(grad):
        plain, _ = actor(observation)
        mirrored, _ = actor(actor.mirror_observation(observation))
    mean, std = plain["mean"].detach(), plain["std"].detach()
    scale = float(mean.abs().max())
    torch.testing.assert_close(mirrored["mean"].detach(), actor.mirror_action(mean), rtol=1e-5, atol=1e-5 * scale)
    torch.testing.assert_close(mirrored["std"].detach(), actor.mirror_action(std).abs(), rtol=1e-5, atol=0)


@pytest.mark.parametrize("grad", [True, False])
@pytest.mark.parametrize("tag", TAGS)
def test_actor_is_equivariant(cusrl, golden, tag, grad):
    actor = restated.golden_actor(cusrl, golden("symmetric_actor"), tag, DEV)
    observation = torch.randn(65, 16, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    _assert_equivariant(actor, observation, grad)


def _preset_actor(cusrl, observation_dim=48, action_dim=12):
    from cusrl_amd.hook import MirrorDef, SymmetricActorFactory

    rng = np.random.default_rng(4)
    plain = cusrl.preset.PpoAgentFactory().to_underlying().actor_factory
    factory = SymmetricActorFactory(plain.backbone_factory, plain.distribution_factory, plain.latent_dim,
                                    mirror_observation=MirrorDef(*restated.mirror_case(rng, observation_dim, True)),
                                    mirror_action=MirrorDef(*restated.mirror_case(rng, action_dim, True)))
    return factory(observation_dim, action_dim).to(DEV)


def test_launch_counts(cusrl):
    actor = _preset_actor(cusrl)
    observation = torch.randn(4096, 48, device=DEV)
    names = ("cusrl_mirror_rows", "cusrl_mlp2_forward", "cusrl_symmetric_head_sample", "cusrl_symmetric_head_fwd",
             "cusrl_symmetric_head_bwd", "cusrl_narrow_linear_bwd", "cusrl_input_layer_bwd", "cusrl_relu_bwd_colsum",
             "cusrl_normal_sample_logp")
    with torch.no_grad():
        actor.explore(observation)  # (tables uploaded, kernels loaded)
        before = {k: _count(k) for k in names}
        action_dist, (action, logp), memory = actor.explore(observation)
    moved = {k: _count(k) - before[k] for k in names}
    assert {k: v for k, v in moved.items() if v} == {"cusrl_mirror_rows": 1, "cusrl_mlp2_forward": 1,
                                                     "cusrl_symmetric_head_sample": 1}, moved
    assert action.shape == action_dist["mean"].shape == action_dist["std"].shape == (4096, 12) and logp.shape == (4096, 1)
    assert memory is None and actor.noise_shape is None
    with torch.no_grad():
        before = {k: _count(k) for k in names}
        actor(observation)
    moved = {k: _count(k) - before[k] for k in names}
    assert {k: v for k, v in moved.items() if v} == {"cusrl_mirror_rows": 1, "cusrl_mlp2_forward": 1, "cusrl_symmetric_head_fwd": 1}

    before = {k: _count(k) for k in names}
    action_dist, _ = actor(observation)
    (action_dist["mean"].sum() + action_dist["std"].sum()).backward()
    moved = {k: _count(k) - before[k] for k in names}
    assert moved["cusrl_mirror_rows"] == 1 and moved["cusrl_symmetric_head_fwd"] == 1 and moved["cusrl_symmetric_head_bwd"] == 1
    assert moved["cusrl_mlp2_forward"] == 0 and moved["cusrl_symmetric_head_sample"] == 0
    # each wrapped layer's backward once: what the wrapped actor's own backward over an ordinary batch of 2B rows launches
    layer_launches = ("cusrl_narrow_linear_bwd", "cusrl_input_layer_bwd", "cusrl_relu_bwd_colsum")
    before = {k: _count(k) for k in layer_launches}
    plain, _ = actor.wrapped(torch.randn(8192, 48, device=DEV))
    plain["mean"].sum().backward()
    assert {k: _count(k) - before[k] for k in layer_launches} == {k: moved[k] for k in layer_launches}, moved
    assert moved["cusrl_narrow_linear_bwd"] == 1 and sum(moved[k] for k in layer_launches) <= 3, moved
    for name, param in actor.named_parameters():
        assert param.grad is not None and torch.isfinite(param.grad).all(), name


# ------------------------------------------------------------------------------------------------ the reference's two updates
def _host(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("compiled", [False, True])
def test_two_updates_replay_the_reference_trace(cusrl, golden, compiled):
    """The reference's two recorded updates, replayed from the recorded buffers, parameters held to the bound of the existing
    update-trace replays.  (Action columns 6 and 7 mirror onto themselves with a flip: their head bias has an exactly zero gradient
    in the reference, which is what the row-paired bias sums of cusrl_symmetric_head_bwd are for — Adam turns any rounding residue
    there into steps of the size of the learning rate.)"""
    from cusrl_amd.hook import MirrorDef, SymmetricActor, SymmetricArchitecture
    from cusrl_amd.hook.on_policy.fused import FusedPpoObjective

    g = golden("symmetric_actor")
    p = "trace_"
    kw = dict(zip((str(k) for k in g[p + "factory_keys"]), (int(v) for v in g[p + "factory_vals"])))
    factory = cusrl.preset.PpoAgentFactory(actor_hidden_dims=(32, 16), critic_hidden_dims=(32, 16), device=DEV,
                                           **kw, **({"compile": True} if compiled else {}))
    underlying = factory.to_underlying()
    underlying.register_hook(SymmetricArchitecture())
    indices = []

    class Capture(cusrl.Hook):
        def post_objective(self, metadata, batch):
            indices.append(batch["flat_index"].squeeze(-1).clone())

    underlying.register_hook(Capture().name_("capture_post"), after="gradient_clipping")
    spec = cusrl.EnvironmentSpec(16, 8, num_instances=8, device=DEV,
                                 mirror_observation=MirrorDef(g["observation_dest"].tolist(), g["observation_flipped"].tolist()),
                                 mirror_action=MirrorDef(g["action_dest"].tolist(), g["action_flipped"].tolist()))
    agent = underlying(spec)
    assert isinstance(agent.actor, SymmetricActor) and FusedPpoObjective.mode(agent.hook) == "fused"
    named = dict(agent.named_parameters())
    assert list(named) == [str(n) for n in g[p + "param_names"]]
    with torch.no_grad():
        for name, param in named.items():
            param.copy_(torch.from_numpy(g[f"{p}param0/{name}"]).to(DEV))
    agent.sampler.permutation_device = "cpu"  # CPU-generator permutations reproduce the CPU reference's stream
    agent.hook["on_policy_statistics"].sampler.permutation_device = "cpu"
    for iteration in range(int(g[p + "iterations"])):
        q = f"{p}{iteration}_"
        leaves = {str(k): g[f"{q}buffer_in/{k}"] for k in g[q + "buffer_keys"]}
        for t in range(kw["num_steps_per_update"]):
            step = {k: torch.from_numpy(np.ascontiguousarray(v[t])).to(DEV) for k, v in leaves.items() if not k.startswith("action_dist.")}
            step["action_dist"] = {key: torch.from_numpy(leaves["action_dist." + key][t]).to(DEV) for key in ("mean", "std")}
            agent.buffer.push(step)
        assert agent.buffer.full and agent.buffer.cursor == 0
        seen = len(indices)
        torch.manual_seed(99 + iteration)
        agent.update()
        # (a step replayed from its graph calls no hook: under compile=True the steps that ran on the host are compared)
        got = indices[seen:]
        assert compiled or len(got) == len(g[q + "indices"])
        if got:
            assert np.array_equal(_host(torch.stack(got)), g[q + "indices"][:len(got)]), "minibatch permutations differ"
        for key in ("next_value", "advantage", "return"):
            np.testing.assert_allclose(_host(agent.buffer[key]), g[f"{q}buffer_out/{key}"], rtol=1e-5, atol=2e-6)
        params = torch.cat([param.detach().reshape(-1) for _, param in agent.named_parameters()])
        expected, offset = g[q + "params_after"], 0
        for name, param in agent.named_parameters():  # (each parameter's figure, before anything is asserted)
            part = np.abs(_host(param).reshape(-1) - expected[offset:offset + param.numel()])
            print(f"update {iteration}, compiled={compiled}: {name} max |difference| {part.max():.3e} at entry {int(part.argmax())}")
            offset += param.numel()
        # the bound the update-trace replays hold their parameters to on the GPU: tests/test_agent_gpu.py:144
        np.testing.assert_allclose(_host(params), expected, rtol=1e-4, atol=2e-6)


# ------------------------------------------------------------------------------------------------ training under capture
def _train(cusrl, compile, iterations=3):
    from cusrl_amd.hook import MirrorDef, SymmetricArchitecture

    cusrl.set_global_seed(7)
    env = cusrl.testing.DummyTorchEnvironment(num_instances=64, observation_dim=12, action_dim=4, device=DEV)
    env.spec.mirror_observation = MirrorDef([1, 0, 3, 2, 4, 5, 7, 6, 8, 9, 11, 10], [4, 8, 9])
    env.spec.mirror_action = MirrorDef([1, 0, 2, 3], [2])
    factory = cusrl.preset.PpoAgentFactory(num_steps_per_update=8, sampler_epochs=2, sampler_mini_batches=2, compile=compile,
                                           optimizer_kwargs={"capturable": True, "fused": True}).to_underlying()
    factory.register_hook(SymmetricArchitecture())
    trainer = cusrl.Trainer(env, factory, num_iterations=iterations, verbose=False)
    trainer.run_training_loop()
    return trainer


@pytest.fixture(scope="module")
def trained(cusrl):
    return {key: _train(cusrl, compile) for key, compile in (("eager", False), ("captured", True), ("again", True))}


def _assert_same_bits(a, b):
    assert set(a.buffer.storage) == set(b.buffer.storage)
    for key in a.buffer.storage:
        assert torch.equal(a.buffer.storage[key], b.buffer.storage[key]), key
    for (name, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), name


def test_training_under_capture_is_bit_identical_to_eager(cusrl, trained):
    from cusrl_amd.hook import SymmetricActor

    captured = trained["captured"].agent
    assert isinstance(captured.actor, SymmetricActor) and captured._graphed_steps
    _assert_same_bits(trained["eager"].agent, captured)


def test_the_same_run_twice_is_bit_identical(cusrl, trained):
    _assert_same_bits(trained["captured"].agent, trained["again"].agent)


@pytest.mark.parametrize("grad", [True, False])
def test_a_trained_actor_is_still_equivariant(cusrl, trained, grad):
    actor = trained["captured"].agent.actor
    observation = torch.randn(65, 12, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    _assert_equivariant(actor, observation, grad)
    for _, param in actor.named_parameters():
        assert torch.isfinite(param).all()
