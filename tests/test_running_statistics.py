"""Running observation statistics (``cusrl_masked_col_stats``, ``cusrl_rms_merge``, ``cusrl_rms_normalize``) against plain
high-precision restatements, at the shapes, masks and data where such kernels go wrong: several partial blocks up to the
256-block cap, channel counts around and beyond the 256-lane block, empty / single-row / sparse masks, the float4 and
scalar paths of the normalisation, ``max_count`` and zero batch counts, and data whose mean is large against its spread
(positions in world coordinates, timers: the cancellation of ``E[x^2] - E[x]^2``)."""

import numpy as np
import pytest
import torch

import cusrl_amd as cusrl
import oracle

DEV = "cuda:0"
CONSTANT = np.float32(-12345.678)


def offset_data(rng, shape, C):
    """``[..., C]`` float32 whose channels have spreads from 1e-3 to 1e2 and means up to 1e5 of their spread; the last
    channel (when C > 1) is the constant CONSTANT."""
    std = 10.0 ** rng.uniform(-3, 2, C)
    ratio = np.array([0.0, 1.0, -1e2, 1e3, -1e4, 1e5])[np.arange(C) % 6]
    x = (ratio * std + std * rng.standard_normal((*shape, C))).astype(np.float32)
    if C > 1:
        x[..., -1] = CONSTANT
    return x


def masks(rng, rows):
    """(label, mask or None) pairs: no mask, all, none, a single row, ~5 % (a done rate), as bool and as uint8."""
    sparse = rng.random(rows) < 0.05
    single = np.zeros(rows, bool)
    if rows:
        single[rows // 2] = True
    out = [("none", None), ("all", np.ones(rows, bool)), ("empty", np.zeros(rows, bool)), ("single", single),
           ("sparse", sparse)]
    return out + [(label + "_u8", m.astype(np.uint8)) for label, m in out[1:]]


def check_stats(x, mask, got, label, constant_last=True):
    """The kernel's (mean, var, count) against the float64 two-pass restatement; ``constant_last``: the last channel is
    CONSTANT (offset_data's)."""
    mean, var, count = (t.cpu().numpy() for t in got)
    ref_mean, ref_var, n = oracle.masked_mean_var(x, mask)
    assert count.shape == (1,) and count[0] == n, label  # exact
    if n == 0:  # the header's promise for an empty selection: exactly (0, 1, 0)
        assert np.array_equal(mean, np.zeros_like(mean)) and np.array_equal(var, np.ones_like(var)), label
        return
    if constant_last and x.shape[-1] > 1:  # a constant channel: mean exactly the constant, var exactly 0
        assert mean[-1] == CONSTANT and var[-1] == 0.0, f"{label}: constant channel gives ({mean[-1]!r}, {var[-1]!r})"
    std = np.sqrt(ref_var)
    err_mean = np.abs(mean.astype(np.float64) - ref_mean) / (np.abs(ref_mean) + std)
    err_var = np.abs(var.astype(np.float64) - ref_var) / np.where(ref_var > 0, ref_var, 1.0)
    assert np.all(err_mean <= 1e-6), f"{label}: mean rel. error {err_mean.max():.3g} at channel {err_mean.argmax()}"
    assert np.all(err_var <= 1e-6), f"{label}: var rel. error {err_var.max():.3g} at channel {err_var.argmax()}"


def test_masked_mean_var_restatement_matches_torch_float64():
    rng = np.random.default_rng(5)
    x = offset_data(rng, (300,), 7)
    for label, mask in masks(rng, 300):
        mean, var, n = oracle.masked_mean_var(x, mask)
        rows = torch.from_numpy(x).double()
        if mask is not None:
            rows = rows[torch.from_numpy(mask.astype(bool))]
        assert n == rows.shape[0], label
        if n == 0:
            assert np.array_equal(mean, np.zeros(7)) and np.array_equal(var, np.ones(7)), label
            continue
        ref_var, ref_mean = torch.var_mean(rows, dim=0, correction=0)
        np.testing.assert_allclose(mean, ref_mean.numpy(), rtol=1e-12, atol=0, err_msg=label)
        np.testing.assert_allclose(var, ref_var.numpy(), rtol=1e-9, atol=1e-300, err_msg=label)
        assert var[-1] == 0.0 and mean[-1] == np.float64(CONSTANT), label


# ------------------------------------------------------------------------------------------------ masked_col_stats
SHAPES = [(rows, C) for rows in (0, 1, 7, 4096, 98307) for C in (1, 2, 3, 5, 48, 127, 128, 129, 200, 255, 256, 257, 300, 1024)
          if rows * C <= 40_000_000]  # 98307 x 1024 only slows the host reference: 4096 x 1024 already fills the 256 blocks


@pytest.mark.gpu
@pytest.mark.parametrize("rows,C", SHAPES)
def test_masked_col_stats_vs_float64(rows, C):
    """Every mask kind at every shape; the phases ``base % C`` of the blocks' two-level fold
    (``first = (c - base % C + C) % C``, ``groups = min(256 / (C + 1), 16)``) vary with C, and 98307 rows go past the
    256-partial cap, so the grid-stride loop runs several rounds per lane."""
    from cusrl_amd import ops

    rng = np.random.default_rng(rows * 1000 + C)
    x = offset_data(rng, (rows,), C)
    xd = torch.from_numpy(x).to(DEV)
    cases = masks(rng, rows) if rows < 98307 else [m for m in masks(rng, rows) if m[0] in ("none", "sparse", "empty_u8")]
    for label, mask in cases:
        md = None if mask is None else torch.from_numpy(mask).to(DEV)
        check_stats(x, mask, ops.masked_col_stats(xd, md), f"rows={rows} C={C} mask={label}")


@pytest.mark.gpu
@pytest.mark.parametrize("C", [5, 48, 300])
def test_masked_col_stats_three_dimensional_and_strided_inputs(C):
    from cusrl_amd import ops

    rng = np.random.default_rng(C)
    x = offset_data(rng, (24, 333), C)  # [T, N, C]
    done = rng.random((24, 333)) < 0.05
    check_stats(x, done, ops.masked_col_stats(torch.from_numpy(x).to(DEV), torch.from_numpy(done).to(DEV)), "3-D")
    check_stats(x, None, ops.masked_col_stats(torch.from_numpy(x).to(DEV)), "3-D, no mask")
    # non-contiguous views: every other row of a [T, 2N, C] buffer; channels picked out of a wider row
    wide = torch.from_numpy(offset_data(rng, (24, 666), 2 * C)).to(DEV)
    rows_view = wide[:, ::2, :C]
    assert not rows_view.is_contiguous()
    check_stats(rows_view.cpu().numpy(), done, ops.masked_col_stats(rows_view, torch.from_numpy(done).to(DEV)), "strided",
                constant_last=False)
    cols_view = wide[..., C:]
    check_stats(cols_view.cpu().numpy(), None, ops.masked_col_stats(cols_view), "column slice")


# ------------------------------------------------------------------------------------------------ rms_merge
@pytest.mark.gpu
@pytest.mark.parametrize("C", [3, 256, 300, 1024])
def test_rms_merge_sequence_is_bit_exact(C):
    """~50 successive updates whose batch counts mix 0 and 1 with large ones, on device batch statistics: the merge
    is bit-exact against its fp32 restatement (the build uses -ffp-contract=off and correctly rounded sqrtf).  Then
    the whole update chain against ``oracle.running_mean_std_update``; then ``max_count`` and counts past 2^31."""
    from cusrl_amd import ops

    rng = np.random.default_rng(C)
    eps = 1e-8
    mean, var, std = torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.ones(C, device=DEV)
    count = torch.zeros(1, dtype=torch.float64, device=DEV)
    r_mean, r_var, r_std, r_count = np.zeros(C, np.float32), np.ones(C, np.float32), np.ones(C, np.float32), 0
    chain = (np.zeros(C, np.float32), np.ones(C, np.float32), np.ones(C, np.float32), 0)
    kinds = ["sparse", "empty", "single", "all", "none"]
    for step in range(50):
        rows = int(rng.choice([1, 7, 512, 2048]))
        x = (rng.standard_normal((rows, C)) * rng.uniform(0.5, 2.0, C) + rng.uniform(-3, 3, C)).astype(np.float32)
        mask = dict(masks(rng, rows))[kinds[step % 5]]
        md = None if mask is None else torch.from_numpy(mask).to(DEV)
        b_mean, b_var, b_count = ops.masked_col_stats(torch.from_numpy(x).to(DEV), md)
        before = [t.clone() for t in (mean, var, std, count)]
        ops.rms_merge_(mean, var, std, count, b_mean, b_var, b_count, eps, None)
        n = int(b_count.item())
        if n == 0:  # nothing merged: every buffer bit-unchanged
            assert all(torch.equal(a, b) for a, b in zip(before, (mean, var, std, count))), step
        r_mean, r_var, r_std, r_count = oracle.rms_merge(r_mean, r_var, r_std, r_count, b_mean.cpu().numpy(),
                                                         b_var.cpu().numpy(), n, eps)
        assert np.array_equal(mean.cpu().numpy(), r_mean), step
        assert np.array_equal(var.cpu().numpy(), r_var), step
        assert np.array_equal(std.cpu().numpy(), r_std), step
        assert count.item() == r_count, step
        selected = x if mask is None else x[mask != 0]
        chain = oracle.running_mean_std_update(*chain[:2], chain[3], selected, eps)
        np.testing.assert_allclose(mean.cpu().numpy(), chain[0], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(var.cpu().numpy(), chain[1], rtol=1e-5, atol=1e-6)
        assert count.item() == chain[3]
    # max_count: the count saturates, the weights keep using the uncapped sum of the step
    for cap in (5000.0, 6000.0):
        x = torch.from_numpy(rng.standard_normal((2048, C)).astype(np.float32)).to(DEV)
        b_mean, b_var, b_count = ops.masked_col_stats(x)
        ops.rms_merge_(mean, var, std, count, b_mean, b_var, b_count, eps, cap)
        r_mean, r_var, r_std, r_count = oracle.rms_merge(r_mean, r_var, r_std, r_count, b_mean.cpu().numpy(),
                                                         b_var.cpu().numpy(), 2048, eps, cap)
        assert count.item() == r_count == cap
        assert np.array_equal(mean.cpu().numpy(), r_mean) and np.array_equal(var.cpu().numpy(), r_var)
        assert np.array_equal(std.cpu().numpy(), r_std)
    # a count past 2^31 (an fp64 device value): the new batch weighs ~1e-6
    big = float(3 << 30) + 0.5e9
    count.fill_(big)
    r_count = big
    x = torch.from_numpy((rng.standard_normal((4096, C)) * 4 + 7).astype(np.float32)).to(DEV)
    b_mean, b_var, b_count = ops.masked_col_stats(x)
    ops.rms_merge_(mean, var, std, count, b_mean, b_var, b_count, eps, None)
    r_mean, r_var, r_std, r_count = oracle.rms_merge(r_mean, r_var, r_std, r_count, b_mean.cpu().numpy(),
                                                     b_var.cpu().numpy(), 4096, eps)
    assert count.item() == r_count == big + 4096
    assert np.array_equal(mean.cpu().numpy(), r_mean) and np.array_equal(var.cpu().numpy(), r_var)
    assert np.array_equal(std.cpu().numpy(), r_std)


# ------------------------------------------------------------------------------------------------ rms_normalize
def _normalize_cases(rng):
    """(label, x, mean, std, expect the float4 path)."""
    def stats(C):
        mean = torch.from_numpy(rng.uniform(-2, 2, C).astype(np.float32)).to(DEV)
        std = torch.from_numpy(rng.uniform(0.05, 3, C).astype(np.float32)).to(DEV)
        return mean, std

    def data(rows, C):
        return torch.from_numpy((rng.standard_normal((rows, C)) * 4).astype(np.float32)).to(DEV)

    cases = []
    for C in (4, 48, 256):
        cases.append((f"float4 C={C}", data(1000, C), *stats(C), True))
    for C in (1, 5, 47, 302):
        cases.append((f"scalar C={C}", data(1000, C), *stats(C), False))
    # storage offset by one float: C % 4 == 0 but not 16-byte aligned -> scalar path
    buf = torch.from_numpy((rng.standard_normal(1000 * 48 + 1) * 4).astype(np.float32)).to(DEV)
    cases.append(("offset input", buf[1:].view(1000, 48), *stats(48), False))
    mean, std = stats(49)
    cases.append(("offset statistics", data(1000, 48), mean[1:], std[1:], False))
    # past the 2048-block grid cap on both paths: grid-stride rounds
    cases.append(("float4 grid-stride", data(16384, 256), *stats(256), True))
    cases.append(("scalar grid-stride", data(4096, 302), *stats(302), False))
    return cases


@pytest.mark.gpu
def test_rms_normalize_is_bit_exact_against_torch():
    from cusrl_amd import ops

    rng = np.random.default_rng(11)
    for label, x, mean, std, vec4 in _normalize_cases(rng):
        assert vec4 == (x.shape[-1] % 4 == 0 and all(t.data_ptr() % 16 == 0 for t in (x, mean, std))), label
        for clamp in (5.0, 0.5, None):
            expect = (x - mean) / std
            if clamp is not None:
                expect = expect.clamp(-clamp, clamp)
            got = ops.rms_normalize(x, mean, std, clamp)
            assert torch.equal(got, expect), f"{label} clamp={clamp}: max diff {(got - expect).abs().max().item()}"
    empty = torch.empty(0, 48, device=DEV)
    mean, std = torch.zeros(48, device=DEV), torch.ones(48, device=DEV)
    assert ops.rms_normalize(empty, mean, std, 5.0).shape == (0, 48)


# ------------------------------------------------------------------------------------------------ the module on the device
@pytest.mark.gpu
def test_running_mean_std_groups_excluded_and_state_on_device():
    rms = cusrl.nn.RunningMeanStd(4, groups=[[0, 1]], excluded_indices=[3]).to(DEV)
    x = torch.tensor([[1.0, 3.0, 5.0, 100.0], [3.0, 5.0, 7.0, -100.0]], device=DEV)
    rms.update(x)
    assert rms.count == 2
    assert torch.allclose(rms.mean, torch.tensor([3.0, 3.0, 6.0, 0.0], device=DEV))  # grouped share, excluded stays (0, 1)
    assert torch.allclose(rms.var[3], torch.tensor(1.0, device=DEV)) and torch.allclose(rms.var[0], rms.var[1])
    # the pooled group variance: mean(var) - group_mean^2 + mean(mean^2) = 1 - 9 + 10 (rms.py:221-231)
    assert torch.allclose(rms.var, torch.tensor([2.0, 2.0, 1.0, 1.0], device=DEV))
    state = rms.state_dict()
    other = cusrl.nn.RunningMeanStd(4).to(DEV)
    other.load_state_dict(state)
    assert other.count == 2 and torch.equal(other.mean, rms.mean) and torch.equal(other.std, rms.std)
    assert torch.allclose(rms.unnormalize(rms.normalize(x))[:, :3], x[:, :3], atol=1e-4)  # channel 3 is clamped at +-10
    # a masked update that selects nothing changes nothing
    before = [t.clone() for t in (rms.mean, rms.var, rms.std, rms._count)]
    rms.update(x, mask=torch.zeros(2, dtype=torch.bool, device=DEV))
    assert all(torch.equal(a, b) for a, b in zip(before, (rms.mean, rms.var, rms.std, rms._count)))


@pytest.mark.gpu
@pytest.mark.parametrize("C", [129, 256, 300])
@pytest.mark.parametrize("max_count", [None, 6000])
def test_wide_amp_transition_statistics_vs_oracle(C, max_count):
    """AMP with a transition too wide for cusrl_amp_prepare (C > 128) takes ``transition_rms.update(agent)``,
    ``update(expert)`` and normalises both (amp.py:122-128): the per-op kernels against ``oracle.amp_prepare``."""
    from cusrl_amd import ops

    assert not ops.amp_prepare_supported(4096, C)
    rng = np.random.default_rng(C)
    rms = cusrl.nn.RunningMeanStd(C, max_count=max_count).to(DEV)
    mean, var, count = np.zeros(C, np.float32), np.ones(C, np.float32), 0
    K = C // 2
    dataset = (rng.standard_normal((1000, C)) * 3 + 1).astype(np.float32)
    for step in range(3):
        agent = (rng.standard_normal((4096, C)) * 2 - 0.5).astype(np.float32)
        picks = rng.integers(0, 1000, 4096)
        if C % 2 == 0:
            ref_agent, ref_expert, mean, var, std, count = oracle.amp_prepare(
                agent[:, :K], agent[:, K:], np.arange(K), dataset, picks, mean, var, count, max_count=max_count)
        else:  # an env-provided amp_obs of odd width: the same two updates and normalisations
            mean, var, std, count = oracle.running_mean_std_update(mean, var, count, agent, max_count=max_count)
            mean, var, std, count = oracle.running_mean_std_update(mean, var, count, dataset[picks], max_count=max_count)
            ref_agent, ref_expert = (np.clip((x - mean) / std, -10, 10).astype(np.float32) for x in (agent, dataset[picks]))
        a, e = torch.from_numpy(agent).to(DEV), torch.from_numpy(dataset[picks]).to(DEV)
        rms.update(a)
        rms.update(e)
        got_agent, got_expert = rms.normalize(a), rms.normalize(e)
        np.testing.assert_allclose(got_agent.cpu().numpy(), ref_agent, rtol=1e-5, atol=2e-5)
        np.testing.assert_allclose(got_expert.cpu().numpy(), ref_expert, rtol=1e-5, atol=2e-5)
        np.testing.assert_allclose(rms.mean.cpu().numpy(), mean, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(rms.var.cpu().numpy(), var, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(rms.std.cpu().numpy(), std, rtol=1e-5, atol=1e-6)
        assert rms.count == count


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.gpu
def test_ppo_preset_with_wide_observation_normalization_runs_eager_and_graphed():
    from cusrl_amd import _native

    cusrl.config.set_device(DEV)
    for compile_ in (False, True):
        cusrl.set_global_seed(23)
        before = _native.launch_counts.get("cusrl_masked_col_stats", 0)
        env = cusrl.testing.DummyTorchEnvironment(num_instances=32, observation_dim=300, action_dim=3, device=DEV)
        factory = cusrl.preset.PpoAgentFactory(num_steps_per_update=6, sampler_epochs=2, sampler_mini_batches=2,
                                               normalize_observation=True, compile=compile_,
                                               optimizer_kwargs={"capturable": True, "fused": True})
        trainer = cusrl.Trainer(env, factory, num_iterations=3, verbose=False)
        trainer.run_training_loop()
        assert _native.launch_counts.get("cusrl_masked_col_stats", 0) > before, compile_
        rms = trainer.agent.hook["observation_normalization"].observation_rms
        assert rms.mean.shape == (300,) and rms.count > 0
        assert torch.isfinite(rms.mean).all() and torch.isfinite(rms.std).all()
        assert np.isfinite(trainer.last_info["Agent/value_loss"]), compile_
        assert np.isfinite(trainer.last_info["Agent/surrogate_loss"]), compile_
