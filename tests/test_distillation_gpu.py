"""Policy distillation on an MI355X: ``cusrl_bias_act`` against float64 and against torch's own fp32 device expression, its
error codes, ``ExpertPolicy`` against the reference's float64 outputs with its launch census, the hook inside a captured rollout
against the host-driven loop, and the reference's recorded three-update trace of the `distillation` preset (golden
``distillation.npz``).

Measured on an MI355X (what DESIGN.md "Distillation" quotes; the tests print the figures).  Largest error in fp32 ulp against
float64 over every kernel case, kernel / torch's fp32 device expression on the same inputs: identity 0 / 0, ReLU 0 / 0, ELU
(alpha 1 and 0.5) 0.808 / 0.808, Tanh 1.284 / 1.284; on the special values ELU 0.154 / 0.154, Tanh 0.341 / 0.341.  ``ExpertPolicy``
against the reference's float64 outputs, of the largest entry: ReLU 1.75e-7, ELU 1.78e-7, Tanh 1.90e-7.  The agent's trace, both
with and without ``compile``: ``distillation_loss`` within 1.8e-7 relative, parameters within 1.5e-8."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import _bijectors
import _distillation as shared

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 1e-5  # the package's parity bar: of the tensor's largest entry
ROWS = (1, 3, 257)
WIDTHS = (1, 3, 4, 12, 64, 260)
CASES = (("identity", 1.0), ("relu", 1.0), ("elu", 1.0), ("elu", 0.5), ("tanh", 1.0))
SYMBOL = "cusrl_bias_act"


@pytest.fixture(scope="module")
def cusrl():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    import cusrl_amd

    cusrl_amd.config.set_device(DEV)
    return cusrl_amd


@pytest.fixture(scope="module")
def g(golden):
    return golden("distillation")


def _count(symbol=SYMBOL):
    from cusrl_amd import _native

    return _native.launch_counts.get(symbol, 0)


def _act(v, activation, alpha):
    """torch's expression, in the dtype of ``v``."""
    if activation == "relu":
        return torch.relu(v)
    if activation == "elu":
        return torch.nn.functional.elu(v, alpha)
    if activation == "tanh":
        return torch.tanh(v)
    return v


def _formula64(x, bias, activation, alpha):
    """The float64 formula of include/cusrl_hip.h on the fp32 sum (the one rounding both device forms share)."""
    v = (x + bias).double()
    if activation == "relu":
        return torch.where(v > 0, v, torch.where(v.isnan(), v, torch.zeros_like(v)))
    if activation == "elu":
        return torch.where(v > 0, v, alpha * torch.expm1(v))
    if activation == "tanh":
        return torch.tanh(v)
    return v


def _operands(rows, width, seed):
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, width, generator=gen) * 3.0).to(DEV)
    bias = torch.randn(width, generator=gen).to(DEV)
    return x, bias


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("activation,alpha", CASES)
def test_kernel_matches_float64_and_torch(cusrl, activation, alpha):
    """Every shape of ROWS x WIDTHS, out of place, in place and from a base pointer offset by one float (the 4-byte form at
    H % 4 == 0): within 1e-5 of the largest entry of the float64 formula and of torch's fp32 device expression, and — over all
    cases — an error in ulp of at most twice that of torch's expression on the same inputs."""
    from cusrl_amd import ops

    worst = {"kernel": 0.0, "torch": 0.0}
    before = _count()
    launches = 0
    for rows in ROWS:
        for width in WIDTHS:
            x, bias = _operands(rows, width, 1000 * rows + width)
            want = _formula64(x, bias, activation, alpha)
            ref = _act(x + bias, activation, alpha)
            assert ops.bias_act_supported(x, bias)
            out = ops.bias_act(x, bias, activation, alpha)
            into = torch.full_like(x, float("nan"))
            assert ops.bias_act(x, bias, activation.upper(), alpha, out=into) is into
            in_place = x.clone()
            assert ops.bias_act(in_place, bias, activation, alpha, out=in_place) is in_place
            # one float into a 16-byte aligned allocation: x, bias and out all on the 4-byte form, guard words on both sides
            x_store = torch.zeros(rows * width + 2, device=DEV)
            b_store = torch.zeros(width + 2, device=DEV)
            o_store = torch.full((rows * width + 2,), 7.0, device=DEV)
            x_off, b_off, o_off = x_store[1:-1].view(rows, width), b_store[1:-1], o_store[1:-1].view(rows, width)
            x_off.copy_(x)
            b_off.copy_(bias)
            assert x_off.data_ptr() % 16 == 4 and o_off.data_ptr() % 16 == 4 and b_off.data_ptr() % 16 == 4
            ops.bias_act(x_off, b_off, activation, alpha, out=o_off)
            assert o_store[0] == 7.0 and o_store[-1] == 7.0, "wrote outside the matrix"
            launches += 4
            for name, got in (("out of place", out), ("out=", into), ("in place", in_place), ("offset", o_off)):
                assert torch.isfinite(got).all(), name
                assert torch.equal(got, out), f"{activation} [{rows}, {width}] {name}: other bits than the out-of-place launch"
                for label, reference in (("float64", want), ("torch", ref)):
                    error = _bijectors.relative_to_largest(got, reference)
                    assert error <= BOUND, f"{activation} [{rows}, {width}] {name} vs {label}: {error:.3e} exceeds {BOUND:.0e}"
            worst["kernel"] = max(worst["kernel"], _bijectors.ulp_error(out, want))
            worst["torch"] = max(worst["torch"], _bijectors.ulp_error(ref, want))
    assert _count() - before == launches
    print(f"{activation} alpha {alpha}: largest error in fp32 ulp against float64 over {len(ROWS) * len(WIDTHS)} shapes: "
          f"kernel {worst['kernel']:.3f} / torch {worst['torch']:.3f}")
    assert worst["kernel"] <= 2 * worst["torch"], f"{worst['kernel']:.3f} ulp is more than twice torch's {worst['torch']:.3f}"


@pytest.mark.parametrize("activation,alpha", CASES)
def test_kernel_special_values(cusrl, activation, alpha):
    """+-0, +-Inf, NaN, -1e-8, -100, +-20 and the largest and smallest normal numbers, on the 16-byte and the 4-byte form: NaN
    and Inf where the float64 formula has them, everything else within 1e-5 of the largest finite entry and within twice
    torch's error in ulp."""
    from cusrl_amd import ops

    tiny, huge = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
    values = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), -1e-8, -100.0, 20.0, -20.0, huge, -huge, tiny, -tiny, 1.0, -1.0, 88.0]
    for width in (4, 1):  # the 16-byte and the 4-byte form
        x = torch.tensor(values, device=DEV).repeat(width).view(width, -1).t().contiguous().view(-1, width)
        bias = torch.zeros(width, device=DEV)
        want = _formula64(x, bias, activation, alpha)
        ref = _act(x + bias, activation, alpha)
        got = ops.bias_act(x, bias, activation, alpha)
        assert torch.equal(got.isnan(), want.isnan()), f"{activation}: NaN does not propagate as the formula's"
        assert torch.equal(got.isinf(), want.float().isinf()) and torch.equal(got[got.isinf()], want.float()[got.isinf()])
        finite = torch.isfinite(want.float())
        for label, reference in (("float64", want), ("torch", ref)):
            error = _bijectors.relative_to_largest(got[finite], reference[finite])
            assert error <= BOUND, f"{activation} width {width} vs {label}: {error:.3e}"
        kernel_ulp, torch_ulp = _bijectors.ulp_error(got[finite], want[finite]), _bijectors.ulp_error(ref[finite], want[finite])
        print(f"{activation} alpha {alpha} width {width}: special values, ulp kernel {kernel_ulp:.3f} / torch {torch_ulp:.3f}")
        assert kernel_ulp <= 2 * torch_ulp or kernel_ulp == 0.0
        if activation == "tanh":
            assert got[x[:, 0] == huge].eq(1.0).all() and got[x[:, 0] == float("-inf")].eq(-1.0).all(), "tanh overflowed"
        if activation == "elu":
            assert got[x[:, 0] == float("-inf")].eq(-alpha).all() and got[x[:, 0] == -100.0].eq(-alpha).all()
            small = got[x[:, 0] == np.float32(-1e-8)].double() / (alpha * float(np.float32(-1e-8)))
            assert small.numel() and ((small - 1).abs() < 1e-6).all(), "expm1, not exp - 1"
    # a NaN or Inf in the bias reaches its column only
    x, bias = _operands(5, 8, 3)
    bias[2], bias[5] = float("nan"), float("inf")
    got = ops.bias_act(x, bias, activation, alpha)
    assert got[:, 2].isnan().all() and not got[:, [0, 1, 3, 4, 6, 7]].isnan().any()
    assert (got[:, 5] == (1.0 if activation == "tanh" else float("inf"))).all()


def test_error_codes_launch_nothing(cusrl):
    from cusrl_amd import _native, ops

    lib = _native.lib()
    invalid, unsupported = _native._CONSTANTS["E_INVALID"], _native._CONSTANTS["E_UNSUPPORTED"]
    x, bias = _operands(3, 4, 9)
    out = torch.full_like(x, 5.0)
    stream = torch.cuda.current_stream().cuda_stream
    relu = _native._CONSTANTS["ACT_RELU"]
    args = lambda **k: tuple({**dict(x=x.data_ptr(), bias=bias.data_ptr(), out=out.data_ptr(), rows=3, H=4, activation=relu,  # noqa: E731
                                     alpha=ctypes.c_float(1.0), stream=stream), **k}.values())
    for name in ("x", "bias", "out"):
        assert lib.cusrl_bias_act(*args(**{name: None})) == invalid, name
    assert lib.cusrl_bias_act(*args(rows=0)) == invalid
    assert lib.cusrl_bias_act(*args(rows=-1)) == invalid
    assert lib.cusrl_bias_act(*args(H=0)) == invalid
    for code in (4, -1, 99):
        assert lib.cusrl_bias_act(*args(activation=code)) == unsupported, code
    torch.cuda.synchronize()
    assert (out == 5.0).all(), "a refused call launched a kernel"
    assert lib.cusrl_bias_act(*args()) == 0
    assert torch.equal(out, torch.relu(x + bias))
    # the Python entry refuses what the kernel does not take, by name
    with pytest.raises(ValueError, match="unknown activation 'gelu'"):
        ops.bias_act(x, bias, "gelu")
    with pytest.raises(_native.NativeError, match="cusrl_bias_act failed with code -3"):
        ops.bias_act(x, bias, 17)
    for bad in (x.cpu(), x.double(), x.t(), x[0], x[:0]):
        assert not ops.bias_act_supported(bad, bias)
    assert not ops.bias_act_supported(x, bias[:3]) and not ops.bias_act_supported(x, bias.double())
    with pytest.raises(ValueError, match="strided"):
        ops.bias_act(x.t(), bias[:3], "relu")


def test_kernel_is_capture_safe(cusrl):
    from cusrl_amd import ops

    x, bias = _operands(257, 64, 11)
    out = torch.empty_like(x)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        ops.bias_act(x, bias, "elu", out=out)  # warm-up
        with torch.cuda.graph(graph, stream=stream):
            ops.bias_act(x, bias, "elu", out=out)
    x.mul_(-1.5)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ops.bias_act(x, bias, "elu"))


# ------------------------------------------------------------------------------------------------ ExpertPolicy
@pytest.mark.parametrize("activation", shared.ACTIVATIONS)
def test_expert_policy_on_the_device(cusrl, g, activation):
    """The reference's float64 outputs within 1e-5 of the largest entry; exactly one ``cusrl_bias_act`` per layer (and one
    normalise launch) on the device form, none for a CPU, a strided or an autocast input, which still give the right values."""
    *_, observation, output32, output64 = shared.tensors(g, activation)
    expert = shared.native_expert(cusrl, g, activation, DEV)
    x = observation.to(DEV)
    before, normalise = _count(), _count("cusrl_rms_normalize")
    got = expert(x)
    assert _count() - before == shared.LAYERS and _count("cusrl_rms_normalize") - normalise == 1
    assert not got.requires_grad and got.shape == output64.shape
    error = _bijectors.relative_to_largest(got, output64)
    print(f"ExpertPolicy {activation}: device form {error:.3e} of the largest entry against the reference's float64 "
          f"(the reference's own float32: {_bijectors.relative_to_largest(output32, output64):.3e})")
    assert error <= BOUND
    unnormalised = cusrl.ExpertPolicy(shared.tensors(g, activation)[0], shared.tensors(g, activation)[1], activation).to(DEV)
    before, normalise = _count(), _count("cusrl_rms_normalize")
    unnormalised(x)
    assert _count() - before == shared.LAYERS and _count("cusrl_rms_normalize") == normalise

    wide = torch.zeros(x.shape[0], 2 * x.shape[1], device=DEV)
    wide[:, ::2] = x
    strided = wide[:, ::2]
    assert not strided.is_contiguous()
    before = _count()
    others = {"strided": expert(strided), "float64": expert(x.double())}
    with torch.autocast("cuda", dtype=torch.bfloat16):
        others["autocast"] = expert(x)
    assert _count() == before, "the torch expression launches no cusrl_bias_act"
    for name, value in others.items():
        assert value.dtype == torch.float32 and not value.requires_grad, name
        assert _bijectors.relative_to_largest(value, output64) <= BOUND, name
    with pytest.raises(RuntimeError, match="ExpertPolicy received CPU tensors"):
        expert.cpu()(observation)  # a gpu test runs with the host forms shut, like a user's process
    expert.to(DEV)


def test_expert_policy_clamps_like_running_mean_std(cusrl, g):
    weights, biases, mean, std, observation, *_ = shared.tensors(g, "Tanh")
    normalizer = cusrl.RunningMeanStd(shared.K, clamp=0.75).to(DEV)
    normalizer.update((observation * 2).to(DEV))
    torch.manual_seed(3)
    actor = cusrl.Actor.Factory(cusrl.Mlp.Factory(shared.HIDDEN, "Tanh", True), cusrl.NormalDist.Factory())(shared.K, shared.A).to(DEV)
    expert = cusrl.ExpertPolicy.from_actor(actor, normalizer)
    x = observation.to(DEV)
    with torch.no_grad():
        latent = actor.backbone.layers(normalizer.normalize(x))
        want = torch.nn.functional.linear(latent, actor.distribution.mean_head.weight, actor.distribution.mean_head.bias)
    assert (normalizer.normalize(x).abs() == 0.75).any(), "the clamp is exercised"
    assert _bijectors.relative_to_largest(expert(x), want.double()) <= BOUND


# ------------------------------------------------------------------------------------------------ the hook in a rollout
def _train(cusrl, g, expert, capture, iterations=6, **overrides):
    cusrl.set_global_seed(21)
    env = cusrl.testing.DummyTorchEnvironment(num_instances=shared.ENVS, observation_dim=shared.K, action_dim=shared.A, device=DEV)
    key = "expert_path" if isinstance(expert, str) else "expert"
    factory = shared.factory(cusrl, None, compile=True, **{key: expert}, **overrides)
    trainer = cusrl.Trainer(env, factory, num_iterations=iterations, verbose=False)
    trainer.capture_rollout = capture  # (the switch of tests/test_captured_rollout.py)
    before = _count()
    trainer.run_training_loop()
    torch.cuda.synchronize()
    return trainer, _count() - before


def _same_bits(a, b):
    assert set(a.buffer.storage) == set(b.buffer.storage) and "expert_action" in a.buffer.storage
    for key in a.buffer.storage:
        assert torch.equal(a.buffer.storage[key], b.buffer.storage[key]), key
    for (name, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.isfinite(p).all() and torch.equal(p, q), name


def test_captured_rollout_with_a_native_expert_is_bit_identical_to_the_host_driven_loop(cusrl, g):
    host, host_calls = _train(cusrl, g, shared.native_expert(cusrl, g, shared.TRACE_ACTIVATION), capture=False)
    assert host._graphed_rollout is None
    captured, captured_calls = _train(cusrl, g, shared.native_expert(cusrl, g, shared.TRACE_ACTIVATION), capture=True)
    graphed = captured._graphed_rollout
    assert graphed is not None and graphed.captured == shared.STEPS and len(graphed.rollouts) == 1
    hook = captured.agent.hook["policy_distillation"]
    assert hook.native_expert and hook.rollout_capture_safe and hook.post_step_device_free
    assert hook.expert.weight_0.device == captured.agent.device
    print(f"{SYMBOL}: {host_calls} calls host-driven, {captured_calls} with the rollout captured (a replay issues no C call); "
          f"minibatch steps captured: {len(captured.agent._graphed_steps)}")
    assert host_calls >= 6 * shared.STEPS * shared.LAYERS and captured_calls > 0  # (warm-up and capture passes issue C calls)
    assert graphed.rollout_replays + graphed.replays > 0, "nothing was replayed"
    _same_bits(host.agent, captured.agent)
    storage = captured.agent.buffer.storage
    for t in range(shared.STEPS):  # (step by step: the GEMM of another row count may sum in another order)
        assert torch.equal(storage["expert_action"][t], hook.expert(storage["observation"][t])), f"step {t}: not the expert's answer"
    want = shared.teacher(g, shared.TRACE_ACTIVATION).double()(storage["observation"].cpu().double())
    assert _bijectors.relative_to_largest(storage["expert_action"], want) <= BOUND


def test_scripted_expert_keeps_the_rollout_host_driven(cusrl, g, tmp_path):
    path = shared.scripted_expert_file(g, shared.TRACE_ACTIVATION, tmp_path)
    before = _count()
    trainer, calls = _train(cusrl, g, path, capture=True)
    agent, graphed = trainer.agent, trainer._graphed_rollout
    hook = agent.hook["policy_distillation"]
    assert isinstance(hook.expert, torch.jit.ScriptModule) and not hook.native_expert
    assert not hook.rollout_capture_safe and not hook.post_step_device_free and hook.eager_phases() == ("step",)
    assert graphed is None or (graphed.captured == 0 and not graphed.rollouts), "a TorchScript expert was captured"
    assert calls == 0 and _count() == before
    storage = agent.buffer.storage
    with torch.no_grad():
        for t in range(shared.STEPS):
            assert torch.equal(storage["expert_action"][t], hook.expert(storage["observation"][t])), f"step {t}"
    want = shared.teacher(g, shared.TRACE_ACTIVATION).double()(storage["observation"].cpu().double())
    assert _bijectors.relative_to_largest(storage["expert_action"], want) <= BOUND
    assert all(torch.isfinite(p).all() for p in agent.parameters()) and np.isfinite(trainer.last_info["Agent/distillation_loss"])


# ------------------------------------------------------------------------------------------------ the agent
@pytest.mark.parametrize("compile", [False, True])
def test_three_updates_replay_the_reference_trace(cusrl, g, compile):
    """Every update from the recorded buffer: ``distillation_loss`` of the minibatch steps to rtol 2e-5 and the parameters after
    the update to 1e-4 (the bounds of tests/test_agent_gpu.py's update traces: GEMM summation order); the critic's head, which
    gets no gradient, does not move."""
    expert = shared.native_expert(cusrl, g, shared.TRACE_ACTIVATION)
    agent = shared.factory(cusrl, DEV, expert=expert, compile=compile)(
        cusrl.EnvironmentSpec(shared.K, shared.A, num_instances=shared.ENVS, device=DEV))
    assert [hook.name for hook in agent.hook] == [str(name) for name in g["trace_hooks"]]
    named = dict(agent.named_parameters())
    assert list(named) == [str(name) for name in g["param_names"]]
    with torch.no_grad():
        for name, param in named.items():
            param.copy_(torch.from_numpy(g[f"param0/{name}"]).to(DEV))
    critic0 = {name: param.detach().clone() for name, param in named.items() if name.startswith("critic.")}
    assert len(critic0) == 2
    agent.sampler.permutation_device = "cpu"  # CPU-generator permutations reproduce the CPU reference's stream
    losses = []
    outer = agent.hook.objective

    def wrapped(metadata, batch):
        result = outer(metadata, batch)
        value = result["distillation_loss"]
        if isinstance(value, torch.Tensor) and not torch.cuda.is_current_stream_capturing():
            losses.append(value.detach().clone())
        return result

    agent.hook.objective = wrapped
    worst_loss = worst_param = 0.0
    for update in range(shared.UPDATES):
        q = f"{update}_"
        leaves = {str(k): g[f"{q}buffer_in/{k}"] for k in g[q + "buffer_keys"]}
        for t in range(shared.STEPS):
            step = {k: torch.from_numpy(np.ascontiguousarray(v[t])).to(DEV) for k, v in leaves.items() if not k.startswith("action_dist.")}
            step["action_dist"] = {key: torch.from_numpy(leaves["action_dist." + key][t]).to(DEV) for key in ("mean", "std")}
            agent.buffer.push(step)
        assert agent.buffer.full and agent.buffer.cursor == 0
        seen = len(losses)
        torch.manual_seed(99 + update)
        metrics = agent.update()
        expected = g[q + "distillation_loss"]
        got = np.array([float(value) for value in losses[seen:]], dtype=np.float32)
        assert len(got) <= len(expected) and (compile or len(got) == len(expected))
        params = torch.cat([param.detach().reshape(-1) for param in named.values()]).cpu().numpy()
        if len(got):
            worst_loss = max(worst_loss, float(np.abs(got / expected[: len(got)] - 1).max()))
        worst_param = max(worst_param, float(np.abs(params - g[q + "params_after"]).max()))
        print(f"compile={compile}, update {update}: {len(got)} of {len(expected)} steps observed eagerly, distillation_loss "
              f"max relative difference {worst_loss:.3e}, parameters max |difference| {worst_param:.3e}, "
              f"captured minibatch steps {len(agent._graphed_steps)}")
        np.testing.assert_allclose(got, expected[: len(got)], rtol=2e-5, atol=1e-6)
        reference = dict(zip((str(k) for k in g[q + "metric_keys"]), g[q + "metric_vals"]))
        assert metrics["Agent/distillation_loss"] == pytest.approx(reference["Agent/distillation_loss"], rel=2e-5)
        np.testing.assert_allclose(params, g[q + "params_after"], rtol=1e-4, atol=2e-6)
        for name, value in critic0.items():
            assert torch.equal(named[name].detach(), value), f"{name} moved without a gradient"
