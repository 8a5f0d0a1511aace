"""The bijector kernel and the modules built on it on an MI355X: both launches of both kinds against the float64 evaluation of
their formulas and against torch's own fp32 device expression, views, special values, error codes, the launch census, the
fallbacks, the distributions and a captured PPO agent whose std goes through the bounded sigmoid.

Measured on an MI355X over every kernel case (what DESIGN.md "Std bijectors" quotes), largest error in fp32 ulp against float64,
kernel / torch's fp32 device expression on the same inputs: softplus forward 1.620 / 1.620, backward 2.390 / 2.638; sigmoid
forward 2.455 / 2.455 and backward 1.68e7 / 1.68e7 (the fp32 ``(1 - s) s`` is 0 beyond ``|x|`` of about 17: the formula's error,
the same bits as torch); every tensor within 1e-7 of the largest entry; modules against the torch expression at most 1.8e-7."""

from __future__ import annotations

import copy

import numpy as np
import pytest
import torch

import _bijectors
from _bijectors import BOUND, SPECS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD, BWD = "cusrl_bijector_fwd", "cusrl_bijector_bwd"


@pytest.fixture(scope="module")
def cusrl():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    import cusrl_amd

    cusrl_amd.config.set_device(DEV)
    return cusrl_amd


def _counts():
    from cusrl_amd import _native

    return _native.launch_counts.get(FWD, 0), _native.launch_counts.get(BWD, 0)


def _delta(before):
    return tuple(now - then for now, then in zip(_counts(), before))


def _kernel(bijector, x, dy):
    """``(y, dx)`` through the autograd Function: exactly one forward and one backward launch."""
    leaf = x.detach().requires_grad_(True)
    before = _counts()
    y = bijector(leaf)
    (dx,) = torch.autograd.grad(y, leaf, grad_outputs=dy)
    assert _delta(before) == (1, 1), "one forward and one backward launch"
    return y.detach(), dx


def _torch(bijector, x, dy):
    """The same through torch's own fp32 device expression; launches nothing of ours."""
    leaf = x.detach().requires_grad_(True)
    before = _counts()
    y = _bijectors.torch_expression(bijector, leaf)
    (dx,) = torch.autograd.grad(y, leaf, grad_outputs=dy)
    assert _delta(before) == (0, 0)
    return y.detach(), dx


# ------------------------------------------------------------------------------------------------ parity with float64
@pytest.mark.parametrize("spec", SPECS)
def test_kernel_matches_float64(cusrl, golden, spec):
    """Every shape of ROWS x WIDTHS: within 1e-5 of the largest entry of the float64 formulas, the gradient mask torch's, and —
    over all shapes — an error in ulp of at most twice that of torch's fp32 device expression."""
    g = golden("bijectors")
    attrs = _bijectors.attributes(g, spec)
    bijector = cusrl.nn.make_bijector(spec)
    worst = {"kernel": [0.0, 0.0], "torch": [0.0, 0.0]}
    for rows in _bijectors.ROWS:
        for width in _bijectors.WIDTHS:
            x, dy = _bijectors.kernel_case(g, rows, width)
            want = _bijectors.formulas(spec, attrs, x, dy)
            got = _kernel(bijector, x.to(DEV), dy.to(DEV))
            ref = _torch(bijector, x.to(DEV), dy.to(DEV))
            assert got[0].shape == (rows, width) and got[1].shape == (rows, width) and got[0].dtype == torch.float32
            for index, name in enumerate(("y", "dx")):
                assert torch.isfinite(got[index]).all()
                error = _bijectors.relative_to_largest(got[index], want[index])
                assert error <= BOUND, f"{spec} [{rows}, {width}] {name}: {error:.3e} of the largest entry exceeds {BOUND:.0e}"
                worst["kernel"][index] = max(worst["kernel"][index], _bijectors.ulp_error(got[index], want[index]))
                worst["torch"][index] = max(worst["torch"][index], _bijectors.ulp_error(ref[index], want[index]))
            if _bijectors.is_softplus(spec):
                assert torch.equal(got[1] == 0, ref[1] == 0), f"{spec} [{rows}, {width}]: the gradient mask is not torch's"
                low, high = np.float32(attrs["min_input"]), np.float32(attrs["max_input"])
                edges = (x == float(low)) | (x == float(high))
                assert (got[1].cpu()[edges] != 0).all(), "inclusive at the edges"
    print(f"{spec}: largest error in fp32 ulp against float64 over {len(_bijectors.ROWS) * len(_bijectors.WIDTHS)} shapes: "
          f"forward kernel {worst['kernel'][0]:.3f} / torch {worst['torch'][0]:.3f}, "
          f"backward kernel {worst['kernel'][1]:.3f} / torch {worst['torch'][1]:.3f}")
    for index, name in enumerate(("forward", "backward")):
        assert worst["kernel"][index] <= 2 * worst["torch"][index], (
            f"{spec} {name}: {worst['kernel'][index]:.3f} ulp is more than twice torch's {worst['torch'][index]:.3f}")


# ------------------------------------------------------------------------------------------------ views
def _offset_view(t):
    """The same values one float off a 16-byte boundary."""
    buffer = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buffer[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("spec", ("sigmoid_0.05_1.0", "softplus_1_0.01_50"))
def test_misaligned_and_strided_operands(cusrl, golden, spec):
    g = golden("bijectors")
    bijector = cusrl.nn.make_bijector(spec)
    x, dy = (t.to(DEV) for t in _bijectors.kernel_case(g, 257, 4))  # n % 4 == 0: the 16-byte lanes when aligned
    assert x.data_ptr() % 16 == 0 and dy.data_ptr() % 16 == 0
    aligned = _kernel(bijector, x, dy)
    for moved in ((_offset_view(x), dy), (x, _offset_view(dy)), (_offset_view(x), _offset_view(dy))):
        shifted = _kernel(bijector, *moved)  # the 4-byte lanes
        assert torch.equal(shifted[0], aligned[0]) and torch.equal(shifted[1], aligned[1])
    wide_x, wide_dy = (t.to(DEV) for t in _bijectors.kernel_case(g, 48, 257))
    strided_x, strided_dy = wide_x.t(), wide_dy.t()[:, ::2]
    assert not strided_x.is_contiguous() and not strided_dy.is_contiguous()
    leaf = strided_x.detach().requires_grad_(True)
    before = _counts()
    y = bijector(leaf[:, ::2])  # a strided view is made contiguous first
    (dx,) = torch.autograd.grad(y, leaf, grad_outputs=strided_dy)
    assert _delta(before) == (1, 1)
    want = _kernel(bijector, strided_x[:, ::2].contiguous(), strided_dy.contiguous())
    assert y.is_contiguous() and torch.equal(y.detach(), want[0]) and torch.equal(dx[:, ::2], want[1])
    assert not dx[:, 1::2].any()


# ------------------------------------------------------------------------------------------------ special values
@pytest.mark.parametrize("spec", ("sigmoid_-1_2_0.1", "softplus_1_0.01_50"))
def test_special_values_come_out_where_torch_puts_them(cusrl, spec):
    """NaN, +-Inf and +-0 in x and dy (beside ordinary values on both sides of the bounds and of torch's threshold): the NaN
    pattern and the signs of infinities and zeros are those of torch's device expression."""
    bijector = cusrl.nn.make_bijector(spec)
    nan, inf = float("nan"), float("inf")
    xs = torch.tensor([nan, inf, -inf, 0.0, -0.0, 0.3, 25.0, -7.0, 100.0, -100.0])
    ds = torch.tensor([nan, inf, -inf, 0.0, -0.0, 1.5, -2.0])
    x = xs.repeat_interleave(ds.numel()).to(DEV)
    dy = ds.repeat(xs.numel()).to(DEV)
    got, want = _kernel(bijector, x, dy), _torch(bijector, x, dy)
    for name, a, b in (("y", got[0], want[0]), ("dx", got[1], want[1])):
        assert torch.equal(torch.isnan(a), torch.isnan(b)), f"{spec} {name}: NaN pattern"
        assert torch.equal(torch.isinf(a), torch.isinf(b)), f"{spec} {name}: Inf pattern"
        assert torch.equal(a == 0, b == 0), f"{spec} {name}: zero pattern"
        special = torch.isinf(b) | (b == 0)
        assert torch.equal(torch.signbit(a)[special], torch.signbit(b)[special]), f"{spec} {name}: signs of infinities and zeros"
        ordinary = torch.isfinite(b) & (b != 0)
        assert _bijectors.relative_to_largest(a[ordinary], b[ordinary]) <= BOUND
    if _bijectors.is_softplus(spec):  # outside the bounds (a NaN x included): exactly +0.0 whatever dy holds
        outside = ~((x >= bijector.min_input) & (x <= bijector.max_input))
        assert outside.any() and not got[1][outside].any() and not torch.signbit(got[1][outside]).any()


# ------------------------------------------------------------------------------------------------ error codes
def test_error_codes(cusrl):
    """Straight through ctypes; none of the refused calls launches or writes anything."""
    from cusrl_amd import _native

    invalid = _native._CONSTANTS["E_INVALID"]
    lib = _native.lib()
    stream = torch.cuda.current_stream().cuda_stream
    x, dy = torch.ones(12, device=DEV), torch.ones(12, device=DEV)
    y, dx = torch.full((12,), 7.0, device=DEV), torch.full((12,), 7.0, device=DEV)
    X, D, Y, G = x.data_ptr(), dy.data_ptr(), y.data_ptr(), dx.data_ptr()
    before = dict(_native.launch_counts)
    good = {0: (0.05, 0.95, 0.0), 1: (2.0, -1.0, 0.5)}
    for kind, params in good.items():
        assert lib.cusrl_bijector_fwd(kind, X, Y, -1, *params, stream) == invalid
        assert lib.cusrl_bijector_bwd(kind, X, D, G, -1, *params, stream) == invalid
        assert lib.cusrl_bijector_fwd(kind, None, Y, 12, *params, stream) == invalid
        assert lib.cusrl_bijector_bwd(kind, X, None, G, 12, *params, stream) == invalid
        assert lib.cusrl_bijector_fwd(kind, X, Y, 0, *params, stream) == 0, "n == 0 succeeds without a launch"
        assert lib.cusrl_bijector_bwd(kind, X, D, G, 0, *params, stream) == 0
    for kind in (-1, 2, 99):
        assert lib.cusrl_bijector_fwd(kind, X, Y, 12, *good[1], stream) == invalid
        assert lib.cusrl_bijector_bwd(kind, X, D, G, 12, *good[1], stream) == invalid
    for params in ((0.0, -1.0, 0.5), (-2.0, -1.0, 0.5), (2.0, 0.5, -1.0)):  # scale <= 0, min_input > max_input
        assert lib.cusrl_bijector_fwd(1, X, Y, 12, *params, stream) == invalid
        assert lib.cusrl_bijector_bwd(1, X, D, G, 12, *params, stream) == invalid
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full((12,), 7.0, device=DEV)) and torch.equal(dx, torch.full((12,), 7.0, device=DEV)), "a refused call wrote"
    assert dict(_native.launch_counts) == before, "the launch counters moved"
    with pytest.raises(_native.NativeError, match=FWD):  # through the ops the refusal is an error, never a quiet fallback
        cusrl.ops.softplus_bijector(x, -2.0, -1.0, 0.5)
    assert lib.cusrl_bijector_fwd(1, X, Y, 12, *good[1], stream) == 0  # and the accepted call writes
    torch.cuda.synchronize()
    assert not (y == 7.0).any()


# ------------------------------------------------------------------------------------------------ fallbacks
@pytest.mark.parametrize("form", ["float64", "bfloat16", "autocast", "double_differentiable"])
def test_fallbacks_stay_torch_and_launch_nothing(cusrl, golden, form):
    from cusrl_amd import ops
    from cusrl_amd.nn.module import double_differentiable

    g = golden("bijectors")
    dtype = {"float64": torch.float64, "bfloat16": torch.bfloat16}.get(form, torch.float32)
    x, dy = (t.to(DEV).to(dtype) for t in _bijectors.kernel_case(g, 40, 12))

    def evaluate(function, *arguments):
        with torch.autocast("cuda", enabled=form == "autocast"):
            if form == "double_differentiable":
                with double_differentiable():
                    return function(*arguments)
            return function(*arguments)

    before = _counts()
    for spec in ("sigmoid_0.05_1.0", "softplus_2_0.05_0.8"):
        bijector = cusrl.nn.make_bijector(spec)
        leaf, leaf_ref = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        assert not evaluate(ops.bijector_supported, leaf)
        out, out_ref = evaluate(bijector, leaf), evaluate(_bijectors.torch_expression, bijector, leaf_ref)
        assert out.dtype == out_ref.dtype and torch.equal(out, out_ref)
        differentiable = form == "double_differentiable"
        (grad,) = torch.autograd.grad(out, leaf, grad_outputs=dy, create_graph=differentiable)
        (grad_ref,) = torch.autograd.grad(out_ref, leaf_ref, grad_outputs=dy, create_graph=differentiable)
        assert torch.equal(grad, grad_ref)
        if differentiable and not _bijectors.is_softplus(spec):  # a second derivative through the sigmoid bijector: torch's
            (second,) = torch.autograd.grad(grad.square().sum(), leaf)
            (second_ref,) = torch.autograd.grad(grad_ref.square().sum(), leaf_ref)
            assert torch.equal(second, second_ref) and second.abs().sum() > 0
    assert _delta(before) == (0, 0)
    if form == "double_differentiable":  # inside the context a pass nobody differentiates launches
        with double_differentiable(), torch.no_grad():
            cusrl.nn.make_bijector("sigmoid")(x)
        assert _delta(before) == (1, 0)


# ------------------------------------------------------------------------------------------------ modules
def _torch_twin(dist):
    """The same distribution with its bijector's tensor forward replaced by torch's expression."""
    twin = copy.deepcopy(dist)
    if hasattr(twin, "std_head"):
        twin.bijector = _bijectors.TorchForm(twin.bijector)
    else:
        twin.std.bijector = _bijectors.TorchForm(twin.std.bijector)
    return twin


@pytest.mark.parametrize("spec", SPECS)
@pytest.mark.parametrize("kind", ["adaptive", "vector"])
def test_distributions_on_the_device(cusrl, kind, spec):
    torch.manual_seed(17)
    B, H, A = 33, 16, 4
    dist = (cusrl.nn.AdaptiveNormalDist(H, A, bijector=spec) if kind == "adaptive" else cusrl.nn.NormalDist(H, A, bijector=spec)).to(DEV)
    if kind == "adaptive":
        # a std that depends on the state; pre-activations within about +-0.8 of the initial one, so that the std of
        # sigmoid_-1_2_0.1 (whose range includes negative values) stays positive: a log-prob needs one
        dist.std_head.weight.data.normal_(0.0, 0.05)
    else:
        dist.std.param.data.add_(torch.linspace(-0.5, 0.5, A, device=DEV))
    twin = _torch_twin(dist)
    latent = torch.randn(B, H, device=DEV)
    weight = torch.randn(B, A, device=DEV)
    results = []
    for module in (dist, twin):
        before = _counts()
        std = module(latent)["std"]
        leaves = [*module.std_head.parameters()] if kind == "adaptive" else [module.std.param]
        grads = torch.autograd.grad((std * weight).sum(), leaves)
        assert _delta(before) == ((1, 1) if module is dist else (0, 0))
        results.append((std.detach(), *grads))
    for name, got, want in zip(("std", "grad 0", "grad 1"), *results):
        error = _bijectors.relative_to_largest(got, want)
        print(f"{kind} {spec} {name}: {error:.3e} of the largest entry against the torch expression")
        assert error <= BOUND, f"{kind} {spec} {name}: {error:.3e}"
    # acting: a contiguous [B, A] std inside the range whose log-prob is compute_logp of the returned action
    bijector = dist.bijector if kind == "adaptive" else dist.std.bijector
    with torch.no_grad():
        before = _counts()
        params, (action, logp) = dist.sample(latent)
        assert _delta(before) == (1, 0)
        std = params["std"]
        assert std.shape == (B, A) and std.is_contiguous() and std.dtype == torch.float32
        if _bijectors.is_softplus(spec):
            # the clamp reaches the ends of [min, max] by construction (the default init_std 1.0 IS softplus_1_0.01_1's upper
            # end): closed interval, up to the rounding of softplus(inverse(end))
            slack = BOUND * bijector.max_value
            assert (std >= bijector.min_value - slack).all() and (std <= bijector.max_value + slack).all()
        else:
            assert (std > bijector.min_value).all() and (std < bijector.max_value).all()
        assert torch.equal(std, results[0][0]) if kind == "adaptive" else torch.equal(std[0], results[0][0][0])
        assert (std > 0).all(), "the case keeps the std positive"
        error = _bijectors.relative_to_largest(logp, dist.compute_logp(params, action))
        assert error <= BOUND, f"{kind} {spec}: log-prob off by {error:.3e}"


# ------------------------------------------------------------------------------------------------ end to end
def test_captured_ppo_agent_with_a_sigmoid_bounded_std(cusrl):
    """The ``ppo`` preset with ``NormalDist.Factory(bijector="sigmoid_0.05_1.0")`` and the captured minibatch step: three
    updates; finite losses, a std strictly inside its bounds, bijector launches counted, and a third update that replays the
    graphs of the second."""

    class Watch(cusrl.Hook):
        def __init__(self):
            super().__init__()
            self.records = []

        def post_update(self):
            agent = self.agent
            graphs = {key: id(step.forward_backward.graph) for key, step in agent._graphed_steps.items() if step.state == 2}
            self.records.append((graphs, agent.actor.distribution.std_vector().clone(), _counts()))

    cusrl.set_global_seed(23)
    env = cusrl.testing.DummyTorchEnvironment(num_instances=64, observation_dim=12, action_dim=4, device=DEV)
    factory = cusrl.preset.PpoAgentFactory(num_steps_per_update=8, sampler_epochs=2, sampler_mini_batches=2, compile=True).to_underlying()
    factory.actor_factory.distribution_factory = cusrl.nn.NormalDist.Factory(bijector="sigmoid_0.05_1.0")
    watch = Watch()
    factory.register_hook(watch)
    start = _counts()
    trainer = cusrl.Trainer(env, factory, num_iterations=3, verbose=False)
    agent = trainer.agent
    assert isinstance(agent.actor.distribution.std.bijector, cusrl.nn.SigmoidBijector)
    initial = agent.actor.distribution.std.param.detach().clone()
    trainer.run_training_loop()
    torch.cuda.synchronize()
    assert len(watch.records) == 3
    for key in ("Agent/value_loss", "Agent/surrogate_loss", "Agent/entropy_loss"):
        assert np.isfinite(trainer.last_info[key]), key
    for graphs, std, _ in watch.records:
        assert torch.isfinite(std).all() and (std > 0.05).all() and (std < 1.0).all(), std
    assert not torch.equal(agent.actor.distribution.std.param.detach(), initial), "the std parameter did not train"
    forward, backward = (now - then for now, then in zip(watch.records[1][2], start))
    print(f"bijector launches issued from Python over two updates: forward {forward}, backward {backward}")
    assert forward > 0 and backward > 0
    assert watch.records[1][0] and len(watch.records[1][0]) == 2, "both minibatch steps are captured after the second update"
    assert watch.records[2][0] == watch.records[1][0], "the third update captured again"
