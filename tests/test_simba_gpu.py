"""Residual add + LayerNorm and the Simba backbone on an MI355X: the two launches against torch's fp32 ``x + r`` (bit for bit)
and the float64 restatement (tests/_simba.py), offset views, fallbacks, ``Simba`` against the reference's recorded run (golden
``simba.npz``), its launch counts and autograd graph, and an agent with Simba backbones with and without compile=True."""

from __future__ import annotations

import itertools

import numpy as np
import pytest
import torch

import _simba

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
BOUND = 1e-5  # the standing bound: outputs relative to the largest entry, gradients in oracle.gradient_error units
ROWS = (1, 3, 257, 2049)  # one wave, one block, several blocks with a ragged last one, several rows per wave
WIDTHS = (5, 63, 64, 100, 256, 260, 1024)  # below / at a wave's 64 chunks, H % 4 != 0, 1 .. 4 chunks per lane
# beyond the issue's grid: enough rows to reach the backward's block cap (256 blocks of 8 waves, 4 rows each)
SHAPES = [*itertools.product(ROWS, WIDTHS), (8200, 5)]
FWD, BWD = "cusrl_add_layer_norm_fwd", "cusrl_add_layer_norm_bwd"


@pytest.fixture(scope="module")
def cusrl():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    import cusrl_amd

    cusrl_amd.config.set_device(DEV)
    return cusrl_amd


def _count(name):
    from cusrl_amd import _native

    return _native.launch_counts.get(name, 0)


def _device(case, *names, grad=()):
    return [torch.from_numpy(np.ascontiguousarray(case[n])).to(DEV).requires_grad_(n in grad) for n in names]


def _run(x, r, gamma, beta, dy, ds):
    """One forward and one backward through the autograd Function: (s, y, d_x, d_r | None, d_gamma, d_beta)."""
    from cusrl_amd import ops

    s, y = ops.AddLayerNorm.apply(x, r, gamma, beta, EPS)
    inputs = [x, gamma, beta] + ([r] if r is not None else [])
    outputs, grad_outputs = ([y, s], [dy, ds]) if ds is not None else ([y], [dy])
    grads = torch.autograd.grad(outputs, inputs, grad_outputs=grad_outputs)
    return s.detach(), y.detach(), grads[0], (grads[3] if r is not None else None), grads[1], grads[2]


def _relative_to_largest(candidate, reference) -> float:
    return float(np.abs(candidate.cpu().numpy().astype(np.float64) - reference).max() / np.abs(reference).max())


@pytest.mark.parametrize("B,H", SHAPES)
def test_kernels_against_the_float64_restatement(cusrl, golden, gradient_parity, B, H):
    case = _simba.kernel_case(golden("simba"), B, H)
    for with_residual, with_ds in itertools.product((False, True), repeat=2):
        x, r, gamma, beta = _device(case, "x", "r", "gamma", "beta", grad=("x", "r", "gamma", "beta"))
        dy, ds = _device(case, "dy", "ds")
        r, ds = (r if with_residual else None), (ds if with_ds else None)
        before = _count(FWD), _count(BWD)
        s, y, d_x, d_r, d_gamma, d_beta = _run(x, r, gamma, beta, dy, ds)
        assert (_count(FWD), _count(BWD)) == (before[0] + 1, before[1] + 1), "one forward and one backward call"
        tag = f"{B}x{H}-{'r' if with_residual else 'plain'}-{'ds' if with_ds else 'nods'}"

        assert torch.equal(s, x.detach() + r.detach() if with_residual else x.detach()), f"{tag}: sum_out is not torch's x + r"
        s64, y64, xhat, rstd = _simba.add_layer_norm64(case["x"], case["r"] if with_residual else None, case["gamma"], case["beta"], EPS)
        d_s64, d_gamma64, d_beta64 = _simba.add_layer_norm_bwd64(case["dy"], case["ds"] if with_ds else None, xhat, rstd, case["gamma"])
        error = _relative_to_largest(y, y64)
        print(f"{tag}: y error {error:.3e} of the largest entry")
        assert error <= BOUND, f"{tag}: y is {error:.3e} of the largest entry away from float64"
        gradient_parity(f"add_layer_norm_d_s[{tag}]", d_x.cpu().numpy(), d_s64, BOUND)
        gradient_parity(f"add_layer_norm_d_gamma[{tag}]", d_gamma.cpu().numpy(), d_gamma64, BOUND)
        gradient_parity(f"add_layer_norm_d_beta[{tag}]", d_beta.cpu().numpy(), d_beta64, BOUND)
        if with_residual:
            assert torch.equal(d_r, d_x), f"{tag}: x and residual share one gradient"

        again = _run(x, r, gamma, beta, dy, ds)  # no atomics, fixed order: the same bits
        for name, first, second in zip(("s", "y", "d_x", "d_r", "d_gamma", "d_beta"), (s, y, d_x, d_r, d_gamma, d_beta), again):
            assert (first is None and second is None) or torch.equal(first, second), f"{tag}: {name} differs between two runs"


def test_width_one(cusrl):
    """H = 1: the row is its own mean, so y = beta, d_s = ds and d_gamma = 0 exactly; d_beta = the column sum of dy.  (No parity
    bound: the true gradients are zero.)"""
    gen = torch.Generator().manual_seed(3)
    x, r, dy, ds = (torch.randn(3, 1, generator=gen).to(DEV) for _ in range(4))
    gamma, beta = (torch.randn(1, generator=gen).to(DEV).requires_grad_(True) for _ in range(2))
    for residual in (None, r):
        xg = x.clone().requires_grad_(True)
        s, y, d_x, _, d_gamma, d_beta = _run(xg, None if residual is None else residual.clone().requires_grad_(True), gamma, beta, dy, ds)
        assert torch.equal(y, beta.detach().expand(3, 1))
        assert torch.equal(d_x, ds)
        assert torch.equal(d_gamma, torch.zeros_like(d_gamma))
        assert torch.equal(d_beta, dy.double().sum(0).float())
    s, y, d_x, _, d_gamma, _ = _run(x.clone().requires_grad_(True), None, gamma, beta, dy, None)
    assert torch.equal(d_x, torch.zeros_like(d_x)) and torch.equal(d_gamma, torch.zeros_like(d_gamma))


def _offset_view(t):
    """The same values one float off a 16-byte boundary."""
    buffer = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buffer[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("B,H", [(3, 260), (257, 64)])
@pytest.mark.parametrize("shifted", ["x", "r", "dy"])
def test_offset_views_give_the_bits_of_the_aligned_call(cusrl, golden, B, H, shifted):
    case = _simba.kernel_case(golden("simba"), B, H)
    x, r, gamma, beta = _device(case, "x", "r", "gamma", "beta")
    dy, ds = _device(case, "dy", "ds")
    assert all(t.data_ptr() % 16 == 0 for t in (x, r, dy, ds))
    leaves = lambda *ts: [t.detach().requires_grad_(True) for t in ts]  # noqa: E731
    aligned = _run(*leaves(x, r, gamma, beta), dy, ds)
    moved = {"x": x, "r": r, "dy": dy}
    moved[shifted] = _offset_view(moved[shifted])
    x2, r2 = (t.requires_grad_(True) for t in (moved["x"], moved["r"]))
    offset = _run(x2, r2, *leaves(gamma, beta), moved["dy"], ds)
    for name, first, second in zip(("s", "y", "d_x", "d_r", "d_gamma", "d_beta"), aligned, offset):
        assert torch.equal(first, second), f"{name} differs when {shifted} is an offset view"


def _torch_expression(x, r, gamma, beta):
    s = x + r
    return s, torch.nn.functional.layer_norm(s, s.shape[-1:], gamma, beta, EPS)


@pytest.mark.parametrize("form", ["wide", "float64", "transposed", "autocast"])
def test_fallbacks_leave_the_kernels_alone(cusrl, form):
    from cusrl_amd import ops

    gen = torch.Generator().manual_seed(5)
    H = 1025 if form == "wide" else 48
    x, r = (torch.randn(40, H, generator=gen).to(DEV) for _ in range(2))
    gamma, beta = (torch.randn(H, generator=gen).to(DEV) for _ in range(2))
    if form == "float64":
        x, r, gamma, beta = (t.double() for t in (x, r, gamma, beta))
    if form == "transposed":
        x = torch.randn(H, 40, generator=gen).to(DEV).t()
        assert not x.is_contiguous()
    before = _count(FWD), _count(BWD)
    for t in (x, gamma):
        t.requires_grad_(True)
    with torch.autocast("cuda", enabled=form == "autocast"):
        assert not ops.add_layer_norm_supported(x, r, gamma, beta)
        s, y = ops.add_layer_norm(x, r, gamma, beta, EPS)
        s_ref, y_ref = _torch_expression(x, r, gamma, beta)
    assert s.dtype == s_ref.dtype and y.dtype == y_ref.dtype
    assert torch.equal(s, s_ref) and torch.equal(y, y_ref)
    grads = torch.autograd.grad(y.float().sum(), [x, gamma])
    grads_ref = torch.autograd.grad(y_ref.float().sum(), [x, gamma])
    assert all(torch.equal(a, b) for a, b in zip(grads, grads_ref))
    assert (_count(FWD), _count(BWD)) == before
    if form == "autocast":  # ... and the module as a whole declines under autocast
        module = cusrl.nn.Simba(12, 48, 1).to(DEV)
        with torch.autocast("cuda"):
            module(torch.randn(8, 12, device=DEV))
        assert (_count(FWD), _count(BWD)) == before


def test_double_differentiable_forward_takes_torchs_ops(cusrl):
    from cusrl_amd.nn.module import double_differentiable

    module = cusrl.nn.Simba(6, 16, 1).to(DEV)
    observation = torch.randn(8, 6, device=DEV, requires_grad=True)
    before = _count(FWD), _count(BWD)
    with double_differentiable():
        output = module(observation)
        (grad,) = torch.autograd.grad(output.sum(), observation, create_graph=True)
    grad.square().sum().backward()  # a second differentiation: torch's own LayerNorm backward is differentiable
    assert (_count(FWD), _count(BWD)) == before and observation.grad is not None
    with torch.no_grad():
        module(observation)
    assert _count(FWD) == before[0] + 2  # outside the context the same module launches (num_blocks + 1)


# ------------------------------------------------------------------------------------------------ the module
def _graph_nodes(output):
    seen, stack = set(), [output.grad_fn]
    while stack:
        node = stack.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        stack.extend(fn for fn, _ in node.next_functions)
    return [type(node).__name__ for node in seen]


@pytest.mark.parametrize("c,batch", [(c, batch) for c in range(4) for batch in (3, 257)])
def test_module_reproduces_the_reference(cusrl, golden, gradient_parity, c, batch):
    g = golden("simba")
    module = _simba.golden_module(cusrl, g, c, DEV)
    num_blocks = _simba.configs(g)[c][2]
    before = _count(FWD), _count(BWD)
    output, grad_input, grads = _simba.run_case(module, g, c, batch, DEV)
    assert (_count(FWD), _count(BWD)) == (before[0] + num_blocks + 1, before[1] + num_blocks + 1)
    nodes = _graph_nodes(output)
    assert sum(name.startswith("AddLayerNorm") for name in nodes) == num_blocks + 1
    assert not [name for name in nodes if name.startswith(("AddBackward", "NativeLayerNorm"))], nodes

    error = _relative_to_largest(output.detach(), g[f"m{c}_{batch}_output"].astype(np.float64))
    print(f"simba case {c} B={batch}: output error {error:.3e} of the largest entry")
    assert error <= BOUND
    gradient_parity(f"simba_gpu_input[{c}-{batch}]", grad_input.cpu().numpy(), g[f"m{c}_{batch}_grad_input"], BOUND)
    for name, grad in grads.items():
        gradient_parity(f"simba_gpu_param[{c}-{batch}-{name}]", *_simba.recorded_gradient(g, c, batch, name, grad), BOUND)

    with torch.no_grad():  # the no-grad pass: the same launches, no statistics saved, the same output bits
        before = _count(FWD), _count(BWD)
        observation = torch.from_numpy(g[f"m{c}_{batch}_input"].astype(np.float32)).to(DEV)
        assert torch.equal(module(observation), output)
        assert (_count(FWD), _count(BWD)) == (before[0] + num_blocks + 1, before[1])


# ------------------------------------------------------------------------------------------------ the agent
def _train(cusrl, compile, iterations=2):
    cusrl.set_global_seed(7)
    env = cusrl.testing.DummyTorchEnvironment(num_instances=64, observation_dim=12, action_dim=4, device=DEV)
    factory = cusrl.preset.PpoAgentFactory(num_steps_per_update=8, sampler_epochs=2, sampler_mini_batches=2, compile=compile,
                                           optimizer_kwargs={"capturable": True, "fused": True}).to_underlying()
    backbone = cusrl.nn.Simba.Factory(hidden_dim=64, num_blocks=2)
    factory.actor_factory.backbone_factory = backbone
    factory.critic_factory.backbone_factory = backbone
    trainer = cusrl.Trainer(env, factory, num_iterations=iterations, verbose=False)
    initial = {name: param.detach().clone() for name, param in trainer.agent.named_parameters()}
    before = _count(FWD), _count(BWD)
    trainer.run_training_loop()
    torch.cuda.synchronize()
    return trainer, initial, (_count(FWD) - before[0], _count(BWD) - before[1])


@pytest.fixture(scope="module")
def trained(cusrl):
    return {key: _train(cusrl, compile) for key, compile in (("eager", False), ("captured", True))}


def test_agent_with_simba_backbones_trains(cusrl, trained):
    trainer, initial, (forward, backward) = trained["eager"]
    agent = trainer.agent
    assert isinstance(agent.actor.backbone, cusrl.nn.Simba) and isinstance(agent.critic.backbone, cusrl.nn.Simba)
    assert forward > 0 and backward == 2 * 2 * 2 * 2 * 3  # iterations x epochs x minibatches x networks x (num_blocks + 1)
    changed = 0
    for name, param in agent.named_parameters():
        assert torch.isfinite(param).all(), name
        changed += int(not torch.equal(param, initial[name]))
    assert changed == len(initial), "every parameter takes part in the update"


def test_training_under_capture_is_bit_identical_to_eager(cusrl, trained):
    """Both minibatch steps replay from their graphs and the parameters are the ``compile=False`` run's bit for bit.  (What this
    pinned down: the replayed value bootstrap evaluates its few truncated rows inside a padded bucket of 256; Simba's no-grad pass
    runs library GEMMs whose summation order depends on the row count — 3 rows alone and inside 256 differ by 9.5e-7 — so a
    Simba critic bootstraps exactly its rows, ``Module.batch_invariant``.)"""
    eager, captured = trained["eager"][0].agent, trained["captured"][0].agent
    # the captured minibatch step admits the module as it is: the steps ran from their graphs (the signal the existing capture
    # tests read), not from an eager fall-back
    assert captured._graphed_steps, "compile=True did not capture the minibatch step"
    print("captured steps:", {key: step.state for key, step in captured._graphed_steps.items()})
    differ = [name for (name, p), (_, q) in zip(eager.named_parameters(), captured.named_parameters()) if not torch.equal(p, q)]
    print(f"{len(differ)} of {len(list(eager.parameters()))} parameters differ in bits between compile=False and compile=True")
    for (name, p), (_, q) in zip(eager.named_parameters(), captured.named_parameters()):
        assert torch.isfinite(q).all(), name
        assert torch.equal(p, q), name
