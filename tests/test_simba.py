"""Simba without a GPU: the module tree, state-dict keys, output and gradients against the reference's recorded run (golden
``simba.npz``), the dims rules and the factory, and the float64 restatement the GPU tests measure the kernels with."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import _simba

BATCHES = (3, 257)
CASES = [(c, batch) for c in range(4) for batch in BATCHES]
BOUND = 1e-5  # the standing bound: outputs relative, gradients in oracle.gradient_error units


@pytest.fixture(scope="module")
def cusrl():
    import cusrl_amd

    return cusrl_amd


def test_simba_is_exported(cusrl):
    from cusrl_amd.nn.simba import Simba, SimbaBlock, SimbaFactory

    for namespace in (cusrl, cusrl.nn):
        assert namespace.Simba is Simba and namespace.SimbaBlock is SimbaBlock and namespace.SimbaFactory is SimbaFactory
        assert {"Simba", "SimbaBlock", "SimbaFactory"} <= set(namespace.__all__)
    assert Simba.Factory is SimbaFactory


def test_golden_holds_the_cases_of_record(golden):
    g = golden("simba")
    assert _simba.configs(g) == [(7, 64, 2, 5, "ReLU"), (48, 100, 1, None, "ReLU"), (12, None, 2, 3, "Tanh"), (9, 260, 0, 4, "ReLU")]
    assert tuple(int(b) for b in g["batches"]) == BATCHES
    assert [int(r) for r in g["kernel_rows"]] == [1, 3, 257, 2049]
    assert [int(h) for h in g["kernel_widths"]] == [5, 63, 64, 100, 256, 260, 1024]
    for c, batch in CASES:  # the reference's own fp32 distance from float64 leaves half the bound and more
        assert g[f"m{c}_{batch}_reference_distance"].max() <= BOUND / 2


@pytest.mark.parametrize("c", range(4))
def test_state_dict_keys_and_strict_load(cusrl, golden, c):
    g = golden("simba")
    input_dim, hidden_dim, num_blocks, output_dim, activation = _simba.configs(g)[c]
    module = cusrl.nn.Simba(input_dim, hidden_dim, num_blocks, output_dim, activation)
    assert list(module.state_dict()) == [str(k) for k in g[f"m{c}_state_keys"]]
    assert [name for name, _ in module.named_parameters()] == [str(k) for k in g[f"m{c}_param_names"]]
    state = _simba.golden_state(g, c)
    assert module.load_state_dict(state, strict=True).missing_keys == []
    for key, value in module.state_dict().items():
        assert torch.equal(value, state[key]), key


@pytest.mark.parametrize("c", range(4))
def test_module_tree_is_the_references(cusrl, golden, c):
    from cusrl_amd.nn.module import Linear
    from cusrl_amd.nn.simba import SimbaBlock

    input_dim, hidden_dim, num_blocks, output_dim, activation = _simba.configs(golden("simba"))[c]
    module = cusrl.nn.Simba(input_dim, hidden_dim, num_blocks, output_dim, activation)
    width = hidden_dim or input_dim
    layers = list(module.blocks)
    expected = ([Linear] if hidden_dim is not None else []) + [SimbaBlock] * num_blocks + [torch.nn.LayerNorm]
    expected += [Linear] if output_dim is not None else []
    assert [type(layer) for layer in layers] == expected
    for block in (layer for layer in layers if type(layer) is SimbaBlock):
        assert [type(m) for m in block] == [torch.nn.LayerNorm, Linear, getattr(torch.nn, activation), Linear]
        assert block[1].weight.shape == (4 * width, width) and block[3].weight.shape == (width, 4 * width)
    # ModuleInitialization walks nn.Linear instances: the project's Linear is one
    linears = [m for m in module.modules() if isinstance(m, torch.nn.Linear)]
    assert len(linears) == 2 * num_blocks + (hidden_dim is not None) + (output_dim is not None)
    assert (module.input_dim, module.output_dim, module.hidden_dim, module.num_blocks) == (input_dim, output_dim or width, width, num_blocks)
    assert not module.is_recurrent


@pytest.mark.parametrize("c,batch", CASES)
def test_cpu_output_and_gradients_reproduce_the_reference(cusrl, golden, gradient_parity, c, batch):
    g = golden("simba")
    module = _simba.golden_module(cusrl, g, c)
    output, grad_input, grads = _simba.run_case(module, g, c, batch)
    expected = g[f"m{c}_{batch}_output"]
    error = np.abs(output.detach().numpy().astype(np.float64) - expected).max() / np.abs(expected).max()
    print(f"simba case {c} B={batch}: output error {error:.3e} of the largest entry")
    assert error <= BOUND
    gradient_parity(f"simba_cpu_input[{c}-{batch}]", grad_input.numpy(), g[f"m{c}_{batch}_grad_input"], BOUND)
    assert set(grads) == {str(k) for k in g[f"m{c}_param_names"]}
    for name, grad in grads.items():
        gradient_parity(f"simba_cpu_param[{c}-{batch}-{name}]", *_simba.recorded_gradient(g, c, batch, name, grad), BOUND)


def test_dims_rules(cusrl):
    plain = cusrl.nn.Simba(12)
    assert (plain.input_dim, plain.hidden_dim, plain.output_dim, plain.num_blocks) == (12, 12, 12, 1)
    assert [type(m).__name__ for m in plain.blocks] == ["SimbaBlock", "LayerNorm"]
    projected = cusrl.nn.Simba(12, hidden_dim=32, num_blocks=0, output_dim=5)
    assert (projected.hidden_dim, projected.output_dim) == (32, 5)
    assert [type(m).__name__ for m in projected.blocks] == ["Linear", "LayerNorm", "Linear"]
    assert projected(torch.zeros(2, 12)).shape == (2, 5)
    assert plain(torch.zeros(4, 3, 12)).shape == (4, 3, 12)  # leading dimensions pass through
    with pytest.raises(ValueError):
        cusrl.nn.Simba(0)


def test_factory(cusrl):
    factory = cusrl.nn.Simba.Factory(hidden_dim=16, num_blocks=3, activation_fn="Tanh")
    module = factory(6, 4)
    assert isinstance(module, cusrl.nn.Simba) and (module.input_dim, module.hidden_dim, module.num_blocks, module.output_dim) == (6, 16, 3, 4)
    assert all(type(block[2]) is torch.nn.Tanh for block in module.blocks if isinstance(block, cusrl.nn.SimbaBlock))
    assert factory(6).output_dim == 16  # no output projection: the width
    assert cusrl.nn.Simba.Factory()(9).hidden_dim == 9
    with pytest.raises(AssertionError):
        factory()
    # the factories of Actor and Value take it like any backbone factory
    actor = cusrl.Actor.Factory(factory, cusrl.NormalDist.Factory())(6, 2)
    critic = cusrl.Value.Factory(factory)(6, 1)
    assert isinstance(actor.backbone, cusrl.nn.Simba) and isinstance(critic.backbone, cusrl.nn.Simba)
    assert actor.backbone.output_dim == 16 and critic(torch.zeros(3, 6))[0].shape == (3, 1)


def test_unknown_activation_raises(cusrl):
    with pytest.raises(ValueError, match="Unknown activation"):
        cusrl.nn.Simba(4, activation_fn="NoSuchActivation")
    assert type(cusrl.nn.Simba(4, activation_fn=torch.nn.GELU).blocks[0][2]) is torch.nn.GELU


def test_block_adds_its_input_back(cusrl):
    torch.manual_seed(0)
    block = cusrl.nn.SimbaBlock(8, "ReLU")
    x = torch.randn(5, 8)
    assert torch.equal(block(x), x + block[3](block[2](block[1](block[0](x)))))
    assert torch.equal(block.branch(block[0](x)), block[3](block[2](block[1](block[0](x)))))


def test_cpu_tensors_take_torchs_expression(cusrl):
    """The predicate declines a CPU tensor; ``ops.add_layer_norm`` is then torch's ``x + r`` and ``F.layer_norm``, bit for bit."""
    from cusrl_amd import _native, ops

    torch.manual_seed(1)
    x, r, gamma, beta = torch.randn(6, 10), torch.randn(6, 10), torch.randn(10), torch.randn(10)
    assert not ops.add_layer_norm_supported(x, r, gamma, beta)
    before = dict(_native.launch_counts)
    s, y = ops.add_layer_norm(x, r, gamma, beta, 1e-5)
    assert torch.equal(s, x + r) and torch.equal(y, torch.nn.functional.layer_norm(x + r, (10,), gamma, beta, 1e-5))
    s, y = ops.add_layer_norm(x, None, gamma, beta, 1e-5)
    assert s is x and torch.equal(y, torch.nn.functional.layer_norm(x, (10,), gamma, beta, 1e-5))
    assert _native.launch_counts == before
    assert _native.MAX_LAYER_NORM_WIDTH == 1024
    assert {"cusrl_add_layer_norm_fwd", "cusrl_add_layer_norm_bwd", "cusrl_add_layer_norm_num_partials"} <= set(_native.EXPORTED_SYMBOLS)


@pytest.mark.parametrize("B,H", [(3, 5), (257, 64), (3, 1)])
@pytest.mark.parametrize("residual", [False, True])
def test_restatement_agrees_with_torch_in_float64(golden, B, H, residual):
    """The yardstick of the GPU tests against torch's own float64 LayerNorm and autograd."""
    g = golden("simba")
    case = _simba.kernel_case(g, B, max(H, 5))
    case = {k: v[..., :H] for k, v in case.items()}
    assert abs(float(_simba.kernel_case(g, 2049, 1024)["x"].mean()) - 1.5) < 0.05
    s, y, xhat, rstd = _simba.add_layer_norm64(case["x"], case["r"] if residual else None, case["gamma"], case["beta"], 1e-5)
    d_s, d_gamma, d_beta = _simba.add_layer_norm_bwd64(case["dy"], case["ds"], xhat, rstd, case["gamma"])
    s_t = torch.from_numpy(s).requires_grad_(True)
    gamma_t, beta_t = (torch.from_numpy(case[k]).double().requires_grad_(True) for k in ("gamma", "beta"))
    y_t = torch.nn.functional.layer_norm(s_t, (H,), gamma_t, beta_t, 1e-5)
    loss = (y_t * torch.from_numpy(case["dy"]).double()).sum() + (s_t * torch.from_numpy(case["ds"]).double()).sum()
    grads = torch.autograd.grad(loss, [s_t, gamma_t, beta_t])
    np.testing.assert_allclose(y, y_t.detach().numpy(), rtol=1e-9, atol=1e-9)
    for mine, theirs in zip((d_s, d_gamma, d_beta), grads):
        np.testing.assert_allclose(mine, theirs.numpy(), rtol=1e-8, atol=1e-8 * max(1.0, float(theirs.abs().max())))
