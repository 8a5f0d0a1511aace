"""``NormalNllLoss`` and ``L2RegularizationLoss`` on the device against the reference's recorded losses and autograd gradients
(golden ``loss_layers.npz``): every case through the public layers, both input forms; the chunked form's single gradient
tensor; a rescaled loss; what stays torch's expression; a captured replay.  Bounds: 1e-5 relative for a loss, 1e-5 of the
largest entry for a gradient — the project's standing ones."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from _loss_layers import EPS, FORMS, GOLDEN, REDUCED, UNREDUCED, case_inputs, check_loss, expected, parse, run_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KERNEL = "cusrl_normal_nll_fwd_bwd"


@pytest.fixture(scope="module")
def cusrl():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    import cusrl_amd

    cusrl_amd.config.set_device(DEV)
    return cusrl_amd


def host(t):
    return t.detach().cpu().numpy()


def _count(name=KERNEL):
    from cusrl_amd import _native

    return _native.launch_counts.get(name, 0)


def _check(case, label, loss, grads, gradient_parity, scale=1.0):
    reference = expected(case, "loss")
    print(f"{label}: loss {loss.item():.9g} vs {float(reference):.9g} (rel {abs(loss.item() - reference) / abs(reference):.2e})")
    np.testing.assert_allclose(loss.item(), reference, rtol=1e-5)
    for name, gradient in grads.items():
        achieved = gradient_parity(f"loss_layers.{name}[{label}]", host(gradient), scale * expected(case, name), 1e-5)
        print(f"{label}: {name} {achieved:.2e} of the largest entry")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", REDUCED)
def test_normal_nll_on_the_device_reproduces_the_reference(cusrl, case, form, gradient_parity):
    before = _count()
    loss, grads = run_case(cusrl, case, form, device=DEV)
    assert _count() == before + 1  # the HIP form: one call for the loss and both gradients
    assert loss.shape == () and loss.is_cuda
    _check(case, f"{case},{form}", loss, grads, gradient_parity)


def test_misaligned_operands_take_the_scalar_path(cusrl, gradient_parity):
    """6x4 is a float4 shape; the same values from views one float off a 16-byte boundary."""
    from cusrl_amd import ops

    case = next(c for c in REDUCED if c.startswith("6x4|"))
    _, mode, full, reduction = parse(case)
    mean, dist, target = case_inputs(case, DEV)

    def shifted(t):
        moved = torch.empty(t.numel() + 1, device=DEV)[1:].view(t.shape).copy_(t)
        assert moved.data_ptr() % 16 == 4 and moved.is_contiguous()
        return moved

    aligned = ops.normal_nll_fwd_bwd(mean, dist, target, mode, full, EPS, reduction)
    for which in range(3):
        operands = [shifted(t) if i == which else t for i, t in enumerate((mean, dist, target))]
        loss, d_mean, d_dist = ops.normal_nll_fwd_bwd(*operands, mode, full, EPS, reduction)
        _check(case, f"{case},shifted{which}", loss, {"d_mean": d_mean, "d_dist": d_dist}, gradient_parity)
        # (the same fp32 arithmetic per element on either path; the block's sum is taken in another order)
        assert torch.equal(d_mean, aligned[1]) and torch.equal(d_dist, aligned[2])


def test_the_chunked_gradient_is_one_tensor(cusrl):
    from cusrl_amd import ops

    case = next(c for c in REDUCED if c.startswith("37x7|"))
    _, mode, full, reduction = parse(case)
    mean, dist, target = case_inputs(case, DEV)
    joint = torch.cat([mean, dist], dim=-1).requires_grad_()
    loss = cusrl.nn.NormalNllLoss(mode=mode, full=full, eps=EPS, reduction=reduction)(joint, target)
    # the loss hangs directly on the input: no split / cat / zero-fill node between them
    assert type(loss.grad_fn).__name__ == "_NormalNllFunctionBackward"
    edges = [fn for fn, _ in loss.grad_fn.next_functions if fn is not None]
    assert len(edges) == 1 and type(edges[0]).__name__ == "AccumulateGrad" and edges[0].variable is joint
    loss.backward()
    assert joint.grad.shape == joint.shape
    # and the binding's two gradients are the halves of one [..., 2K] tensor
    _, d_mean, d_dist = ops.normal_nll_fwd_bwd(joint.detach(), None, target, mode, full, EPS, reduction)
    K = mean.shape[-1]
    assert d_mean._base is d_dist._base and d_mean._base.shape == joint.shape and d_mean._base.is_contiguous()
    assert d_mean.untyped_storage().data_ptr() == d_dist.untyped_storage().data_ptr()
    assert d_dist.data_ptr() == d_mean.data_ptr() + 4 * K and d_mean.stride() == d_dist.stride() == (2 * K, 1)
    assert torch.equal(d_mean._base, joint.grad)


@pytest.mark.parametrize("form", FORMS)
def test_a_rescaled_loss_scales_both_gradients(cusrl, form, gradient_parity):
    case = next(c for c in REDUCED if c.startswith("37x7|std|"))
    loss, grads = run_case(cusrl, case, form, device=DEV, scale=2.5)
    _check(case, f"{case},{form},x2.5", loss, grads, gradient_parity, scale=2.5)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", UNREDUCED)
def test_no_reduction_keeps_torchs_expression(cusrl, case, form, gradient_parity):
    before = _count()
    loss, grads = run_case(cusrl, case, form, device=DEV)
    assert _count() == before
    check_loss(loss, expected(case, "loss"), gradient_parity, f"loss_layers.unreduced.loss[{case},{form}]")
    for name, gradient in grads.items():
        gradient_parity(f"loss_layers.unreduced.{name}[{case},{form}]", host(gradient), expected(case, name), 1e-5)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", [c for c in REDUCED if c.startswith("37x7|") and "|0|mean" in c])
def test_a_target_that_needs_a_gradient_keeps_torchs_expression(cusrl, case, form, gradient_parity):
    before = _count()
    loss, grads = run_case(cusrl, case, form, device=DEV, target_grad=True)
    assert _count() == before and set(grads) == {"d_mean", "d_dist", "d_target"}
    _check(case, f"{case},{form},target", loss, grads, gradient_parity)


def test_other_dtypes_keep_torchs_expression(cusrl):
    case = next(c for c in REDUCED if c.startswith("5x12|"))
    _, mode, full, reduction = parse(case)
    mean, dist, target = (t.double() for t in case_inputs(case, DEV))
    before = _count()
    loss = cusrl.nn.NormalNllLoss(mode=mode, full=full, eps=EPS, reduction=reduction)((mean, dist), target)
    assert _count() == before and loss.dtype == torch.float64
    np.testing.assert_allclose(loss.item(), expected(case, "loss"), rtol=1e-5)


def test_captured_replays_equal_eager_bit_for_bit(cusrl):
    """The 37x7 chunked form (scalar path, misaligned ``dist``) on one stream in a graph, replayed with the inputs refilled in
    place; nothing in the graph is a memset."""
    from cusrl_amd import ops

    cases = [c for c in REDUCED if c.startswith("37x7|") and c.endswith("|1|mean")][:3]
    fills = []
    for case in cases:  # three sets of values of one shape (whatever their variance parameter was drawn as)
        mean, dist, target = case_inputs(case, DEV)
        fills.append((torch.cat([mean, dist], dim=-1), target))
    arguments = ("log_var", True, EPS, "mean")
    eager = [ops.normal_nll_fwd_bwd(joint, None, target, *arguments) for joint, target in fills]
    joint, target = fills[0][0].clone(), fills[0][1].clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.normal_nll_fwd_bwd(joint, None, target, *arguments)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, stream=stream):
        loss, d_mean, d_dist = ops.normal_nll_fwd_bwd(joint, None, target, *arguments)
    census = ops.graph_census(graph)
    assert census["memset"] == 0 and census["kernel"] == 1, census  # one self-finalising block, nothing to zero
    graph.instantiate()
    for (new_joint, new_target), (eager_loss, eager_d_mean, eager_d_dist) in zip(fills[::-1], eager[::-1]):
        joint.copy_(new_joint)
        target.copy_(new_target)
        loss.fill_(float("nan"))
        d_mean._base.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss, eager_loss) and torch.equal(d_mean, eager_d_mean) and torch.equal(d_dist, eager_d_dist)


@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
def test_l2_regularization_on_the_device(cusrl, reduction, gradient_parity):
    x = torch.from_numpy(GOLDEN["l2_input"]).to(DEV).requires_grad_()
    before = _count("cusrl_sumsq_fwd_bwd")
    loss = cusrl.nn.L2RegularizationLoss(reduction=reduction)(x)
    assert _count("cusrl_sumsq_fwd_bwd") == before + (reduction != "none")
    (2.5 * loss).backward(torch.ones_like(loss))
    check_loss(loss, GOLDEN[f"l2_{reduction}_loss"], gradient_parity, "loss_layers.l2_unreduced")
    gradient_parity(f"loss_layers.l2[{reduction}]", host(x.grad), 2.5 * GOLDEN[f"l2_{reduction}_d_input"], 1e-5)


def test_the_binding_refuses_what_it_cannot_take(cusrl):
    from cusrl_amd import ops

    mean, dist, target = (torch.randn(6, 4, device=DEV) for _ in range(3))
    before = _count()
    with pytest.raises(ValueError, match="even last dimension"):
        ops.normal_nll_fwd_bwd(torch.randn(6, 5, device=DEV), None, target, "log_var", False, 1e-6, "mean")
    with pytest.raises(ValueError, match="differ in shape"):
        ops.normal_nll_fwd_bwd(mean, dist[:5], target, "log_var", False, 1e-6, "mean")
    with pytest.raises(ValueError, match="differ in shape or are empty"):
        ops.normal_nll_fwd_bwd(mean, dist, target[:, :3], "log_var", False, 1e-6, "mean")
    with pytest.raises(ValueError, match="differ in shape or are empty"):
        ops.normal_nll_fwd_bwd(mean[:0], dist[:0], target[:0], "log_var", False, 1e-6, "mean")
    with pytest.raises(TypeError, match="float32"):
        ops.normal_nll_fwd_bwd(mean, dist, target.double(), "log_var", False, 1e-6, "mean")
    with pytest.raises(RuntimeError, match="lives on cpu"):
        ops.normal_nll_fwd_bwd(mean, dist, target.cpu(), "log_var", False, 1e-6, "mean")
    assert _count() == before  # nothing reached the device
    # shapes that only broadcast are torch's expression in the layer
    loss = cusrl.nn.NormalNllLoss()((mean, dist), target[:1])
    assert _count() == before and loss.shape == ()
