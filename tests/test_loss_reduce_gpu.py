"""The reduction tail the loss kernels share (``csrc/loss_reduce.hpp``) at the sizes where it switches: 16 384 elements, the last
size one block finalises itself; the first sizes beyond it (9 blocks, a vector and a scalar shape); and ``[262145, 8]``, just
over 1024 * 2048 elements, where the grid is capped and every thread strides.  The block counts are asserted through the
``cusrl_*_num_partials`` exports, so a moved launch rule fails here instead of leaving the finalize launch uncovered.  Every op is
compared with a float64 evaluation of its formula — 1e-5 relative for a loss, for a gradient the bound of the family's own
test file — and called twice: the two results are bit-equal, the summation order being fixed."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from _smoothness import closed_form_f64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (shape, blocks): [.., 4] / [.., 8] rows take the 16-byte loops where an op has them, [.., 2] / [.., 3] rows the scalar ones
SHAPES = [((4096, 4), 1), ((8192, 2), 1), ((4097, 4), 9), ((5462, 3), 9), ((262145, 8), 1024)]
IDS = [f"{rows}x{K}" for (rows, K), _ in SHAPES]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    import cusrl_amd
    from cusrl_amd import ops

    cusrl_amd.config.set_device(DEV)
    return ops


def _lib():
    from cusrl_amd import _native

    return _native.lib()


def _randn(*shape, seed):
    return torch.randn(*shape, device=DEV, generator=torch.Generator(DEV).manual_seed(seed))


def _f64(tensor):
    return tensor.detach().cpu().double()


def _twice(call):
    """The op's outputs, after asserting that a second call on the same inputs repeats every one of them bit for bit."""
    first, second = call(), call()
    for a, b in zip(first, second):
        assert (a is None and b is None) or torch.equal(a.view(torch.int32), b.view(torch.int32)), "two calls on the same inputs differ"
    return first


def _check_loss(label, loss, reference):
    loss, reference = float(loss), float(reference.detach() if isinstance(reference, torch.Tensor) else reference)
    print(f"{label}: loss {loss:.9g} vs {reference:.9g} (rel {abs(loss - reference) / abs(reference):.2e})")
    np.testing.assert_allclose(loss, reference, rtol=1e-5)


@pytest.mark.parametrize(("shape", "blocks"), SHAPES, ids=IDS)
def test_mse_loss(ops, shape, blocks):
    n = shape[0] * shape[1]
    assert _lib().cusrl_mse_loss_num_partials(n) == blocks
    prediction, target = _randn(*shape, seed=1), _randn(*shape, seed=2)
    loss, grad = _twice(lambda: ops.mse_loss_fwd_bwd(prediction, target))
    difference = _f64(prediction) - _f64(target)
    _check_loss(f"mse{shape}", loss, difference.square().mean())
    np.testing.assert_allclose(grad.cpu().numpy(), (2.0 * difference / n).numpy(), rtol=1e-5, atol=1e-9)  # test_auxiliary_rewards.py


@pytest.mark.parametrize(("shape", "blocks"), SHAPES, ids=IDS)
def test_sumsq(ops, shape, blocks):
    assert _lib().cusrl_mse_loss_num_partials(shape[0] * shape[1]) == blocks
    x = _randn(*shape, seed=3)
    loss, grad = _twice(lambda: ops.sumsq_fwd_bwd(x, 0.3, 0.6))
    _check_loss(f"sumsq{shape}", loss, 0.3 * _f64(x).square().sum())
    np.testing.assert_allclose(grad.cpu().numpy(), (0.6 * x).cpu().numpy(), rtol=1e-6)  # test_auxiliary_rewards.py


@pytest.mark.parametrize("form", ["in_place", "column_table"])
@pytest.mark.parametrize(("shape", "blocks"), SHAPES, ids=IDS)
def test_column_mse(ops, gradient_parity, shape, blocks, form):
    """``in_place``: the first K columns of a K-wide target (the 16-byte loop for K % 4 == 0); ``column_table``: K columns picked
    out of a wider target in descending order (always the scalar loop)."""
    rows, K = shape
    assert _lib().cusrl_column_mse_num_partials(rows, K) == blocks
    prediction = _randn(rows, K, seed=4)
    if form == "in_place":
        target, columns, picked = _randn(rows, K, seed=5), None, slice(None)
    else:
        target = _randn(rows, K + 3, seed=5)
        picked = list(range(K + 1, 1, -1))
        columns = ops.column_table(picked, K + 3, DEV)
    loss, grad = _twice(lambda: ops.column_mse_fwd_bwd(prediction, target, columns, 0.7))
    difference = _f64(prediction) - _f64(target)[:, picked]
    _check_loss(f"column_mse{shape},{form}", loss, 0.7 * difference.square().mean())
    gradient_parity(f"loss_reduce.column_mse[{shape},{form}]", grad.cpu().numpy(), (1.4 * difference / (rows * K)).numpy(), 1e-5)


@pytest.mark.parametrize(("shape", "blocks"), SHAPES, ids=IDS)
def test_normal_nll(ops, gradient_parity, shape, blocks):
    rows, K = shape
    assert _lib().cusrl_normal_nll_num_partials(rows, K) == blocks
    mean, log_var, target = _randn(rows, K, seed=6), 0.5 * _randn(rows, K, seed=7), _randn(rows, K, seed=8)
    loss, d_mean, d_dist = _twice(lambda: ops.normal_nll_fwd_bwd(mean, log_var, target, "log_var", False, 1e-6, "mean"))
    m, d, t = _f64(mean).requires_grad_(), _f64(log_var).requires_grad_(), _f64(target)
    reference = (0.5 * (d + (t - m).square() / d.exp())).mean()  # (log_var stays far above log(eps): the clamp is idle)
    ref_mean, ref_dist = torch.autograd.grad(reference, (m, d))
    _check_loss(f"normal_nll{shape}", loss, reference)
    gradient_parity(f"loss_reduce.normal_nll.d_mean[{shape}]", d_mean.cpu().numpy(), ref_mean.numpy(), 1e-5)
    gradient_parity(f"loss_reduce.normal_nll.d_dist[{shape}]", d_dist.cpu().numpy(), ref_dist.numpy(), 1e-5)


@pytest.mark.parametrize(("shape", "blocks"), SHAPES, ids=IDS)
def test_mirror_loss_with_a_std_matrix(ops, shape, blocks):
    from cusrl_amd.hook import MirrorDef

    B, A = shape
    assert _lib().cusrl_mirror_mse_num_partials(B * A) == blocks
    rng = np.random.default_rng(A)
    dest, flipped = rng.permutation(A).tolist(), [0]
    mirror = MirrorDef(dest, flipped)
    mean, mirrored_mean = _randn(B, A, seed=9), _randn(B, A, seed=10)
    std, mirrored_std = _randn(B, A, seed=11).abs() + 0.1, _randn(B, A, seed=12)
    table = mirror.device_table(DEV, A)
    losses, *grads = _twice(lambda: ops.mirror_mse_fwd_bwd(mean, mirrored_mean, table, 0.5, std, mirrored_std))
    leaves = [_f64(t).requires_grad_() for t in (mean, mirrored_mean, std, mirrored_std)]
    sign, index = torch.tensor(mirror.multiplier.tolist(), dtype=torch.float64), torch.tensor(dest)
    loss_mean = 0.5 * (leaves[0] - leaves[1][:, index] * sign).square().mean()
    loss_std = 0.5 * (leaves[2] - (leaves[3][:, index] * sign).abs()).square().mean()
    _check_loss(f"mirror{shape}.mean", losses[0], loss_mean)
    _check_loss(f"mirror{shape}.std", losses[1], loss_std)
    for got, expected in zip(grads, torch.autograd.grad(loss_mean + loss_std, leaves)):
        achieved = (_f64(got) - expected).abs().max().item() / expected.abs().max().item()
        print(f"mirror{shape}: gradient {achieved:.2e} of the largest entry")
        assert achieved <= 1e-6  # test_symmetry_gpu.py


@pytest.mark.parametrize(("B", "A", "walk_blocks"), [(64, 4, 1), (257, 1, 2)], ids=["BA256", "BA257"])
def test_action_smoothness(ops, gradient_parity, B, A, walk_blocks):
    """``B * A`` = 256: the one walk block finishes its own sums; 257: two blocks and the finalize launch."""
    T = 4
    count_blocks = -(-B // 256)
    assert _lib().cusrl_action_smoothness_workspace(T, B, A) == 2 * (count_blocks + walk_blocks)
    mean = _randn(T, B, A, seed=13)
    done = torch.rand(T, B, 1, device=DEV, generator=torch.Generator(DEV).manual_seed(14)) < 0.2
    w1, w2 = torch.full((A,), 0.5, device=DEV), torch.full((A,), 0.25, device=DEV)
    losses, counts, d_mean = _twice(lambda: ops.action_smoothness_fwd_bwd(mean, done, w1, w2))
    reference = closed_form_f64(mean.cpu().numpy(), done.cpu().numpy(), [0.5] * A, [0.25] * A)
    assert counts.tolist() == [reference["n1"], reference["n2"]] and min(counts.tolist()) > 0
    _check_loss(f"smoothness[B{B},A{A}].1st", losses[0], reference["loss1"])
    _check_loss(f"smoothness[B{B},A{A}].2nd", losses[1], reference["loss2"])
    gradient_parity(f"loss_reduce.smoothness[B{B},A{A}]", (d_mean[0] + d_mean[1]).cpu().numpy(), reference["d_mean"], 1e-5)
