"""``cusrl_mlp3_forward`` (csrc/mlp3_forward.hip) on an MI355X: exact on the integer stacks of tests/_mlp3_forward.py (whose
conditions tests/test_mlp3_forward.py checks on the CPU), within four times the library chain's own error on random values,
row-independent, ``cusrl_normal_sample_logp`` behind the same mean, guarded, and reached from ``Actor`` / ``Value``."""

from __future__ import annotations

import pytest
import torch

import _mlp3_forward as M
from cusrl_amd import _native, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, SENTINEL = 64, 0x7FA5A5A5   # floats on either side of a guarded output, and the bits they hold


def _launches() -> int:
    return _native.launch_counts.get("cusrl_mlp3_forward", 0)


def _random_case(widths, K, A, rows, seed):
    """Default-initialised nn.Linear weights and normal inputs, on the device."""
    torch.manual_seed(seed)
    linears = [torch.nn.Linear(a, b) for a, b in zip((K, *widths), (*widths, A))]
    layers = tuple(t.detach().to(DEV) for m in linears for t in (m.weight, m.bias))
    return torch.randn(rows, K).to(DEV), layers


def _errors(x, layers, activation, got, chain):
    """Largest error of the kernel and of the library chain against float64, relative to the accumulated magnitude."""
    want, mag, _ = M.reference(x, layers, activation)
    e_kernel, e_chain = (float(((t.double().cpu() - want).abs() / mag).max()) for t in (got, chain))
    print(f"{activation} {tuple(x.shape)}: kernel {e_kernel:.3e}, library chain {e_chain:.3e} of the accumulated magnitude")
    return e_kernel, e_chain


@pytest.mark.parametrize("K", M.EXACT_KS)
@pytest.mark.parametrize("widths", M.TRIPLES, ids=str)
def test_integer_stacks_equal_float64(widths, K):
    for rows in M.EXACT_ROWS:
        for A in M.EXACT_OUTS:
            for bias4 in (True, False):
                x, layers, want = M.integer_case(K, widths, rows, A, bias4)
                x, layers = x.to(DEV), tuple(None if t is None else t.to(DEV) for t in layers)
                assert ops.mlp3_forward_supported(x, layers, "ReLU")
                before = _launches()
                got = ops.mlp3_forward(x, layers, "ReLU").double().cpu()
                assert _launches() == before + 1
                assert torch.equal(got, want), f"{K}->{widths}->{A} at {rows} rows, b4={bias4}: {int((got != want).sum())} differ"


@pytest.mark.parametrize("activation", ("ELU", "Tanh"))
@pytest.mark.parametrize("widths", M.TRIPLES, ids=str)
def test_random_values_within_four_times_the_library_chains_own_error(widths, activation):
    x, layers = _random_case(widths, 48, 12, 1000, seed=50)
    e_kernel, e_chain = _errors(x, layers, activation, ops.mlp3_forward(x, layers, activation, 1.0), M.library_chain(x, layers, activation))
    assert e_chain > 0 and e_kernel <= 4 * e_chain, (e_kernel, e_chain)


@pytest.mark.parametrize("widths", ((512, 256, 128), (128, 128, 128)), ids=str)
def test_rows_do_not_depend_on_tile_workgroup_or_row_count(widths):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for rows in (16 * cus - 1, 16 * cus + 17):   # either side of one grid round (and of the streamed regime's two tilings)
        x, layers = _random_case(widths, 48, 12, rows, seed=60)
        perm = torch.randperm(rows, generator=torch.Generator().manual_seed(61)).to(DEV)
        out = ops.mlp3_forward(x, layers, "ELU")
        assert torch.equal(ops.mlp3_forward(x[perm].contiguous(), layers, "ELU"), out[perm]), rows
        assert torch.equal(ops.mlp3_forward(x[:16].contiguous(), layers, "ELU"), out[:16]), rows


@pytest.mark.parametrize("A", (3, 12))
@pytest.mark.parametrize("widths", ((512, 256, 128), (128, 128, 128)), ids=str)
def test_sampling_epilogue_is_normal_sample_logp_behind_the_same_mean(widths, A):
    rows = 16 * torch.cuda.get_device_properties(0).multi_processor_count + 17
    x, layers = _random_case(widths, 48, A, rows, seed=70)
    eps, std = torch.randn(rows, A).to(DEV), (torch.rand(A) * 0.9 + 0.1).to(DEV)
    action, logp, mean, repeated = ops.mlp3_forward(x, layers, "ELU", std=std, eps=eps)
    assert torch.equal(mean, ops.mlp3_forward(x, layers, "ELU"))
    want_action, want_logp, want_repeated = ops.normal_sample_logp(mean, std, eps, repeat_std=True)
    assert torch.equal(action, want_action) and torch.equal(logp, want_logp) and torch.equal(repeated, want_repeated)


def _guarded(numel, offset=0):
    bits = torch.full((GUARD + offset + numel + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    return bits, bits.data_ptr() + 4 * (GUARD + offset)


@pytest.mark.parametrize("A", (1, 5, 12, 16))
def test_nothing_outside_the_outputs_is_written_and_refusals_write_nothing(A):
    lib, rows, K, widths = _native.lib(), 37, 48, (512, 256, 128)
    x, layers = _random_case(widths, K, A, rows, seed=80)
    eps, std = torch.randn(rows, A).to(DEV), (torch.rand(A) * 0.9 + 0.1).to(DEV)
    action, logp, mean, repeated = ops.mlp3_forward(x, layers, "ELU", std=std, eps=eps)

    def call(x_ptr, K, widths, layers, sampled, out_ptr, bufs=(None, None, None)):
        w1, b1, w2, b2, w3, b3, w4, b4 = (t.data_ptr() for t in layers)
        tail = (std.data_ptr(), eps.data_ptr(), *bufs) if sampled else (None,) * 5
        rc = lib.cusrl_mlp3_forward(x_ptr, rows, K, w1, b1, widths[0], w2, b2, widths[1], w3, b3, widths[2], w4, b4, A, 2, 1.0,
                                    out_ptr, *tail, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    for sampled in (True, False):
        (out, out_ptr), guarded = _guarded(rows * A), [_guarded(n) for n in (rows * A, rows, rows * A)]
        assert call(x.data_ptr(), K, widths, layers, sampled, out_ptr, tuple(ptr for _, ptr in guarded) if sampled else (None,) * 3) == 0
        for (bits, _), want in [(( out, out_ptr), mean)] + (list(zip(guarded, (action, logp, repeated))) if sampled else []):
            assert bool((bits[:GUARD] == SENTINEL).all()) and bool((bits[GUARD + want.numel():] == SENTINEL).all())
            assert torch.equal(bits[GUARD:GUARD + want.numel()], want.view(torch.int32).flatten())
    # refused by the host entry point, nothing launched: an unsupported triple, K = 68, a misaligned input
    wide = _random_case((512, 256, 64), K, A, rows, seed=81)[1]
    x68, layers68 = _random_case(widths, 68, A, rows, seed=82)
    shifted = torch.empty(rows * K + 1, device=DEV)[1:]
    for x_ptr, k, w, ls in ((x.data_ptr(), K, (512, 256, 64), wide), (x68.data_ptr(), 68, widths, layers68), (shifted.data_ptr(), K, widths, layers)):
        out, out_ptr = _guarded(rows * A)
        assert call(x_ptr, k, w, ls, False, out_ptr) == M.UNSUPPORTED
        assert bool((out == SENTINEL).all())


def test_actor_and_value_take_the_pass_without_grad_only():
    from cusrl_amd.nn import Actor, Mlp, NormalDist, Value
    from cusrl_amd.nn.module import Linear

    torch.manual_seed(90)
    actor = Actor(Mlp(48, (512, 256, 128), activation_fn="ELU", ends_with_activation=True), NormalDist(128, 12)).to(DEV)
    value = Value(Mlp(48, (128, 128, 128), activation_fn="ELU", ends_with_activation=True), Linear(128, 1)).to(DEV)
    observation = torch.randn(512, 48, device=DEV)

    stack = lambda backbone, head: tuple(t.detach() for m in (*backbone.layers[0::2], head) for t in (m.weight, m.bias))  # noqa: E731
    with torch.no_grad():
        before = _launches()
        fused_mean, fused_value = actor(observation)[0]["mean"], value.evaluate(observation)
        assert _launches() == before + 2
        torch.manual_seed(91)
        dist, (action, logp), _ = actor.explore(observation)
        assert _launches() == before + 3 and "backbone.output" not in actor.intermediate_repr
        assert torch.equal(dist["mean"], fused_mean) and action.shape == (512, 12) and logp.shape == (512, 1)
        actor.fused_inference = value.fused_inference = False
        chain_mean, chain_value = actor(observation)[0]["mean"], value.evaluate(observation)
        assert _launches() == before + 3
        actor.fused_inference = value.fused_inference = True
    for layers, got, chain in ((stack(actor.backbone, actor.distribution.mean_head), fused_mean, chain_mean),
                               (stack(value.backbone, value.value_head), fused_value, chain_value)):
        e_kernel, e_chain = _errors(observation, layers, "ELU", got, chain)
        assert e_chain > 0 and e_kernel <= 4 * e_chain, (e_kernel, e_chain)
    before = _launches()
    out, _ = actor(observation)   # with autograd on, the differentiable chain runs (and leaves the latent)
    assert out["mean"].requires_grad and value.evaluate(observation).requires_grad and _launches() == before
    assert "backbone.output" in actor.intermediate_repr


def test_captured_rollout_of_a_streamed_actor_replays_as_one_graph():
    """(512, 256, 128) is fused in the eager warm-up steps and left to the chain inside a capture: the whole-rollout graph must
    still be captured and replayed, with no exploration noise drawn ahead for steps that would not take it."""
    import cusrl_amd as cusrl

    cusrl.config.set_device(DEV)
    cusrl.set_global_seed(21)
    env = cusrl.testing.DummyTorchEnvironment(num_instances=256, observation_dim=12, action_dim=4, device=DEV)
    factory = cusrl.preset.PpoAgentFactory(
        num_steps_per_update=8, sampler_epochs=2, sampler_mini_batches=2, compile=True, activation_fn="ELU",
        actor_hidden_dims=(512, 256, 128), critic_hidden_dims=(128, 128, 128), optimizer_kwargs={"capturable": True, "fused": True})
    trainer = cusrl.Trainer(env, factory, num_iterations=6, verbose=False)
    trainer.capture_rollout = True
    before = _launches()
    trainer.run_training_loop()
    graphed = trainer._graphed_rollout
    assert env.generator_free and len(graphed.rollouts) == 1 and graphed.rollout_replays == 2 and graphed.noise_draws == 0
    assert _launches() > before and all(bool(p.isfinite().all()) for p in trainer.agent.parameters())
