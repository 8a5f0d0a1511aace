"""``cusrl_attn_step_forward`` (csrc/attention_step.hip) on an MI355X: against its formulas (include/cusrl_hip.h) in float64 within
the bound of every MFMA attention kernel, the rolled window bit for bit, its edges, and reached from the causal encoder layer inside
``ops.fused_attention_step()`` with the same memories as outside it."""

from __future__ import annotations

import math

import pytest
import torch

from _attention import BOUND, relative_to_largest
from cusrl_amd import _native, nn, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SYMBOL = "cusrl_attn_step_forward"
UNSUPPORTED = -3                   # CUSRL_E_UNSUPPORTED
GUARD, SENTINEL = 64, 0x7FA5A5A5   # words on either side of a guarded output, and the bits they hold
N = 273


def _case(W, C, H, slopes, seed=0, n=N):
    generator = torch.Generator().manual_seed(seed)
    draw = lambda *shape: torch.randn(*shape, generator=generator)  # noqa: E731
    mask = torch.rand(n, W, generator=generator) < 0.5
    return {"qf": draw(n, H, C), "x": draw(n, C), "cache": draw(n, W, C), "mask": mask,
            "slopes": torch.tensor(nn.causal_attn.get_alibi_slopes(H)) if slopes else None, "scale": 1.0 / math.sqrt(C)}


def _formulas(case):
    """ctx by the header's formulas in float64: the softmax over the visible keys of the raw window, the new input last."""
    window = torch.cat([case["cache"], case["x"][:, None]], dim=1).double()
    W = case["cache"].shape[1]
    s = torch.einsum("nhc,njc->nhj", case["qf"].double(), window) * torch.tensor(case["scale"], dtype=torch.float32).double()
    if case["slopes"] is not None:
        s = s - case["slopes"].double()[None, :, None] * (W - torch.arange(W + 1)).double()
    visible = torch.cat([case["mask"], torch.ones(len(window), 1, dtype=torch.bool)], dim=1)
    return torch.einsum("nhj,njc->nhc", s.masked_fill(~visible[:, None], -math.inf).softmax(-1), window)


def _launch(case, cache=True, out=None):
    on = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    before = _native.launch_counts.get(SYMBOL, 0)
    got = ops.attention_step_forward(on(case["qf"]), on(case["x"]), on(case["cache"]) if cache else None, on(case["mask"]) if cache else None,
                                     on(case["slopes"]), scale=case["scale"], window=case["cache"].shape[1], out=out)
    assert _native.launch_counts.get(SYMBOL, 0) == before + 1
    return got


@pytest.mark.parametrize("slopes", (False, True))
@pytest.mark.parametrize("H", (1, 3, 16))
@pytest.mark.parametrize("C", (4, 20, 64, 128))
@pytest.mark.parametrize("W", (1, 15, 16, 17, 40))
def test_the_kernel_matches_its_formulas_and_rolls_the_window(W, C, H, slopes):
    case = _case(W, C, H, slopes)
    ctx, cache_out, mask_out = _launch(case)
    error = relative_to_largest(ctx, _formulas(case))
    print(f"W={W} C={C} H={H} slopes={slopes}: {error:.3e} of the largest entry")
    assert torch.isfinite(ctx).all() and error <= BOUND
    want_cache = torch.cat([case["cache"][:, 1:], case["x"][:, None]], dim=1)
    want_mask = torch.cat([case["mask"][:, 1:], torch.ones(N, 1, dtype=torch.bool)], dim=1)
    assert mask_out.dtype == torch.bool and torch.equal(mask_out.cpu(), want_mask)
    assert torch.equal(cache_out.cpu().view(torch.int32), want_cache.view(torch.int32))


@pytest.mark.parametrize("W, C, H", ((17, 20, 3), (40, 128, 16)))
def test_hidden_keys_contribute_exactly_nothing(W, C, H):
    case = _case(W, C, H, slopes=True, seed=1)
    alone = case["x"][:, None].expand(-1, H, -1).to(DEV)
    assert torch.equal(_launch(dict(case, mask=torch.zeros_like(case["mask"])))[0], alone)   # an all-hidden cache
    ctx, cache_out, mask_out = _launch(case, cache=False)                                      # no cache at all
    assert torch.equal(ctx, alone) and not cache_out[:, :-1].any() and torch.equal(cache_out[:, -1].cpu(), case["x"])
    assert mask_out.dtype == torch.bool and not mask_out[:, :-1].any() and mask_out[:, -1].all()
    poisoned = torch.where(case["mask"][:, :, None], case["cache"], torch.full_like(case["cache"], math.nan))
    assert torch.equal(_launch(dict(case, cache=poisoned))[0], _launch(case)[0])              # NaN in the hidden rows


def test_a_rows_bits_do_not_depend_on_the_batch():
    case = _case(17, 20, 3, slopes=True, seed=2)
    whole = _launch(case)
    for n in (0, 5, N - 1):
        one = {key: value[n:n + 1] if key in ("qf", "x", "cache", "mask") else value for key, value in case.items()}
        assert all(torch.equal(got[0], want[n]) for got, want in zip(_launch(one), whole))


def _guarded(shape, dtype):
    sentinel = SENTINEL if dtype == torch.float32 else 0xA5
    words = torch.full((GUARD + math.prod(shape) + GUARD,), sentinel, dtype=torch.int32 if dtype == torch.float32 else torch.uint8, device=DEV)
    return words, words[GUARD:-GUARD].view(dtype).view(shape), sentinel


def test_guard_words_stay_and_overlapping_buffers_are_refused():
    W, C, H = 17, 20, 3
    case = _case(W, C, H, slopes=False, seed=3)
    guarded = [_guarded(shape, dtype) for shape, dtype in (((N, H, C), torch.float32), ((N, W, C), torch.float32), ((N, W), torch.bool))]
    got = _launch(case, out=tuple(view for _, view, _ in guarded))
    assert all(torch.equal(a, b) for a, b in zip(got, _launch(case)))
    for words, _, sentinel in guarded:
        assert bool((words[:GUARD] == sentinel).all()) and bool((words[-GUARD:] == sentinel).all())

    qf, x, cache, mask = (case[name].to(DEV) for name in ("qf", "x", "cache", "mask"))

    def refused(ctx=None, cache_out=None, mask_out=None):
        fresh = [_guarded(shape, dtype)[1] for shape, dtype in (((N, H, C), torch.float32), ((N, W, C), torch.float32), ((N, W), torch.uint8))]
        outs = [given if given is not None else own for given, own in zip((ctx, cache_out, mask_out), fresh)]
        rc = getattr(_native.lib(), SYMBOL)(qf.data_ptr(), x.data_ptr(), cache.data_ptr(), mask.data_ptr(), None, 1.0, *(o.data_ptr() for o in outs),
                                            N, H, W, C, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc == UNSUPPORTED and bool((fresh[0].view(torch.int32) == SENTINEL).all()) and bool((fresh[2] == 0xA5).all())

    assert refused(cache_out=cache) and refused(mask_out=mask.view(torch.uint8)) and refused(ctx=qf) and refused(cache_out=cache[1:])


def _attention64(attn, x, memory):
    """The attention module's step in float64: both projections, the masked softmax over the window, ``out_proj``."""
    n, W, H, D = len(x), attn.window_size, attn.num_heads, attn.head_dim
    p = {name: value.detach().double().cpu() for name, value in attn.named_parameters()}
    cache = torch.zeros(n, W, x.shape[-1]) if memory is None else memory["input_cache"].cpu().view(n, W, -1)
    visible = torch.zeros(n, W, dtype=torch.bool) if memory is None else memory["cache_mask"].cpu()
    window = torch.cat([cache, x.cpu()[:, None]], dim=1).double()
    q = (x.double().cpu() @ p["q_proj.weight"].T + p["q_proj.bias"]).view(n, H, D)
    k, v = (window @ p["kv_proj.weight"].T + p["kv_proj.bias"]).view(n, W + 1, 2, H, D).unbind(2)
    s = torch.einsum("nhd,njhd->nhj", q, k) * torch.tensor(1.0 / math.sqrt(D), dtype=torch.float32).double()
    if attn.alibi_slopes is not None:
        s = s - attn.alibi_slopes.double().cpu()[None, :, None] * (W - torch.arange(W + 1)).double()
    visible = torch.cat([visible, torch.ones(n, 1, dtype=torch.bool)], dim=1)
    o = torch.einsum("nhj,njhd->nhd", s.masked_fill(~visible[:, None], -math.inf).softmax(-1), v)
    return o.flatten(1) @ p["out_proj.weight"].T + p["out_proj.bias"]


@pytest.mark.parametrize("layer_norm", (None, "pre", "post"))
@pytest.mark.parametrize("use_alibi", (False, True))
def test_the_layer_steps_through_the_kernel_inside_the_context(use_alibi, layer_norm):
    """Worst pairs measured (folded, unfolded): DESIGN.md §7 "Attention step on the matrix cores"."""
    torch.manual_seed(4)
    n, E, W = 37, 32, 5
    layer = nn.CausalTransformerEncoderLayer(E, 4, W, use_alibi=use_alibi, layer_norm=layer_norm).to(DEV)
    attended = []   # what self_attn returned: the unfolded call, then the folded one, per step
    layer.self_attn.register_forward_hook(lambda module, args, result: attended.append(result[0]))
    memories, worst = [None, None], [0.0, 0.0]
    with torch.no_grad():
        for t in range(8):
            x = torch.randn(n, E, device=DEV)
            if t == 4:
                done = torch.rand(n, 1, device=DEV) < 0.5
                for memory in memories:
                    layer.reset_memory(memory, done)
            if t == 6:
                layer.self_attn.q_proj.weight.mul_(1.5)   # the folded weights must follow
            before, old = _native.launch_counts.get(SYMBOL, 0), memories[0]
            outputs = [None, None]
            outputs[0], memories[0] = layer(x, memories[0])
            assert _native.launch_counts.get(SYMBOL, 0) == before
            with ops.fused_attention_step():
                outputs[1], memories[1] = layer(x, memories[1])
            assert _native.launch_counts.get(SYMBOL, 0) == before + 1
            assert outputs[0].shape == outputs[1].shape == (n, E) and torch.isfinite(outputs[1]).all()
            for key in ("input_cache", "cache_mask"):
                assert memories[0][key].dtype == memories[1][key].dtype and torch.equal(memories[0][key], memories[1][key]), (t, key)
            want = _attention64(layer.self_attn, memories[0]["input_cache"][:, -E:], old)
            errors = [relative_to_largest(got, want) for got in attended[-2:]]
            worst = max(worst, errors, key=lambda pair: abs(pair[1] - pair[0]))
            assert max(errors) <= BOUND, (t, errors)
    print(f"alibi={use_alibi} layer_norm={layer_norm}: unfolded {worst[0]:.3e}, folded {worst[1]:.3e} of the largest entry")
