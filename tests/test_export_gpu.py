"""The deploy kernels and ``nn.DeployedPolicy`` on an MI355X: ``cusrl_deploy_prologue`` against the two launches it replaces and
against its host restatement, ``cusrl_deploy_epilogue`` against the torch expression and its host restatement (all bit for
bit), the three policies of ``export.npz`` on the device, and a 4096-env policy against the agent's own deterministic act."""

from __future__ import annotations

import math

import pytest
import torch

import _export as shared

pytestmark = pytest.mark.gpu
DEVICE = "cuda:0"


@pytest.fixture(scope="module")
def cusrl():
    import cusrl_amd

    return cusrl_amd


@pytest.fixture(scope="module")
def g(golden):
    return golden("export")


def _bits(tensor: torch.Tensor) -> torch.Tensor:
    return tensor.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ prologue
EPSILON = 1e-8
REPLACE = (0.25, 7.0, -7.0)


def _prologue_operands(B: int, K: int, offset: bool):
    """Observations with NaN, +Inf and -Inf in them (row 0 and the last row at least), statistics with a channel whose std is
    sqrt(epsilon); ``offset``: the observation is a slice one float behind a 16-byte boundary."""
    gen = torch.Generator().manual_seed(1000 * B + 10 * K + offset)
    flat = torch.randn(B * K + 1, generator=gen) * 3.0
    observation = flat[1:].view(B, K) if offset else flat[:-1].view(B, K)
    specials = (float("nan"), float("inf"), float("-inf"), -0.0, 1e-41)
    for i, value in enumerate(specials):
        observation[(i * 7) % B, (i * 3) % K] = value
        observation[B - 1 - (i * 5) % B, K - 1 - (i * 2) % K] = value
    mean = torch.randn(K, generator=gen)
    std = torch.rand(K, generator=gen) + 0.1
    std[K // 2] = math.sqrt(EPSILON)  # a constant channel: var = 0
    device_flat = flat.to(DEVICE)
    device_observation = device_flat[1:].view(B, K) if offset else device_flat[:-1].view(B, K)
    assert device_observation.is_contiguous() and (device_observation.data_ptr() % 16 != 0) == offset
    return observation.contiguous(), device_observation, mean, std


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset"])
@pytest.mark.parametrize("K", [1, 7, 48])
@pytest.mark.parametrize("B", [1, 3, 257])
def test_prologue_has_the_bits_of_the_two_launches_and_of_its_host_restatement(cusrl, B, K, offset):
    from cusrl_amd import _native, ops

    observation, device_observation, mean, std = _prologue_operands(B, K, offset)
    device_mean, device_std = mean.to(DEVICE), std.to(DEVICE)
    zero, one = torch.zeros(K, device=DEVICE), torch.ones(K, device=DEVICE)
    # each optional part absent in turn (and all of them present); an absent normaliser is the identity (x - 0) / 1
    for replace, normalize, clamp in ((REPLACE, True, 5.0), (None, True, 5.0), (REPLACE, False, 5.0), (REPLACE, True, None),
                                      (REPLACE, False, None), (None, False, None)):
        chained = device_observation.clone()
        if replace is not None:
            ops.nan_to_num_(chained, nan=replace[0], posinf=replace[1], neginf=replace[2])
        if normalize or clamp is not None:
            chained = ops.rms_normalize(chained, device_mean if normalize else zero, device_std if normalize else one, clamp)
        before = _native.launch_counts.get("cusrl_deploy_prologue", 0)
        fused = ops.deploy_prologue(device_observation, replace, device_mean if normalize else None, device_std if normalize else None,
                                    clamp)
        assert _native.launch_counts["cusrl_deploy_prologue"] == before + 1
        host = ops.deploy_prologue_cpu(observation, replace, mean if normalize else None, std if normalize else None, clamp)
        label = f"replace={replace is not None} normalize={normalize} clamp={clamp}"
        assert torch.equal(_bits(fused), _bits(chained)), label
        assert torch.equal(_bits(fused), _bits(host)), label
    in_place = device_observation.clone()
    assert ops.deploy_prologue(in_place, REPLACE, device_mean, device_std, 5.0, out=in_place) is in_place
    assert torch.equal(_bits(in_place), _bits(ops.deploy_prologue(device_observation, REPLACE, device_mean, device_std, 5.0)))


def test_deploy_entries_check_their_arguments_without_a_launch(cusrl):
    from cusrl_amd import _native, ops

    lib = _native.lib()
    p = 0x1000
    assert lib.cusrl_deploy_prologue(p, None, p, None, 1.0, p, 4, 4, None) == -1  # mean without std
    assert lib.cusrl_deploy_prologue(None, None, None, None, 1.0, p, 4, 4, None) == -1
    assert lib.cusrl_deploy_prologue(p, None, None, None, 1.0, p, 4, 0, None) == -1
    assert lib.cusrl_deploy_prologue(p + 2, None, None, None, 1.0, p, 4, 4, None) == -1
    assert lib.cusrl_deploy_prologue(p, None, None, None, 1.0, p, 4, 2**31, None) == -3
    assert lib.cusrl_deploy_prologue(None, None, None, None, 1.0, None, 0, 4, None) == 0  # B == 0: nothing launched
    assert lib.cusrl_deploy_epilogue(p, None, p, None, None, None, 4, 4, None, None, 0, None) == -1  # scale without shift
    assert lib.cusrl_deploy_epilogue(p, None, None, None, p, None, 4, 4, None, None, 0, None) == -1  # lo without hi
    assert lib.cusrl_deploy_epilogue(p, None, None, None, None, None, 4, 4, p, None, 8, None) == -1  # done without memory
    assert lib.cusrl_deploy_epilogue(None, p, None, None, None, None, 4, 4, None, None, 0, None) == -1
    assert lib.cusrl_deploy_epilogue(p, p, None, None, None, None, 4, 2**31, None, None, 0, None) == -3
    assert lib.cusrl_deploy_epilogue(None, None, None, None, None, None, 0, 4, None, None, 0, None) == 0
    with pytest.raises(ValueError, match="contiguous fp32"):
        ops.deploy_prologue(torch.zeros(4, 4), None)
    with pytest.raises(ValueError, match="together"):
        ops.deploy_prologue(torch.zeros(4, 4, device=DEVICE), None, torch.zeros(4, device=DEVICE), None)


# ------------------------------------------------------------------------------------------------ epilogue
@pytest.mark.parametrize("M", [8, 16])
@pytest.mark.parametrize("A", [1, 12])
@pytest.mark.parametrize("B", [1, 3, 257])
def test_epilogue_has_the_bits_of_the_torch_expression_and_leaves_other_memory_rows_alone(cusrl, B, A, M):
    from cusrl_amd import _native, ops

    gen = torch.Generator().manual_seed(100 * B + 10 * A + M)
    y = torch.randn(B, A, generator=gen) * 2.0
    bias, scale, shift = torch.randn(A, generator=gen), torch.rand(A, generator=gen) * 3.0 + 0.1, torch.randn(A, generator=gen)
    lo, hi = -torch.rand(A, generator=gen) - 0.2, torch.rand(A, generator=gen) + 0.2
    memory = torch.randn(B, M, generator=gen)
    mixed = torch.rand(B, generator=gen) < 0.5
    mixed[0] = True
    if B > 1:
        mixed[1] = False
    dones = {"none": None, "all false": torch.zeros(B, dtype=torch.bool), "all true": torch.ones(B, dtype=torch.bool), "mixed": mixed}
    parts = [(True, True), (True, False), (False, True), (False, False)]  # (affine, clip): each optional part absent in turn
    for (affine, clip), (label, done) in [(p, d) for p in parts for d in dones.items()]:
        expected = y + bias
        if affine:
            expected = expected * scale  # one multiply, then one add: two roundings
            expected = expected + shift
        if clip:
            expected = torch.clamp(expected, lo, hi)
        expected_memory = memory.clone()
        if done is not None:
            expected_memory[done] = 0
        device_y, device_memory = y.to(DEVICE), memory.to(DEVICE)
        arguments = lambda move: (move(bias), move(scale) if affine else None, move(shift) if affine else None,  # noqa: E731
                                  move(lo) if clip else None, move(hi) if clip else None, None if done is None else move(done))
        before = _native.launch_counts.get("cusrl_deploy_epilogue", 0)
        assert ops.deploy_epilogue_(device_y, *arguments(lambda t: t.to(DEVICE)), device_memory if done is not None else None) is device_y
        assert _native.launch_counts["cusrl_deploy_epilogue"] == before + 1  # the action and the memory rows: ONE launch
        host_y, host_memory = y.clone(), memory.clone()
        ops.deploy_epilogue_cpu_(host_y, *arguments(lambda t: t), host_memory if done is not None else None)
        what = f"affine={affine} clip={clip} done={label}"
        assert torch.equal(_bits(device_y), _bits(expected)), what
        assert torch.equal(_bits(host_y), _bits(expected)), what
        assert torch.equal(_bits(device_memory), _bits(expected_memory)), what  # rows outside `done`: untouched, bit for bit
        assert torch.equal(_bits(host_memory), _bits(expected_memory)), what


def test_epilogue_takes_a_memory_off_a_16_byte_boundary_and_of_odd_width(cusrl):
    from cusrl_amd import ops

    flat = torch.randn(5 * 7 + 1, device=DEVICE)
    memory = flat[1:].view(5, 7)
    kept = memory.clone()
    done = torch.tensor([True, False, False, True, False], device=DEVICE)
    y = torch.randn(5, 3, device=DEVICE)
    expected = y + 1.0
    ops.deploy_epilogue_(y, torch.ones(3, device=DEVICE), done=done, memory=memory)
    kept[done] = 0
    assert torch.equal(memory, kept) and torch.equal(y, expected) and float(flat[0]) != 0.0


# ------------------------------------------------------------------------------------------------ the policy on the device
@pytest.fixture(scope="module")
def policies(cusrl, g, tmp_path_factory):
    directory = tmp_path_factory.mktemp("export_gpu")
    return {case: cusrl.DeployedPolicy.load(shared.build_agent(cusrl, g, case).export(directory, case), map_location=DEVICE)
            for case in shared.CASES}


@pytest.mark.parametrize("case", shared.CASES)
def test_deployed_policy_reproduces_the_reference_on_the_device(cusrl, g, policies, case):
    from cusrl_amd import _native

    policy = policies[case]
    counts = dict(_native.launch_counts)
    actions, memories, resets = shared.replay(policy, g, case, DEVICE)
    moved = lambda name: _native.launch_counts.get(name, 0) - counts.get(name, 0)  # noqa: E731
    steps = actions.shape[0]
    assert moved("cusrl_deploy_prologue") == (steps if case != "lstm" else 0)  # (the LSTM case has nothing in front of its GEMM)
    assert moved("cusrl_deploy_epilogue") == steps  # the native path ran, not the torch expression
    assert actions.is_cuda and shared.relative_to_largest(actions, torch.from_numpy(g[f"{case}/action"])) <= shared.PARITY
    if case == "mlp":
        return
    assert shared.relative_to_largest(memories, torch.from_numpy(g[f"{case}/memory"])) <= shared.PARITY
    assert shared.relative_to_largest(resets, torch.from_numpy(g[f"{case}/memory_reset"])) <= shared.PARITY
    done = torch.from_numpy(g[f"{case}/done"]).to(DEVICE)
    assert (resets[done] == 0).all() and torch.equal(resets[~done], memories[~done])
    # a call with done= is a call followed by reset(done), bit for bit — and one launch less
    fused_actions, _, fused_resets = shared.replay(policy, g, case, DEVICE, fused_done=True)
    assert torch.equal(_bits(fused_actions), _bits(actions)) and torch.equal(_bits(fused_resets), _bits(resets))


def test_non_native_inputs_take_the_torch_expression_and_cpu_tensors_are_refused(cusrl, g, policies):
    policy = policies["mlp"]
    observation = torch.from_numpy(g["mlp/observation"])[0].to(DEVICE)
    native = policy(observation)
    strided = torch.stack([observation, observation], dim=-1)[..., 0]
    assert not strided.is_contiguous()
    for other in (policy(strided), policy(observation.double())):
        assert other.dtype == torch.float32 and shared.relative_to_largest(other, native) <= shared.PARITY
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert shared.relative_to_largest(policy(observation), native) <= shared.PARITY
    with pytest.raises(RuntimeError, match="CPU tensors"):
        policy.to("cpu")(observation.cpu())
    policy.to(DEVICE)


def test_a_4096_env_policy_equals_the_agents_own_deterministic_act(cusrl, tmp_path):
    from cusrl_amd import _native

    torch.manual_seed(7)
    factory = cusrl.preset.PpoAgentFactory(num_steps_per_update=8, normalize_observation=True, device=DEVICE)
    agent = factory(cusrl.template.environment.EnvironmentSpec(48, 12, device=DEVICE))
    observation = torch.randn(4096, 48, device=DEVICE) * 2.0 + 0.5
    agent.act(observation)  # the statistics see a batch: mean and std leave 0 and 1
    policy = cusrl.DeployedPolicy.load(agent.export(tmp_path), map_location=DEVICE)
    agent.set_inference_mode(True, deterministic=True)  # the parent's path: agent.act with deterministic=True
    expected = agent.act(observation.clone())
    before = _native.launch_counts.get("cusrl_mlp2_forward", 0)
    action = policy(observation)
    assert _native.launch_counts.get("cusrl_mlp2_forward", 0) == before + 1  # the shape the one-launch inference pass takes
    assert tuple(action.shape) == (4096, 12) and shared.relative_to_largest(action, expected) <= shared.PARITY
