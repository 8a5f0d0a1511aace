"""The float64 references of the policy-statistics kernels (``oracle.policy_stats``, ``oracle.categorical_policy_stats``) pinned
without a GPU against float64 ``torch.distributions`` — what the reference's ``OnPolicyStatistics`` goes through — then every
case of the GPU tests (tests/test_policy_stats_gpu.py) run through a float32 numpy restatement of the kernels' per-row
arithmetic and the GPU tests' own assertions: correct fp32 arithmetic stays inside the bounds the kernels are held to."""

import numpy as np
import pytest
import torch

import _policy_stats as P
import oracle

CATEGORICAL = [case for case in P.CASES if case.family == "categorical"]
GAUSSIAN = [case for case in P.CASES if case.family == "gaussian"]


def _torch_categorical(data):
    """(kl, iw) of stats.py:28-40 through float64 torch.distributions: compute_kl_div / compute_logp of a one-hot actor."""
    from torch.distributions import OneHotCategorical, kl_divergence

    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731
    p = OneHotCategorical(logits=t(data["old_logits"]), validate_args=False)
    q = OneHotCategorical(logits=t(data["new_logits"]), validate_args=False)
    kl = kl_divergence(p, q).unsqueeze(-1)
    logp = q.log_prob(t(data["action"])).unsqueeze(-1)
    weighted = t(data["advantage"]) * (logp - t(data["old_logp"]).unsqueeze(-1)).exp()
    return kl.mean().item(), weighted.mean().item()


@pytest.mark.parametrize("case", [case for case in CATEGORICAL if case.B <= 257], ids=lambda case: case.name)
def test_categorical_oracle_is_float64_torch_distributions(case):
    data = P.inputs(case)
    if case.variant == "shifted":
        # torch's own float64 normaliser is rounded at the logits' magnitude (one ulp of 1e4 is 1.8e-12): compared on the
        # unshifted pair, which test_categorical_input_conditions shows to be the same distributions exactly
        want_kl, want_iw = _torch_categorical({**data, "old_logits": data["far"][0], "new_logits": data["far"][1]})
    else:
        want_kl, want_iw = _torch_categorical(data)
    (kl, iw, std), mass = oracle.categorical_policy_stats(*P.operands(case, data), return_mass=True)
    assert (kl, iw, std) == oracle.categorical_policy_stats(*P.operands(case, data)) and std == 0.0 and mass[2] == 0.0
    if case.variant == "masked_new_only":
        assert kl == np.inf and want_kl == np.inf and mass[0] == np.inf
    else:
        assert abs(kl - want_kl) <= 1e-12 * max(1.0, mass[0]), (kl, want_kl)
        assert np.isfinite(mass[0]) and abs(kl) <= mass[0] * (1 + 1e-12)
    assert abs(iw - want_iw) <= 1e-12 * max(1.0, mass[1]), (iw, want_iw)
    assert abs(iw) <= mass[1] * (1 + 1e-12)


def test_categorical_oracle_special_values_by_hand():
    """Two actions, probabilities written out: q_j = 0 < p_j makes the row +inf, p_j = 0 contributes nothing whatever q_j is,
    and where both are 0 the second overwrite wins."""
    log = np.log
    minus = -np.inf
    old = np.array([[log(0.25), log(0.75), minus], [log(0.25), log(0.75), minus], [log(0.5), minus, log(0.5)]])
    new = np.array([[log(0.5), log(0.5), minus], [log(0.5), log(0.25), log(0.25)], [log(0.5), log(0.5), minus]])
    action = np.array([[0, 1, 0], [0, 1, 0], [1, 0, 0]], np.float32)
    rows = [oracle.categorical_policy_stats(old[i:i + 1], new[i:i + 1], action[i:i + 1], np.zeros(1), np.ones((1, 2)), return_mass=True)
            for i in range(3)]
    want0 = 0.25 * log(0.25 / 0.5) + 0.75 * log(0.75 / 0.5)
    assert abs(rows[0][0][0] - want0) <= 1e-14 and abs(rows[0][0][1] - 0.5) <= 1e-14
    assert abs(rows[0][1][0] - (0.25 * (abs(log(0.25)) + log(2)) + 0.75 * (abs(log(0.75)) + log(2)))) <= 1e-14
    want1 = 0.25 * log(0.25 / 0.5) + 0.75 * log(0.75 / 0.25)  # the action only the old policy masks contributes 0
    assert abs(rows[1][0][0] - want1) <= 1e-14 and abs(rows[1][0][1] - 0.25) <= 1e-14
    assert rows[2][0][0] == np.inf and abs(rows[2][0][1] - 0.5) <= 1e-14  # only the new policy masks action 2


def test_gaussian_mass_does_not_disturb_the_statistics():
    """The inputs of test_oracle_golden.py::test_policy_stats_matches_torch_distributions: same three values with and without
    ``return_mass``, against torch.distributions, and a mass that dominates each of them."""
    from torch.distributions import Normal, kl_divergence

    rng = np.random.default_rng(5)
    B, A = 257, 6
    mp, mq = rng.standard_normal((B, A)).astype(np.float32), rng.standard_normal((B, A)).astype(np.float32)
    sp, sq = (rng.random((B, A)) + 0.5).astype(np.float32), (rng.random((B, A)) + 0.5).astype(np.float32)
    action = (mp + sp * rng.standard_normal((B, A))).astype(np.float32)
    advantage = rng.standard_normal((B, 1)).astype(np.float32)
    p, q = Normal(torch.from_numpy(mp), torch.from_numpy(sp)), Normal(torch.from_numpy(mq), torch.from_numpy(sq))
    old_logp = p.log_prob(torch.from_numpy(action)).sum(-1, keepdim=True)
    kl = kl_divergence(p, q).sum(-1, keepdim=True).mean().item()
    iw = (torch.from_numpy(advantage) * (q.log_prob(torch.from_numpy(action)).sum(-1, keepdim=True) - old_logp).exp()).mean().item()
    plain = oracle.policy_stats(mp, sp, mq, sq, action, old_logp.numpy(), advantage)
    stats, mass = oracle.policy_stats(mp, sp, mq, sq, action, old_logp.numpy(), advantage, return_mass=True)
    assert stats == plain and len(mass) == 3
    np.testing.assert_allclose(stats, (kl, iw, float(sq.mean())), rtol=2e-5)
    assert all(abs(s) <= m for s, m in zip(stats, mass)) and mass[2] == stats[2]
    # by hand, one element: r = 4, t1 = 1 -> 0.5 (4 + 1 + 1 + log 4)
    (_, _, _), (m_kl, m_iw, m_std) = oracle.policy_stats([[1.0]], [[2.0]], [[0.0]], [[1.0]], [[0.0]], [0.0], [[-2.0]], return_mass=True)
    assert abs(m_kl - 0.5 * (6.0 + np.log(4.0))) <= 1e-14 and m_std == 1.0
    assert abs(m_iw - 2.0 * np.exp(-0.5 * np.log(2.0 * np.pi))) <= 1e-14


@pytest.mark.parametrize("case", GAUSSIAN[:8], ids=lambda case: case.name)
def test_gaussian_oracle_is_float64_torch_distributions(case):
    from torch.distributions import Normal, kl_divergence

    data = P.inputs(case)
    t = lambda name: torch.from_numpy(np.asarray(data[name], np.float64))  # noqa: E731
    p, q = Normal(t("old_mean"), t("old_std")), Normal(t("new_mean"), t("new_std"))
    kl = kl_divergence(p, q).sum(-1, keepdim=True).mean().item()
    ratio = (q.log_prob(t("action")).sum(-1, keepdim=True) - t("old_logp").unsqueeze(-1)).exp()
    (got_kl, got_iw, got_std), mass = P.reference(case)
    assert abs(got_kl - kl) <= 1e-12 * mass[0] and abs(got_iw - (t("advantage") * ratio).mean().item()) <= 1e-12 * mass[1]
    assert abs(got_std - t("new_std").mean().item()) <= 1e-12 * mass[2]


@pytest.mark.parametrize("case", P.CASES, ids=lambda case: case.name)
def test_fp32_restatement_passes_the_gpu_assertions(case):
    P.check(case, P.F32.run(case, P.inputs(case)))


@pytest.mark.parametrize("case", CATEGORICAL, ids=lambda case: case.name)
def test_categorical_input_conditions(case):
    """Conditions on the inputs, not measurements: live normalised log-probabilities >= -60, masked ones exactly -inf, the
    log-ratio within +-20, a one-hot action live under both policies; and the float64 oracle and the fp32 restatement agree
    on which rows are infinite."""
    data = P.inputs(case)
    B, A = case.B, case.A
    rows = np.arange(B)
    for logits, masked in ((data["old_logits"], data["masked_old"]), (data["new_logits"], data["masked_new"])):
        assert logits.dtype == np.float32 and logits.shape == (B, A)
        assert case.variant == "masked_new_only" or not masked[:, 0].any()  # (that variant's one entry may be column 0)
        assert np.array_equal(np.isneginf(logits), masked) and np.isfinite(logits[~masked]).all()
        for normalised in (P._log_softmax(logits), P._log_softmax(logits.astype(np.float64)).astype(np.float32)):
            assert np.array_equal(np.isneginf(normalised), masked)
            assert (normalised[~masked] >= P.LIVE_LOG_PROBABILITY).all()
    taken = data["taken"]
    assert np.array_equal(data["action"].sum(-1), np.ones(B)) and np.array_equal(data["action"].argmax(-1), taken)
    assert not data["masked_old"][rows, taken].any() and not data["masked_new"][rows, taken].any()
    log_ratio = P._log_softmax(data["new_logits"])[rows, taken] - data["old_logp"].astype(np.float64)
    assert (np.abs(log_ratio) <= P.LOG_RATIO_LIMIT).all()
    infinite = (data["masked_new"] & ~data["masked_old"]).any(-1)
    if case.variant == "masked_new_only":
        assert np.array_equal(np.nonzero(infinite)[0], sorted({0, B // 2})) and (data["masked_new"].sum(-1) <= 1).all()
    else:
        assert not infinite.any()
    if case.variant == "masked_both":
        assert np.array_equal(data["masked_old"], data["masked_new"])
    if case.variant == "same":
        assert np.array_equal(data["old_logits"], data["new_logits"])
    if case.variant == "shifted":
        for shifted, far in zip((data["old_logits"], data["new_logits"]), data["far"]):
            shift = shifted.astype(np.float64) - far.astype(np.float64)  # exactly +-1e4, one constant per row
            assert np.array_equal(np.abs(shift), np.full((B, A), 1e4)) and (shift == shift[:, :1]).all()
    # row by row: float64 oracle and fp32 restatement classify the same rows as infinite
    per_row64 = np.array([oracle.categorical_policy_stats(data["old_logits"][i:i + 1], data["new_logits"][i:i + 1], data["action"][i:i + 1],
                                                          data["old_logp"][i:i + 1], data["advantage"][i:i + 1])[0]
                          for i in (range(B) if B <= 257 else sorted({0, 1, B // 2 - 1, B // 2, B // 2 + 1, B - 1}))])
    picked = np.arange(B) if B <= 257 else np.array(sorted({0, 1, B // 2 - 1, B // 2, B // 2 + 1, B - 1}))
    per_row32 = []
    for i in picked:
        row = {k: data[k][i:i + 1] for k in P.OPERANDS["categorical"]}
        per_row32.append(P.F32.run(case._replace(B=1), row)[0])
    assert np.array_equal(np.isinf(per_row64), infinite[picked]) and np.array_equal(np.isinf(per_row32), infinite[picked])
    assert np.isfinite(per_row64[~infinite[picked]]).all() and np.isfinite(np.array(per_row32)[~infinite[picked]]).all()


@pytest.mark.parametrize("case", GAUSSIAN, ids=lambda case: case.name)
def test_gaussian_input_conditions(case):
    data = P.inputs(case)
    log_ratio = P._normal_logp(data["action"], data["new_mean"], data["new_std"]) - data["old_logp"].astype(np.float64)
    assert (np.abs(log_ratio) <= P.LOG_RATIO_LIMIT).all()
    assert (data["old_std"] > 0).all() and (data["new_std"] > 0).all()
    if case.variant == "tiny_std":
        for std in (data["old_std"], data["new_std"]):
            assert (std >= np.float32(1e-3)).all() and (std <= np.float32(2e-3)).all()
    if case.variant == "same":
        assert np.array_equal(data["old_mean"], data["new_mean"]) and np.array_equal(data["old_std"], data["new_std"])


def test_case_table_covers_the_edges():
    """The shapes and variants the issue names are in the table (a guard against an edit that drops one)."""
    for family, widths, variants in (("categorical", {1, 2, 3, 18, 64}, P.CATEGORICAL_VARIANTS), ("gaussian", {1, 4, 12, 40}, P.GAUSSIAN_VARIANTS)):
        cases = [case for case in P.CASES if case.family == family]
        assert {case.B for case in cases} == {1, 63, 64, 65, 255, 256, 257, 65537, 70001}
        assert {case.A for case in cases} == widths == {case.A for case in cases if case.B == 257}
        for B in {case.B for case in cases}:
            assert any(case.A > 1 for case in cases if case.B == B) and any(case.D > 1 for case in cases if case.B == B), (family, B)
        assert {case.D for case in cases} == {1, 3} and {case.variant for case in cases} == set(variants)
        for variant in variants:  # every variant spans more than one workgroup and more than one finalize stride somewhere
            assert any(case.B > 256 for case in cases if case.variant == variant), (family, variant)
            assert any(case.B > 65536 for case in cases if case.variant == variant), (family, variant)
        assert max(case.B * case.A * 4 for case in cases) <= 18 * 2**20
    assert len({case.name for case in P.CASES}) == len(P.CASES) == len({case.seed for case in P.CASES})
    assert P.num_partials(65537) == 257 and P.num_partials(70001) == 274 and P.num_partials(256) == 1 and P.num_partials(257) == 2
    # the taken action is the last column somewhere, and not pinned to column 0
    taken = np.concatenate([P.inputs(case)["taken"] for case in P.CASES if case.family == "categorical" and case.B == 257 and case.A == 18])
    assert (taken == 17).any() and (taken != 0).mean() > 0.5
    assert not P.WIDENED  # (a widened bound needs its measured basis in the module docstring)
