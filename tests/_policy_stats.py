"""Shared by the tests of ``csrc/policy_stats.hip`` (tests/test_policy_stats.py on the CPU, test_policy_stats_gpu.py on the
device): the case table, the seeded inputs, the float64 references (``oracle.policy_stats`` /
``oracle.categorical_policy_stats``), the assertions, and a float32 numpy restatement of each kernel's per-row arithmetic —
fp32 inside a row, float64 across rows, as the kernels do — that the CPU test runs through those very assertions: the
evidence, obtainable without a GPU, that correct fp32 code stays inside the bounds the device is held to.

A case is ``(family, B, A, D, variant, seed)``.  B sits at the wave (64) and workgroup (256) edges and at 65537 / 70001 rows:
257 and 274 partial rows, i.e. past one stride of the finalize loop, the second with a ragged last workgroup.

Bounds — one rule: a statistic lies within ``1e-5 * mass`` of the float64 value, ``mass`` being the mean of the absolute
values of every term that enters its sum (``return_mass`` of the oracle): the project's standing fp32 bar.  Exact where the
arithmetic is exact: the KL of ``same`` is 0.0, the KL of ``masked_new_only`` is +inf, slot 2 of the categorical family is 0.0.
No variant needed a wider bound: over all cases the restatement's worst error, in units of ``1e-5 * mass``, is 0.43 (the
Gaussian importance-weighted advantage of ``tiny_std`` at B = 65, A = 40, where |logp| ~ 200 turns the fp32 rounding of a
row's log-probability into a relative error of its weight; 0.21 for ``close``, 0.09 for ``far``), 0.0006 for the ``close``
Gaussian KL (its terms cancel to ~1e-3 of their mass, which is why the mass and not the value is the yardstick), below 0.01
for every ``action_std`` and below 0.08 for every categorical statistic.

Input conditions (checked by the CPU test, not measured): every live normalised log-probability is >= -60 and every masked
one is exactly -inf — the kernel decides ``q_j == 0`` on ``expf(z - logsumexp)`` and torch on the softmax probabilities, which
differ only in a band near fp32 underflow; |log-ratio| <= 20.  The ``far`` logits are multiples of 2^-8 inside +-16, so that
the +-1e4 row constants of ``shifted`` are added exactly: ``shifted`` is the same pair of distributions as ``far``."""

from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import oracle

BLOCK = 256  # rows per workgroup of both kernels and threads of the finalize
RELATIVE = 1e-5
LOG_RATIO_LIMIT = 20.0
LIVE_LOG_PROBABILITY = -60.0
# {(family, variant, statistic index): bound in units of mass} — empty: the rule above holds for every case
WIDENED: dict[tuple[str, str, int], float] = {}

CATEGORICAL_VARIANTS = ("close", "far", "same", "masked_both", "masked_old_only", "masked_new_only", "shifted")
GAUSSIAN_VARIANTS = ("close", "far", "same", "tiny_std")


class Case(NamedTuple):
    family: str  # categorical | gaussian
    B: int
    A: int
    D: int
    variant: str
    seed: int

    @property
    def name(self) -> str:
        return f"{self.family}/{self.variant}/B{self.B}A{self.A}D{self.D}"


def num_partials(B: int) -> int:
    return -(-B // BLOCK)


def _table() -> list[Case]:
    cases = []

    def add(family, B, A, D, variants):
        for variant in variants:
            if family == "categorical" and A == 1 and variant.startswith("masked"):
                continue  # (one action: column 0 is always live, there is nothing to mask)
            cases.append(Case(family, B, A, D, variant, len(cases) + 1))

    # every B with an A > 1 and a D > 1; every A at B = 257; all variants at every small shape
    for B, A, D in ((1, 3, 3), (1, 64, 1), (63, 18, 1), (63, 2, 3), (64, 3, 3), (65, 18, 3), (255, 2, 3), (256, 64, 3),
                    (257, 1, 1), (257, 2, 3), (257, 3, 1), (257, 18, 3), (257, 64, 1)):
        add("categorical", B, A, D, CATEGORICAL_VARIANTS)
    add("categorical", 65537, 3, 3, ("far", "masked_both", "masked_new_only"))
    add("categorical", 65537, 18, 1, ("close", "masked_old_only"))
    add("categorical", 70001, 3, 3, ("same", "shifted", "masked_new_only"))
    add("categorical", 70001, 64, 1, ("close", "far"))  # 17.9 MB per [B, A] operand: the largest case
    for B, A, D in ((1, 4, 3), (1, 1, 1), (63, 12, 3), (64, 4, 3), (65, 40, 1), (65, 4, 3), (255, 12, 3), (256, 4, 3),
                    (257, 1, 3), (257, 4, 1), (257, 12, 3), (257, 40, 1)):
        add("gaussian", B, A, D, GAUSSIAN_VARIANTS)
    add("gaussian", 65537, 4, 3, ("close", "far"))
    add("gaussian", 65537, 12, 1, ("same", "tiny_std"))
    add("gaussian", 70001, 12, 3, ("close", "far", "tiny_std"))
    add("gaussian", 70001, 40, 1, ("far", "same"))
    return cases


CASES = _table()


def find(family: str, variant: str, B: int, A: int | None = None) -> Case:
    return next(c for c in CASES if (c.family, c.variant, c.B) == (family, variant, B) and A in (None, c.A))


# ------------------------------------------------------------------------------------------------ inputs
def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _log_softmax(z):
    z = np.asarray(z, np.float64)
    m = z.max(-1, keepdims=True)
    return (z - m) - np.log(np.exp(z - m).sum(-1, keepdims=True))


def _far_logits(rng, B, A):
    return np.clip(np.round(4.0 * rng.standard_normal((B, A)) * 256.0) / 256.0, -16.0, 16.0)


def _categorical_inputs(case: Case) -> dict:
    rng = np.random.default_rng(case.seed)
    B, A, D, variant = case.B, case.A, case.D, case.variant
    old = _far_logits(rng, B, A)
    new = _far_logits(rng, B, A)
    masked_old = np.zeros((B, A), bool)
    masked_new = np.zeros((B, A), bool)
    if variant == "close":
        old = 2.0 * rng.standard_normal((B, A))
        new = old + 0.05 * rng.standard_normal((B, A))
    elif variant == "same":
        new = old.copy()
    elif variant in ("masked_both", "masked_old_only"):
        masked_old = rng.random((B, A)) < 0.3
        masked_old[:, 0] = False  # column 0 is always live
        if variant == "masked_both":
            masked_new = masked_old.copy()
    live = ~(masked_old | masked_new)
    # the taken action: uniform among the actions live under both policies (never pinned to column 0)
    score = np.where(live, rng.random((B, A)), -1.0)
    taken = score.argmax(-1)
    if variant == "masked_new_only":  # one entry of row B // 2 (and of row 0): live old logit, -inf new one, not the taken action
        for row in sorted({0, B // 2}):
            masked_new[row, (taken[row] + 1 + rng.integers(A - 1)) % A] = True
    old, new = _f32(old), _f32(new)
    old[masked_old] = -np.inf
    new[masked_new] = -np.inf
    data = {}
    if variant == "shifted":
        data["far"] = (old.copy(), new.copy())
        shift = _f32(np.where(rng.random((B, 1)) < 0.5, -1e4, 1e4))
        old, new = old + shift, new + shift  # exact: multiples of 2^-8 below 2^14
    action = np.zeros((B, A), np.float32)
    action[np.arange(B), taken] = 1.0
    rows = np.arange(B)
    log_p, log_q = _log_softmax(old)[rows, taken], _log_softmax(new)[rows, taken]
    noisy = log_p + 0.3 * rng.standard_normal(B)
    old_logp = _f32(np.clip(noisy, log_q - (LOG_RATIO_LIMIT - 1.0), log_q + (LOG_RATIO_LIMIT - 1.0)))
    data.update(old_logits=old, new_logits=new, action=action, old_logp=old_logp, advantage=_f32(rng.standard_normal((B, D))),
                taken=taken, masked_old=masked_old, masked_new=masked_new)
    return data


def _normal_logp(x, mean, std):
    x, mean, std = (np.asarray(a, np.float64) for a in (x, mean, std))
    return (-((x - mean) ** 2) / (2.0 * std**2) - np.log(std) - 0.5 * np.log(2.0 * np.pi)).sum(-1)


def _gaussian_inputs(case: Case) -> dict:
    rng = np.random.default_rng(case.seed)
    B, A, D, variant = case.B, case.A, case.D, case.variant
    normal = lambda *s: rng.standard_normal(s)  # noqa: E731
    mp, sp = _f32(normal(B, A)), _f32(rng.random((B, A)) + 0.5)
    if variant == "close":  # the recipe of test_policy_stats_vs_oracle: an updated policy within 5 % of the old one
        mq, sq = _f32(mp + 0.05 * normal(B, A)), _f32(sp * np.exp(0.05 * normal(B, A)))
        action = _f32(mp + sp * normal(B, A))
        old_logp = _f32(_normal_logp(action, mp, sp))
    else:
        if variant == "far":
            mq, sq = _f32(mp + 3.0 * normal(B, A)), _f32(sp * np.exp(rng.uniform(-3.0, 3.0, (B, A))))
        elif variant == "same":
            mq, sq = mp.copy(), sp.copy()
        else:  # tiny_std
            sp, sq = _f32(rng.uniform(1e-3, 2e-3, (B, A))), _f32(rng.uniform(1e-3, 2e-3, (B, A)))
            mq = _f32(mp + 1e-3 * normal(B, A))
        action = _f32(mq + sq * normal(B, A))
        old_logp = _f32(_normal_logp(action, mq, sq) + rng.uniform(-3.0, 3.0, B))
    return dict(old_mean=mp, old_std=sp, new_mean=mq, new_std=sq, action=action, old_logp=old_logp,
                advantage=_f32(normal(B, D)))


OPERANDS = {"categorical": ("old_logits", "new_logits", "action", "old_logp", "advantage"),
            "gaussian": ("old_mean", "old_std", "new_mean", "new_std", "action", "old_logp", "advantage")}


def inputs(case: Case) -> dict:
    """Every operand of the case's launch as float32 arrays ([B, A], ``old_logp`` [B], ``advantage`` [B, D]), plus what the
    CPU test checks the input conditions on (``taken``, the masks; ``far``: the unshifted logits of a ``shifted`` case)."""
    return _categorical_inputs(case) if case.family == "categorical" else _gaussian_inputs(case)


def operands(case: Case, data: dict) -> tuple:
    return tuple(data[name] for name in OPERANDS[case.family])


@functools.lru_cache(maxsize=None)
def _reference(case: Case):
    data = inputs(case)
    fn = oracle.categorical_policy_stats if case.family == "categorical" else oracle.policy_stats
    want = fn(*operands(case, data), return_mass=True)
    if case.variant == "shifted":  # ... and the statistics of the unshifted pair
        far = oracle.categorical_policy_stats(*data["far"], *operands(case, data)[2:], return_mass=True)
        return want, far
    return want, None


def reference(case: Case):
    """``((kl, iw, std), (mass_kl, mass_iw, mass_std))`` in float64, computed once per case and shared."""
    return _reference(case)[0]


# ------------------------------------------------------------------------------------------------ fp32 restatement
class F32:
    """Both kernels in numpy float32: every per-row intermediate rounded to fp32 in the kernel's order (no fused
    multiply-add: the library is built with contraction off), the rows then summed in float64 and divided as the finalize does.
    ``run(case, data)`` returns the three float32 outputs."""

    @staticmethod
    def finalize(kl, iw, std, B, A, D):
        sums = [np.asarray(v, np.float64).sum() for v in (kl, iw, std)]
        return np.array([sums[0] / B, sums[1] / (B * D), sums[2] / (B * A)]).astype(np.float32)

    @classmethod
    def run(cls, case: Case, data: dict) -> np.ndarray:
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            return getattr(cls, case.family)(case, *operands(case, data))

    @staticmethod
    def weighted(advantage, weight):
        iw = np.zeros_like(weight)
        for d in range(advantage.shape[1]):
            iw = iw + advantage[:, d] * weight
        return iw

    @classmethod
    def gaussian(cls, case, mp, sp, mq, sq, x, old_logp, advantage):
        f = np.float32
        B, A = mp.shape
        kl, logp, std_sum = np.zeros(B, f), np.zeros(B, f), np.zeros(B, f)
        for a in range(A):
            ratio = sp[:, a] / sq[:, a]
            var_ratio = ratio * ratio
            z = (mp[:, a] - mq[:, a]) / sq[:, a]
            kl = kl + f(0.5) * (var_ratio + z * z - f(1.0) - np.log(var_ratio))
            diff = x[:, a] - mq[:, a]
            logp = logp + (-(diff * diff) / (f(2.0) * (sq[:, a] * sq[:, a])) - np.log(sq[:, a]) - f(0.918938533204672741780329736406))
            std_sum = std_sum + sq[:, a]
        weight = np.exp(logp - old_logp)
        return cls.finalize(kl, cls.weighted(advantage, weight), std_sum, B, A, advantage.shape[1])

    @classmethod
    def categorical(cls, case, zp, zq, action, old_logp, advantage):
        f = np.float32
        B, A = zp.shape
        mp, mq = zp.max(-1), zq.max(-1)
        sp, sq = np.zeros(B, f), np.zeros(B, f)
        for j in range(A):
            sp, sq = sp + np.exp(zp[:, j] - mp), sq + np.exp(zq[:, j] - mq)
        taken = action.argmax(-1)  # first maximum
        log_sp, log_sq = np.log(sp), np.log(sq)
        kl = np.zeros(B, f)
        for j in range(A):
            lp, lq = (zp[:, j] - mp) - log_sp, (zq[:, j] - mq) - log_sq
            pj = np.exp(lp)
            t = pj * (lp - lq)
            t = np.where(np.exp(lq) == f(0.0), f(np.inf), t)
            t = np.where(pj == f(0.0), f(0.0), t)
            kl = kl + t
        rows = np.arange(B)
        weight = np.exp(((zq[rows, taken] - mq) - log_sq) - old_logp)
        return cls.finalize(kl, cls.weighted(advantage, weight), np.zeros(B, f), B, A, advantage.shape[1])


# ------------------------------------------------------------------------------------------------ assertions
STATISTICS = ("kl_divergence", "importance_weighted_advantage", "action_std")


def _bound(case: Case, k: int, mass: float) -> float:
    return WIDENED.get((case.family, case.variant, k), RELATIVE) * mass


def _within(case, k, got, want, mass, what="float64"):
    error, bound = abs(float(got) - want), _bound(case, k, mass)
    print(f"{case.name}:{STATISTICS[k]}: |got - {what}| = {error:.3e}, bound {bound:.3e} ({error / bound if bound else 0.0:.3f} of it)")
    assert np.isfinite(got) and error <= bound, (
        f"{case.name}:{STATISTICS[k]}: {float(got)!r} vs {what} {want!r}: off by {error:.3e} > {bound:.3e} (mass {mass:.3e})")
    return error / bound if bound else 0.0


def check(case: Case, got) -> list[float]:
    """``got``: the three float32 outputs of one launch (or of the restatement).  Returns the achieved error of each
    statistic in units of its bound (0 where the statistic is pinned exactly)."""
    got = np.asarray(got)
    assert got.shape == (3,) and got.dtype == np.float32, (case.name, got.shape, got.dtype)
    (want, mass), far = _reference(case)
    used = [0.0, 0.0, 0.0]
    if case.variant == "same":
        assert got[0] == 0.0, f"{case.name}: the KL of a policy with itself is {got[0]!r}, not 0.0"
    elif case.variant == "masked_new_only":
        assert want[0] == np.inf
        assert got[0] == np.inf, f"{case.name}: the KL is {got[0]!r}, not +inf, with an action only the new policy masks"
    else:
        assert np.isfinite(want[0])
        used[0] = _within(case, 0, got[0], want[0], mass[0])
    used[1] = _within(case, 1, got[1], want[1], mass[1])
    if case.family == "categorical":
        assert got[2] == 0.0 and not np.signbit(got[2]), f"{case.name}: slot 2 is {got[2]!r}, not 0.0"
    elif case.variant == "same":
        np.testing.assert_allclose(got[2], np.float32(want[2]), rtol=1e-6, err_msg=f"{case.name}:action_std")
    else:
        used[2] = _within(case, 2, got[2], want[2], mass[2])
    if far is not None:  # shifted: the statistics of the unshifted pair, to the same bounds
        for k in (0, 1):
            _within(case, k, got[k], far[0][k], far[1][k], "float64 of the unshifted logits")
    return used
