"""world_size-2 gloo run on CPU of ``RewardNormalization``'s cross-rank merge (after tests/test_distributed_cpu.py): the step is
rank-local, ``pre_update`` — where ``ObservationNormalization(defer_synchronization=True)`` merges — pools what each rank added
since the last merge by count, and both ranks leave it with the same triple."""

import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    out = tmp_path_factory.mktemp("reward_normalization_dist")
    env = dict(os.environ, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), str(ROOT / "tests" / "_reward_normalization_dist_worker.py"), str(out)]
    done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    return [json.loads((out / f"rank{r}.json").read_text()) for r in range(2)]


def _pooled(triples):
    """Count-weighted pooling of per-rank (mean, var, count) rows in float64."""
    means, vars_, counts = (np.array([np.asarray(t)[k] for t in triples]) for k in range(3))
    total = counts.sum(axis=0)
    mean = (means * counts).sum(axis=0) / total
    var = ((vars_ + (means - mean) ** 2) * counts).sum(axis=0) / total
    return mean, var, total


def test_both_ranks_hold_the_same_triple_after_each_merge(ranks):
    for round_ in range(2):
        assert ranks[0]["merged"][round_] == ranks[1]["merged"][round_]
        assert ranks[0]["local"][round_] != ranks[1]["local"][round_]


def test_first_merge_pools_the_ranks_by_count(ranks):
    mean, var, total = _pooled([rank["local"][0] for rank in ranks])
    merged = np.asarray(ranks[0]["merged"][0])
    np.testing.assert_allclose(merged[0], mean, rtol=1e-7)
    np.testing.assert_allclose(merged[1], var, rtol=1e-7)
    np.testing.assert_allclose(merged[2], total, rtol=1e-12)
    assert total[0] == pytest.approx(2e-4 + 3 * (5 + 9))


def test_second_merge_adds_only_what_each_rank_added_since(ranks):
    """The count after the second merge is the first merged count plus both ranks' new rows — the shared part is not counted twice."""
    merged = np.asarray(ranks[0]["merged"][1])
    assert merged[2, 0] == pytest.approx(2e-4 + 6 * (5 + 9), rel=1e-9)
    for rank in ranks:  # each rank went on from the merged triple: its local count is that plus its own rows
        N = 5 + 4 * rank["rank"]
        assert np.asarray(rank["local"][1])[2, 0] == pytest.approx(np.asarray(rank["merged"][0])[2, 0] + 3 * N, rel=1e-12)
    assert np.isfinite(merged).all() and (merged[1] > 0).all()
