"""Worker for tests/test_reward_normalization_distributed.py: one rank of a world_size-2 gloo job (launched by torchrun).  Each
rank steps ``RewardNormalization`` on its own rewards (host form), merges in ``pre_update``, steps on and merges again."""

import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import torch  # noqa: E402

import cusrl_amd as cusrl  # noqa: E402  (reads RANK / LOCAL_RANK / WORLD_SIZE at import)
from _reward_normalization import inputs, make_hook  # noqa: E402
from cusrl_amd.utils import distributed  # noqa: E402


def main(out_dir: str):
    cusrl.config.set_device("cpu")
    assert distributed.enabled() and distributed.world_size() == 2
    rank = distributed.rank()
    N, R = 5 + 4 * rank, 2  # the ranks hold different numbers of envs: the merge weighs by count
    reward, terminated, truncated = inputs(N, R)
    reward = reward * (1.0 + 9.0 * rank)  # ... and see rewards of different scale
    hook = make_hook(cusrl, N, R)
    result = {"rank": rank, "local": [], "merged": []}
    for round_ in range(2):
        for t in range(3 * round_, 3 * round_ + 3):
            hook.post_step({"reward": torch.from_numpy(reward[t].copy()), "terminated": torch.from_numpy(terminated[t]).unsqueeze(-1),
                            "truncated": torch.from_numpy(truncated[t]).unsqueeze(-1)})
        assert not hook._is_synchronized
        result["local"].append(hook.statistics.stats.tolist())
        hook.pre_update(None)
        assert hook._is_synchronized
        result["merged"].append(hook.statistics.stats.tolist())
    hook.pre_update(None)  # nothing added since: no collective, nothing changes
    assert hook.statistics.stats.tolist() == result["merged"][-1]
    distributed.barrier()
    Path(out_dir, f"rank{rank}.json").write_text(json.dumps(result))


if __name__ == "__main__":
    main(sys.argv[1])
