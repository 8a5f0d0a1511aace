"""Regenerate ``player.npz``: the reference's ``Player`` (cusrl/template/player.py) and ``SaveTransition``
(cusrl/hook/player/save_transition.py) run on the CPU over the scripted environment and agent of tests/_player.py — a fixed
``[T, N, D]`` reward table and ``[T, N]`` terminated / truncated tables (N = 5, D = 2), observation = (step index, env index).

Three runs: ``num_steps = 12``; ``num_episodes = 2``; ``num_episodes = 1`` with ``SaveTransition(save_interval=4)``.  Recorded per
run: the step count at exit, the ``episode_count`` after every step, the three metrics, and for the third run every saved array
under ``run3/<file name>/<key>`` with the file names in ``run3_files``.

    python tests/golden/make_player_golden.py
"""

from __future__ import annotations

import sys
import tempfile
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from make_golden import META, import_reference  # noqa: E402

from _player import make_tables, scripted_classes  # noqa: E402

HERE = Path(__file__).resolve().parent
RUNS = {"run1": dict(num_steps=12), "run2": dict(num_episodes=2), "run3": dict(num_episodes=1)}
METRICS = ("Mean step reward", "Mean episode reward", "Mean episode length")


def main():
    cusrl = import_reference()
    from cusrl.hook.player.save_transition import SaveTransition  # noqa: PLC0415

    Environment, Agent = scripted_classes(cusrl)
    reward, terminated, truncated = make_tables()
    out = dict(META, reward=reward, terminated=terminated, truncated=truncated)

    class Trajectory(cusrl.Player.Hook):
        def __init__(self):
            self.counts = []

        def step(self, step, transition):  # (called before this step's resets are counted: recorded one step late, see close)
            if step:
                self.counts.append(self.player.episode_count.clone().numpy())

        def close(self):
            self.counts.append(self.player.episode_count.clone().numpy())

    for name, limits in RUNS.items():
        with tempfile.TemporaryDirectory() as directory:
            trajectory = Trajectory()
            hooks = [trajectory]
            if name == "run3":
                hooks.append(SaveTransition(Path(directory) / "transition", save_interval=4))
            environment = Environment(reward, terminated, truncated)
            player = cusrl.Player(environment, Agent(environment.spec), hooks=hooks, verbose=False, progress_bar=False, **limits)
            metrics = player.run_playing_loop()
            out[f"{name}_steps"] = np.array(player.step_count)
            out[f"{name}_episode_count"] = np.stack(trajectory.counts)
            for metric in METRICS:
                out[f"{name}_{metric.lower().replace(' ', '_')}"] = np.asarray(metrics[metric], dtype=np.float64)
            if name == "run3":
                files = sorted(path.name for path in Path(directory).iterdir())
                out["run3_files"] = np.array(files)
                for file in files:
                    with np.load(Path(directory) / file) as saved:
                        for key in saved.files:
                            out[f"run3/{file}/{key}"] = saved[key]
    np.savez_compressed(HERE / "player.npz", **out)
    print(f"wrote {HERE / 'player.npz'}: " + ", ".join(f"{name} {int(out[name + '_steps'])} steps" for name in RUNS))


if __name__ == "__main__":
    main()
