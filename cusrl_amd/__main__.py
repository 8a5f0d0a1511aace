"""``python -m cusrl_amd``: the command-line front end of the experiment zoo (``cusrl_amd.zoo``).

    python -m cusrl_amd list-experiments
    python -m cusrl_amd train --environment CartPole-v1 --algorithm ppo [--num-envs N] [--num-iterations N] [--device D] [--seed S]
                              [--log-dir DIR]
"""

from __future__ import annotations

import argparse
import sys


def _parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(prog="python -m cusrl_amd", description="Train the registered experiments of cusrl_amd.zoo.")
    commands = parser.add_subparsers(dest="command", required=True)
    commands.add_parser("list-experiments", help="print the registered experiments, one per line")
    train = commands.add_parser("train", help="train one registered experiment")
    train.add_argument("--environment", required=True, help="environment name of the experiment, e.g. CartPole-v1")
    train.add_argument("--algorithm", required=True, help="algorithm name of the experiment, e.g. ppo")
    train.add_argument("--num-envs", type=int, default=None, help="number of parallel envs (default: the experiment's)")
    train.add_argument("--num-iterations", type=int, default=None, help="number of iterations (default: the experiment's)")
    train.add_argument("--device", default=None, help="device of the envs and the agent (default: the configured one)")
    train.add_argument("--seed", type=int, default=None, help="global seed (default: drawn)")
    train.add_argument("--log-dir", default=None, help="run directory for checkpoints (default: none are written)")
    return parser


def main(argv: list[str] | None = None) -> int:
    import cusrl_amd
    from cusrl_amd import zoo

    args = _parser().parse_args(argv)
    if args.command == "list-experiments":
        print("\n".join(zoo.list_experiments()))
        return 0
    spec = zoo.get_experiment(args.environment, args.algorithm)
    if args.seed is not None:
        cusrl_amd.set_global_seed(args.seed)
    logger_factory = cusrl_amd.make_logger_factory(None, args.log_dir, name=spec.name)
    trainer = spec.make_trainer(num_envs=args.num_envs, num_iterations=args.num_iterations, device=args.device, seed=args.seed,
                                logger_factory=logger_factory, verbose=True)
    trainer.run_training_loop()
    return 0


if __name__ == "__main__":
    sys.exit(main())
