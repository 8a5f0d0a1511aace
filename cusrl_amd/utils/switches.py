"""Every ``CUSRL_*`` environment switch of the Python host, declared once and read in one place.

``read("EPOCH_GRAPHS")`` parses ``CUSRL_EPOCH_GRAPHS`` from the live ``os.environ``: nothing is cached here, so WHEN a switch
takes effect is decided by where its caller reads it — ``moment`` records that (``import``: frozen into a module / class
constant; ``construct``: read by a constructor; ``call``: read at every call, capture or plan).  ``declared()`` lists the
declarations; INTEGRATION.md, "Environment switches", has the long prose and the measurements, and tests/test_host_logic.py
holds the two against each other.

Kinds and what ``read`` returns — every parse is as lenient as the read site it replaced::

    on      True unless the text is "0"
    off     False unless the text is "1"
    choice  the text looked up in the mapping declared here; any other text: the mapping's fallback
    int     int(text): the two plain integers raise ValueError on anything else, a launch-shape option (_option) skips it
    path    a file name, as text
    text    the text as it stands

``default`` is what an unset variable means, spelled as INTEGRATION.md prints it: on / off / auto / unset / the number / the text.
"""

from __future__ import annotations

import os
from collections.abc import Callable
from typing import Any, NamedTuple

__all__ = ["Switch", "declared", "read"]


class Switch(NamedTuple):
    name: str
    kind: str
    default: str
    moment: str
    effect: str
    parse: Callable[[str | None], Any]  # (None: the variable is unset)
    mark: str = ""  # "test-only" | "library": read by libcusrl_hip.so, never by the host


def _on(name, moment, effect, mark=""):
    return Switch(name, "on", "on", moment, effect, lambda text: text != "0", mark)


def _off(name, moment, effect, mark=""):
    return Switch(name, "off", "off", moment, effect, lambda text: text == "1", mark)


def _choice(name, default, moment, effect, mapping, fallback):
    return Switch(name, "choice", default, moment, effect, lambda text: mapping.get(text, fallback))


def _int(name, default, moment, effect):
    return Switch(name, "int", str(default), moment, effect, lambda text: default if text is None else int(text))


def _option_int(text):
    try:
        return int(text)
    except (TypeError, ValueError):
        return None


def _option(name, option, mapping=None):
    """A launch-shape / cache-policy override handed to ``cusrl_set_option``: the option's value, or None for "leave the kernel's
    own rule" — which is what an unknown value meant to the library, too, while it still read these itself."""
    return Switch(name, "int" if mapping is None else "choice", "auto", "call", f"cusrl_set_option({option!r}) when the library is loaded",
                  _option_int if mapping is None else lambda text: mapping.get(text))


def _text(name, default, moment, effect, unset=None, kind="text", mark=""):
    return Switch(name, kind, default, moment, effect, lambda text: unset if text is None else text, mark)


def _tuned_gemms(text):
    """False: off; True: the shipped file; else the path of another selection file."""
    return {None: True, "0": False, "1": True}.get(text, text)


SWITCHES: dict[str, Switch] = {switch.name.removeprefix("CUSRL_"): switch for switch in (
    _on("CUSRL_NATIVE_COLLECTIVES", "import", "CONFIG.native_collectives: the C-ABI collectives inside the step graph"),
    _on("CUSRL_CAPTURE_ROLLOUT", "construct", "Trainer: whole env steps of capturable envs replay from hipGraphs"),
    _on("CUSRL_WHOLE_ROLLOUT_GRAPH", "construct", "GraphedRolloutStep: one graph replay per rollout, not per env step"),
    _on("CUSRL_DEFER_LOSS_FINALIZE", "construct", "ActorCritic: captured steps drop the loss kernel's finalize launch"),
    _int("CUSRL_RECORD_THRESHOLD_BYTES", 128 << 20, "construct", "Buffer: smallest sampled size that builds the per-slot record"),
    _choice("CUSRL_CONCURRENT_CRITIC", "auto", "construct", "ActorCritic: force the critic's stream-branch off / on",
            {None: None, "0": False}, True),
    _choice("CUSRL_GRAPH_MEMSETS", "replace", "call", "_Capture.capture: keep the memset nodes of captured regions",
            {"keep": "keep"}, "replace"),
    _int("CUSRL_WIDE_LINEAR_MIN_ROWS", 1, "import", "nn.module: rows from which a linear layer takes the hand-written backward"),
    _off("CUSRL_SPLIT_ALLREDUCE", "import", "CONFIG.split_gradient_allreduce: per-network gradient all-reduce"),
    _text("CUSRL_HIP_LIBRARY", "unset", "import", "_native.LIB_PATH: another build of libcusrl_hip.so", kind="path"),
    _on("CUSRL_PREFETCH_PERMUTATIONS", "construct", "MiniBatchSampler: permutations drawn ahead on a side stream"),
    _on("CUSRL_FUSED_RNN", "call", "nn.gru: recurrent cores as GEMMs + HIP gate passes, not MIOpen"),
    _on("CUSRL_AMP_CLOSED_FORM", "import", "AdversarialMotionPrior.closed_form_objective's default"),
    Switch("CUSRL_TUNED_GEMMS", "path", "on", "import, call", "CONFIG.tuned_gemms (import) and the selection file "
           "enable_tuned_gemms loads (call)", _tuned_gemms),
    _text("CUSRL_CAPTURE_ERROR_MODE", "auto", "call", "_Capture.capture: stream-capture error mode of every capture"),
    _choice("CUSRL_EPOCH_GRAPHS", "update", "construct", "GraphedEpochs: one graph per update / epoch / minibatch step",
            {"0": "off", "1": "epoch", "epoch": "epoch"}, "update"),
    _on("CUSRL_SEPARATE_VALUE_TERM", "construct", "ActorCritic: the value term as its own launch on the critic's branch"),
    _text("CUSRL_PREFETCH_GATHER", "tail", "construct", "GraphedEpochs: where a step's gather is issued (tail / side / else inside)",
          unset="tail"),
    _on("CUSRL_INPUT_LAYER_KERNEL", "import", "nn.module: the bottom layer's backward as one launch"),
    _choice("CUSRL_PIPELINE_LOGS", "on", "construct", "Trainer: an iteration's log written behind the next rollout's launch",
            {"0": "off", "late": "late"}, "on"),
    _on("CUSRL_FUSED_INFERENCE", "import", "nn.module: no-grad passes of Actor / Value as one launch"),
    _on("CUSRL_TWO_WINDOW_STEP", "call", "ActorCritic step plan: per-network gradient assembly + Adam launch, no join"),
    _on("CUSRL_SIDE_STREAM_PROBE", "call", "side_stream: candidates are probed until one runs beside the busy streams"),
    _off("CUSRL_SIDE_STREAM_PRIORITY", "call", "side_stream: the first candidate is a high-priority stream"),
    _on("CUSRL_NORMED_MAIN_FIRST", "call", "FlatAdam: a multi-rank unjoined step captures the main window's launch first"),
    _off("CUSRL_STEP_MAIN_FIRST", "call", "FlatAdam: a single process's unjoined step does so, too"),
    _on("CUSRL_PREDRAW_NOISE", "construct", "GraphedRolloutStep: a rollout's exploration noise drawn ahead of its launch"),
    _on("CUSRL_FUSE_EPILOGUE_PUSH", "construct", "GraphedRolloutStep: step epilogue and buffer append as one launch"),
    _on("CUSRL_FUSED_ENV", "construct", "testing.SyntheticEnvironment: its one-launch Philox step"),
    _option("CUSRL_GAE_POLICY", "gae_policy", {"0": 1, "5": 6, "7": 8}),
    _option("CUSRL_GAE_BLOCK", "gae_block"),
    _option("CUSRL_LOSS_POLICY", "loss_policy", {"0": 1, "1": 2}),
    _option("CUSRL_PUSH_POLICY", "push_policy", {"0": 1, "3": 2}),
    _option("CUSRL_COLSUM_ROWS", "colsum_rows"),
    _option("CUSRL_HEAD_ROWS", "head_rows"),
    _option("CUSRL_GRU_BIAS_ROWS", "gru_bias_rows"),
    _text("CUSRL_RCCL_LIBRARY", "unset", "call", "the RCCL the C-ABI communicator loads", kind="path", mark="library"),
    _text("CUSRL_COMM_FAULT", "unset", "call", "native_comm start-up: inject a failure, <stage>:<rank>", unset="", mark="test-only"),
    _off("CUSRL_HOST_FORMS", "call", "host_form: hooks accept CPU tensors", mark="test-only"),
    _off("CUSRL_SHARE_GPU", "import", "CONFIG.share_gpu: every rank drives cuda:0 over gloo", mark="test-only"),
)}


def read(key: str) -> Any:
    """The parsed value of ``CUSRL_<key>`` as the environment holds it now."""
    switch = SWITCHES[key]
    return switch.parse(os.environ.get(switch.name))


def publish(name: str, value: str) -> None:
    """Leave ``name=value`` in the process environment for whoever is started from here (the one variable the package WRITES
    besides the seed: ``TRIAL_LOG_DIR``, the run directory of a ``Logger`` — cusrl/template/logger.py:94)."""
    os.environ[name] = value


def declared() -> tuple[Switch, ...]:
    return tuple(SWITCHES.values())
