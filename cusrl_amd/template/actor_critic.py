"""Actor-critic agent: rollout into the HBM buffer, then minibatch PPO-style updates driven by hooks
(counterpart of cusrl/template/actor_critic.py:23-418; ``export`` writes this package's own policy file, template/export.py —
ONNX and TorchScript output are out of scope).

Differences that matter on MI355X (semantics unchanged):
* ``buffer.push`` is one HIP launch per env step; minibatches come from one gather launch (template/buffer.py);
* gradients live in ONE flat fp32 buffer (``FlatGradients``): ``zero_grad`` is a single memset, the per-step
  data-parallel all-reduce (RCCL over xGMI) needs no pack / unpack copies, and norm clipping is one reduction;
* the loss is ``Objectives.loss()`` — the fused kernel's pre-summed total when the stock PPO hooks are fused,
  otherwise the reference's left-fold ``sum(objectives.values())``.
"""

from __future__ import annotations

from collections.abc import Callable, Iterable, Mapping, Sequence
from contextlib import contextmanager
from dataclasses import dataclass
from typing import Any

import torch

from cusrl_amd.nn.actor import Actor, Value
from cusrl_amd.nn.module import collect_split_weight_grads, register_unit_gradient
from cusrl_amd.template.agent import Agent, AgentFactory, preserve_io_format
from cusrl_amd.template.buffer import Buffer, Sampler
from cusrl_amd.template.environment import EnvironmentSpec
from cusrl_amd.template.hook import Hook, HookComposite
from cusrl_amd.template.optimizer import OptimizerFactory, build_optimizer
from cusrl_amd.utils import switches
from cusrl_amd.utils.config import CONFIG
from cusrl_amd.utils.distributed import FlatGradients, UnjoinedStep, broadcast_parameters, reduce_gradients

__all__ = ["ActorCritic", "ActorCriticFactory", "HookList", "StepContext", "StepPlan", "plan_step"]


def _hashable(value):
    """A metadata value as part of a step-graph key: hashable as it is, else its frozen form, else its repr."""
    from cusrl_amd.template.graphs import _freeze

    try:
        hash(value)
        return value
    except TypeError:
        frozen = _freeze(value)
        try:
            hash(frozen)
            return frozen
        except TypeError:
            return repr(value)


ONE_PASS, JOINED, UNJOINED, SPLIT = "one pass", "joined", "unjoined", "split"


@dataclass(frozen=True)
class StepPlan:
    """How a minibatch step differentiates and steps its parameters (:func:`plan_step`).  ``mode``, for a step whose loss has a
    summand of the critic's own, evaluated on the critic's stream (hook/on_policy/value.py):
    ``ONE_PASS`` — the critic shares parameters: the streams join, one backward over every summand;
    ``JOINED`` — the critic's summand differentiated on its stream, the others' on the main one, met once in front of ONE
    assembly; ``UNJOINED`` — the same, but inside a whole-update graph (``StepContext.unjoined``) each window is assembled
    and stepped (``FlatAdam``) where its backward ran, and the streams do not meet; ``SPLIT`` — a multi-rank job's per-network
    split (``CONFIG.split_gradient_allreduce``): each window averaged as soon as it is assembled, with or without that summand."""

    mode: str
    critic_ids: tuple[int, ...] = ()  # the windows' parameters (indices into FlatGradients.params): the critic's ...
    other_ids: tuple[int, ...] = ()  # ... and everybody else's
    ranges: tuple[tuple[int, int], tuple[int, int]] | None = None  # UNJOINED: element ranges, the others' and the critic's
    reduce_windows: tuple[tuple[int, int], ...] = ()  # SPLIT: element ranges averaged one by one, the critic's first


def _stock_optim(hook: Hook) -> bool:
    """Does ``hook`` leave the gradients alone between the backward and the step?  The stock clipping of the default group
    does: it hands its coefficient to the flat Adam step (``FlatAdam.defer_clip``)."""
    from cusrl_amd.hook.on_policy.gradient_clipping import GradientClipping

    if type(hook).post_optim is not Hook.post_optim:
        return False
    return type(hook).pre_optim is Hook.pre_optim or (isinstance(hook, GradientClipping) and not hook.groups)


def plan_step(critic_ids: Sequence[int] | None, offsets: Sequence[int], size: int, *, multi_rank: bool = False,
              split_allreduce: bool = False, native_comm: bool = False, branch_stream: bool = False, flat_adam: bool = False,
              hooks: Iterable[Hook] = (), two_window: bool = True) -> StepPlan:
    """The :class:`StepPlan` of a flat gradient buffer whose parameters start at element ``offsets`` (``size`` in all).
    ``critic_ids``: the critic's parameters, None when it shares one with the actor or a hook; ``native_comm``: the C-ABI
    communicator; ``branch_stream``: the critic's stream exists (``compile=True``); ``hooks``: the active hooks;
    ``two_window``: the ``CUSRL_TWO_WINDOW_STEP`` switch.

    The split route needs the critic's parameters in one run.  A step may stay unjoined when each network's parameters form
    one run, no hook but the stock clipping comes between backward and step (a ``pre_optim`` could read the window on the
    other stream) and, with several ranks, the all-reduce can be captured where it belongs: ONE collective over the whole
    buffer through the C-ABI communicator, behind both assemblies (``reduce_gradients``)."""
    if not critic_ids:
        return StepPlan(ONE_PASS)
    critic = tuple(critic_ids)
    others = tuple(i for i in range(len(offsets)) if i not in set(critic))

    def spans(ids):  # element ranges of the runs of consecutive parameters in `ids` (alignment padding included)
        runs = []
        for i in ids:
            if runs and i == runs[-1][-1] + 1:
                runs[-1].append(i)
            else:
                runs.append([i])
        return [(offsets[run[0]], offsets[run[-1] + 1] if run[-1] + 1 < len(offsets) else size) for run in runs]

    critic_spans, other_spans = spans(critic), spans(others)
    if multi_rank and split_allreduce and branch_stream and others and len(critic_spans) == 1:
        return StepPlan(SPLIT, critic, others, reduce_windows=tuple(critic_spans + other_spans))
    if (two_window and flat_adam and len(critic_spans) == len(other_spans) == 1
            and not (multi_rank and (split_allreduce or not native_comm)) and all(_stock_optim(hook) for hook in hooks)):
        return StepPlan(UNJOINED, critic, others, ranges=(other_spans[0], critic_spans[0]))
    return StepPlan(JOINED, critic, others)


@dataclass
class StepContext:
    """What the captured step body being issued (template/graphs.py) tells the hooks and ``ActorCritic._backward``.  Every
    field holds its default outside of one; :meth:`set` installs values for the duration of a body."""

    critic_stream: torch.cuda.Stream | None = None  # the critic's forward, value term and backward run there (ValueLoss)
    deferred_loss_owner: Any = None  # the fused objective runs without its finalize launch (ops.DeferredLoss)
    branch_tail: Callable[[], None] | None = None  # issued once, at the tail of the critic's branch (the next step's gather)
    unjoined: list[UnjoinedStep] | None = None  # a step may leave its streams unjoined and files its record here (None: it joins)
    batch_on_branch: bool = False  # the step's rows were gathered on the critic's stream, which need not meet the main one

    @contextmanager
    def set(self, **fields):
        saved = {name: getattr(self, name) for name in fields}
        self.__dict__.update(fields)
        try:
            yield self
        finally:
            self.__dict__.update(saved)


class HookList(list):
    """List of hooks with by-name attribute access (actor_critic.py:23-62)."""

    def to_dict(self):
        return {hook.name: hook for hook in self}

    @classmethod
    def from_dict(cls, data: dict[str, Hook]) -> "HookList":
        return cls(hook.name_(name) for name, hook in data.items())

    def __getattr__(self, name: str) -> Any:
        for hook in self:
            if hook.name == name:
                return hook
        raise AttributeError(f"'{type(self).__name__}' object has no attribute '{name}'")

    @classmethod
    def coerce(cls, data: Any) -> "HookList":
        if isinstance(data, dict):
            return cls.from_dict(data)
        if isinstance(data, (list, tuple)):
            return cls(data)
        raise TypeError(f"Unsupported hooks payload: {type(data)!r}")


@dataclass(kw_only=True)
class ActorCriticFactory(AgentFactory):
    actor_factory: Any
    critic_factory: Any
    optimizer_factory: OptimizerFactory | Mapping[str, OptimizerFactory]
    sampler: Sampler
    hooks: list

    def __post_init__(self):
        self.hooks = HookList.coerce(self.hooks)

    def __call__(self, environment_spec: EnvironmentSpec) -> "ActorCritic":
        return ActorCritic(
            environment_spec=environment_spec, actor_factory=self.actor_factory, critic_factory=self.critic_factory,
            optimizer_factory=self.optimizer_factory, sampler=self.sampler, hooks=self.hooks,
            num_steps_per_update=self.num_steps_per_update, name=self.name, device=self.device, compile=self.compile,
            autocast=self.autocast,
        )

    def register_hook(self, hook: Hook, index: int | None = None, before: str | None = None, after: str | None = None):
        """Insert ``hook`` at ``index``, or relative to a named hook; append by default (``:97-136``)."""
        if (index is not None) + (before is not None) + (after is not None) > 1:
            raise ValueError("Only one of index, before, or after can be specified")
        if before is not None:
            index = self.get_hook_index(before)
        elif after is not None:
            index = self.get_hook_index(after) + 1
        elif index is None:
            index = len(self.hooks)
        self.hooks.insert(index, hook)
        return self

    def get_hook(self, hook_name: str) -> Hook:
        return self.hooks[self.get_hook_index(hook_name)]

    def get_hook_index(self, hook_name: str) -> int:
        for i, hook in enumerate(self.hooks):
            if hook.name == hook_name:
                return i
        raise ValueError(f"No hook named '{hook_name}' is registered")


class ActorCritic(Agent):
    Factory = ActorCriticFactory
    MODULES = ["actor", "critic", "hook"]
    STATEFULS = ["optimizer", "grad_scaler"]

    def __init__(self, environment_spec: EnvironmentSpec, actor_factory, critic_factory, optimizer_factory,
                 sampler: Sampler, hooks: Iterable[Hook], num_steps_per_update: int, name: str = "Agent",
                 device=None, compile: bool | str = False, autocast=False):
        super().__init__(environment_spec, num_steps_per_update, name, device, compile, autocast)
        self.value_dim = environment_spec.reward_dim
        self.buffer_capacity = num_steps_per_update
        self.actor_factory, self.critic_factory, self.optimizer_factory = actor_factory, critic_factory, optimizer_factory
        self.fuse_objective = True
        self._fused_objective = None

        self.hook = HookComposite(hooks)
        self.hook.pre_init(self)
        # (the factories as `pre_init` left them: a hook may have replaced one — SymmetricArchitecture wraps the actor's)
        self.actor: Actor = self.actor_factory(self.observation_dim, self.action_dim)
        action_aware = getattr(self.critic_factory, "action_aware", False)
        self.critic: Value = self.critic_factory(self.state_dim + self.action_dim * action_aware, self.value_dim)
        self.buffer = Buffer(self.buffer_capacity, self.parallelism, device=self.device)
        self.sampler = sampler
        self.grad_scaler = torch.GradScaler(device=self.device.type, enabled=self.grad_scaler_enabled)
        self.actor_memory = None
        self.hook.init()

        if self.device.type == "cuda" and CONFIG.tuned_gemms:
            from cusrl_amd.utils.tuning import enable_tuned_gemms

            enable_tuned_gemms()  # measured rocBLAS / hipBLASLt kernel choice for this workload's GEMM shapes
        self.actor = self.setup_module(self.actor)
        self.critic = self.setup_module(self.critic)
        self.optimizer = build_optimizer(optimizer_factory, self.named_parameters())
        self._graphed_act = None
        self._graphed_steps: dict[tuple, Any] = {}
        self._graphed_epochs = None
        self.step_context = StepContext()
        self._while_waiting = None  # host work to issue while a pre_update hook waits for the device (run_while_waiting)
        self._minibatches_done = None  # event behind the last minibatch step of the previous update (its index rows may be redrawn)
        self._graph_key_reads = 0
        self._graph_budget_warned = False
        self._metadata_reads: set[str] = set()  # metadata keys hooks read inside captured steps (graphs.TrackedMetadata)
        if self.compile:
            # `compile=True` = hipGraph replay of the act step and of every minibatch step (template/graphs.py)
            if self.device.type != "cuda":
                raise RuntimeError("compile=True captures hipGraphs and needs a GPU device")
            if any(not group.get("capturable", False) for group in self.optimizer.param_groups):
                raise ValueError("compile=True needs a graph-capturable optimizer, e.g. Adam(capturable=True, fused=True)")
            from cusrl_amd.template.graphs import GraphedAct

            self._graph_stream = torch.cuda.Stream(device=self.device)
            self._graph_pool = torch.cuda.graph_pool_handle()
            # second branch of the captured minibatch step (critic forward / backward, hook/on_policy/value.py)
            self._branch_stream = torch.cuda.Stream(device=self.device)
            # True / False force it; None (default, the switch unset) = per composition, where it measured faster
            # (GraphedTrainStep._critic_branch)
            self.concurrent_critic = switches.read("CONCURRENT_CRITIC")
            # captured minibatch steps run the fused objective without its one-block finalize launch (ops.DeferredLoss)
            self.defer_loss_finalize = switches.read("DEFER_LOSS_FINALIZE")
            self._graphed_act = GraphedAct(self)
        self.flat_gradients: FlatGradients | None = None
        self._unit_grads: dict[tuple, torch.Tensor] = {}
        # the value term of the stock composition as its own launch + root on the critic's branch of a captured step (A/B switch)
        self._separate_value_term = switches.read("SEPARATE_VALUE_TERM")
        if isinstance(self.optimizer, torch.optim.Optimizer) and not self.grad_scaler_enabled:
            self.flat_gradients = FlatGradients(self.optimizer)
        self.flat_optimizer = None
        if self.flat_gradients is not None and self.device.type == "cuda" and all(
                group.get("fused") for group in self.optimizer.param_groups):
            # a fused Adam / AdamW was asked for: step it as ONE HIP launch over flat buffers (utils/flat_optimizer.py)
            from cusrl_amd.utils.flat_optimizer import FlatAdam

            if FlatAdam.eligible(self.optimizer, self.flat_gradients):
                self.flat_optimizer = FlatAdam(self.optimizer, self.flat_gradients)
                self.flat_optimizer.metrics = self.metrics
        self._set_training_mode(False)
        self.hook.post_init()
        broadcast_parameters(self.parameters())
        self.hook.apply_schedule(0)

    def _save_transition(self, *, _clone: bool = True, **fields):
        """Store non-None fields as device tensors.  ``_clone`` keeps the reference's defensive copy
        (agent.py:257-261) for values that must survive an ``env.step`` before they are pushed (observation, state,
        recurrent memory); values pushed into the buffer right away are stored as they are."""
        device, transition = self.device, self.transition
        for key, value in fields.items():
            if value is None:
                continue
            if not _clone and type(value) is torch.Tensor and value.device == device:
                transition[key] = value  # the common case in the rollout loop: already a tensor where it belongs
                continue
            try:
                self.transition[key] = self.to_nested_tensor(value) if _clone else self._as_nested_tensor(value)
            except Exception as error:
                raise ValueError(f"Failed to convert transition field '{key}' to a tensor") from error

    def _as_nested_tensor(self, value):
        if isinstance(value, (tuple, list)):
            return tuple(self._as_nested_tensor(v) for v in value)
        if isinstance(value, Mapping):
            return {k: self._as_nested_tensor(v) for k, v in value.items()}
        return torch.as_tensor(value, device=self.device)

    @torch.no_grad()
    @preserve_io_format
    def act(self, observation, state=None):
        if self._graphed_act is not None:
            observation_t = torch.as_tensor(observation, device=self.device)
            state_t = None if state is None else torch.as_tensor(state, device=self.device)
            if self._graphed_act.supported(observation_t, state_t):
                return self._graphed_act.run(observation_t, state_t)
        self.transition.clear()
        self._save_transition(observation=observation, state=state)
        self.hook.pre_act(self.transition)
        with self.autocast():
            action_dist, (action, action_logp), next_memory = self.actor.explore(
                self.transition["observation"], memory=self.actor_memory, deterministic=self.deterministic,
                backbone_kwargs={"sequential": False},
            )
        self._save_transition(actor_memory=self.actor_memory)
        self.transition.update(action_dist=action_dist, action=action, action_logp=action_logp)
        self.actor_memory = next_memory
        self.hook.post_act(self.transition)
        return self.transition["action"]

    @torch.no_grad()
    def step(self, next_observation, reward, terminated, truncated, next_state=None, **kwargs) -> bool:
        self._save_transition(_clone=False, next_observation=next_observation, next_state=next_state, reward=reward,
                              terminated=terminated, truncated=truncated, **kwargs)
        transition = self.transition
        if transition["terminated"].dtype != torch.bool:
            raise TypeError("'terminated' must have dtype bool")
        if transition["truncated"].dtype != torch.bool:
            raise TypeError("'truncated' must have dtype bool")
        supplied = kwargs.get("done")  # extension: the trainer's fused step epilogue already formed terminated | truncated
        if not (type(supplied) is torch.Tensor and supplied.dtype == torch.bool and supplied.shape == transition["terminated"].shape
                and supplied.device == transition["terminated"].device):
            transition["done"] = transition["terminated"] | transition["truncated"]
        self.hook.post_step(transition)
        if not self.inference_mode:
            self.buffer.push(transition)  # a1: every leaf of the transition in one HIP launch
        self.actor.reset_memory(self.actor_memory, transition["done"])
        ready = super().step(next_observation, reward, terminated, truncated, next_state, **kwargs)
        return ready and self.hook.should_update(transition)

    def replay_step(self) -> bool:
        """Host half of :meth:`step` for an env step whose device work was replayed from a hipGraph
        (template/graphs.py GraphedRolloutStep): hooks' host effects, buffer cursor, update cadence."""
        self.hook.on_replay("step")
        if not self.inference_mode:
            self.buffer.replay_push()
        ready = Agent.step(self, None, None, None, None)
        return ready and self.hook.should_update(self.transition)

    def _steps_draw_random(self) -> bool:
        """Does anything between two permutation draws consume torch's generator (a hook's objective, a dropout layer)?"""
        if any(hook.active and hook.objective_draws_random for hook in self.hook):
            return True
        modules = [self.actor, self.critic] + [m for hook in self.hook for m in hook._modules.values() if m is not None]
        return any(isinstance(layer, torch.nn.modules.dropout._DropoutNd) and layer.p > 0
                   for module in modules for layer in module.modules())

    def _check_sampler_prefetch(self):
        if hasattr(self.sampler, "prefetch") and getattr(self, "_sampler_prefetch_checked", None) is not self.sampler:
            self._sampler_prefetch_checked = self.sampler
            if self._steps_draw_random():
                self.sampler.prefetch = False  # keep the reference's interleaving of permutation and in-step draws

    def update(self):
        self._check_sampler_prefetch()
        # The first epoch's permutation depends on nothing pre_update computes: drawn NOW (side stream), it runs under
        # pre_update's kernels instead of between them and the first minibatch step.  Only when no hook this package does not
        # know could draw from the generator inside pre_update (the reference draws the permutation behind it,
        # cusrl/sampler/mini_batch_sampler.py:56): none of this package's hooks does.
        early = self._draw_epochs(prepare=False) if self._draws_early() else None
        if early is not None:
            from cusrl_amd.template.graphs import epoch_graphs_mode

            if epoch_graphs_mode() == "update":
                # the whole-update graph needs EVERY epoch's permutation before it starts: the remaining draws are issued while
                # the host has nothing to do — ValueComputation.pre_update waits for the truncated count of a region it has
                # just launched (`run_while_waiting`) — and run under that region on the side stream
                def while_waiting():
                    early.draw(len(early) - 1)
                    if self._graphed_epochs is not None:  # ... and the host half of the update graph's launch (GraphedEpochs.prepare)
                        self._graphed_epochs.prepare(early)

                self._while_waiting = while_waiting
        try:
            self.hook.pre_update(self.buffer)  # a3-a6: next_value, GAE, advantage normalisation
        finally:
            self._while_waiting = None
        with self._training_mode():
            # (recurrent networks: dynamic sequence counts, not capturable; a hook's collective / host read-back stays out of capture)
            graphed = self._graphable()
            if graphed:
                from cusrl_amd.template.graphs import GraphedTrainStep

                # every epoch's permutation drawn up front on the draw-ahead stream (same generator calls, same order):
                # once every step replays from its own graph, a whole epoch's steps replay from ONE graph that reads its
                # index slices in place and gathers each step's rows while the step before it runs (template/graphs.py
                # GraphedEpochs); until then — and whenever a condition does not hold — the steps run graph by graph over
                # the very same permutations
                from cusrl_amd.template.graphs import GraphedEpochs

                drawn = early if early is not None else self._draw_epochs()
                if drawn is not None and self._graphed_epochs is None:
                    self._graphed_epochs = GraphedEpochs(self)
                steps = () if drawn is not None and self._graphed_epochs.run(drawn) else (
                    self._iter_drawn(drawn) if drawn is not None else self.sampler.iter_indices(self.buffer))
                for metadata, indices in steps:
                    key = self._step_key(metadata, indices.numel())
                    if (step := self._graphed_steps.get(key)) is None:
                        if self._graph_key_reads != len(self._metadata_reads):
                            # the set of metadata keys hooks read has grown: graphs keyed on the shorter signature can
                            # never be looked up again — release them (and their static buffers)
                            self._graph_key_reads = len(self._metadata_reads)
                            width = len(key)
                            for stale in [k for k in self._graphed_steps if len(k) != width]:
                                self._graphed_steps.pop(stale).flush_metrics()
                        step = self._graphed_steps[key] = GraphedTrainStep(self, key[0], key[1])
                        budget = self.sampler.num_epochs * (self.sampler.num_mini_batches if isinstance(self.sampler.num_mini_batches, int)
                                                            else max(self.sampler.num_mini_batches)) if hasattr(self.sampler, "num_epochs") else 0
                        if budget and len(self._graphed_steps) > budget and not self._graph_budget_warned:
                            self._graph_budget_warned = True
                            self.warn(f"{len(self._graphed_steps)} minibatch-step graphs for {budget} steps per update: a hook reads "
                                      f"metadata whose values keep changing ({sorted(self._metadata_reads)}); every distinct value is "
                                      "its own capture")
                    step.run(metadata, indices)
                if drawn is not None:
                    if self._minibatches_done is None:
                        self._minibatches_done = torch.cuda.Event()
                    self._minibatches_done.record(torch.cuda.current_stream())
                # what the replays accumulated on the device (metric taps, loss sums): handed to the metrics, read in ONE host
                # copy together with everything else this update recorded (Agent.update -> Metrics.summary)
                for step in self._graphed_steps.values():
                    step.flush_metrics()
                if self._graphed_epochs is not None:
                    self._graphed_epochs.flush_metrics()
            else:
                for metadata, batch in self.sampler(self.buffer):  # a7/a8
                    self._train_step(metadata, batch)
        self.hook.post_update()
        self.hook.apply_schedule(self.iteration + 1)
        return super().update()

    def run_while_waiting(self) -> None:
        """Called by a hook right before it blocks on a device result it has just launched the work for: host work that depends
        on neither (here: drawing the later epochs' permutations) is issued now instead of behind the wait."""
        pending, self._while_waiting = self._while_waiting, None
        if pending is not None:
            pending()

    def _graphable(self) -> bool:
        """Does this update's minibatch loop go through captured steps (``compile=True``, an index-yielding sampler, feed-forward
        networks, no hook that keeps its objective phase out of capture)?"""
        if not (self.compile and hasattr(self.sampler, "iter_indices")) or self.actor.is_recurrent or self.critic.is_recurrent:
            return False
        from cusrl_amd.template.graphs import eager_phases

        return "objective" not in eager_phases(self)

    def _draws_early(self) -> bool:
        return self._graphable() and all(type(hook).__module__.startswith("cusrl_amd.") for hook in self.hook if hook.active)

    def _draw_epochs(self, prepare: bool = True):
        """The sampler's up-front permutations (``DrawnEpochs``) when whole-epoch graphs are on and the sampler offers them."""
        from cusrl_amd.template.graphs import epoch_graphs_enabled

        if not (epoch_graphs_enabled() and hasattr(self.sampler, "draw_epochs")):
            return None
        # (the draw only has to wait for the previous update's readers of the index rows — not for whatever the main stream has
        # been given since)
        return self.sampler.draw_epochs(self.buffer, after=self._minibatches_done, prepare=prepare)

    def _step_key(self, metadata, numel: int) -> tuple:
        """Key of the captured minibatch step that serves ``metadata``: slot, sampling form, batch size and the value of every
        metadata key a hook ever read (steps whose values differ are different captures)."""
        key = (metadata["mini_batch_index"], metadata["temporal"], numel)
        if self._metadata_reads:
            key += tuple((name, _hashable(metadata.get(name))) for name in sorted(self._metadata_reads)
                         if name not in ("mini_batch_index", "temporal"))
        return key

    @staticmethod
    def _iter_drawn(drawn):
        """``(metadata, index slice)`` of every minibatch of permutations drawn by ``sampler.draw_epochs`` — each epoch after
        its permutation's event."""
        for epoch, row in enumerate(drawn.plan):
            drawn.wait(epoch)
            for metadata, lo, hi in row:
                yield dict(metadata), drawn.permutations[epoch, lo:hi]

    def _zero_grad(self):
        if self.flat_optimizer is not None:
            self.flat_optimizer.discard_pending_clip()  # a clip deferred for a step that never ran must not leak into this one
        if self.flat_gradients is None:
            self.optimizer.zero_grad()
        elif not self.flat_gradients.intact():
            self.flat_gradients.attach()

    def _backward(self, loss):
        """Gradients of ``loss`` into ``p.grad``.  With the flat gradient buffer the per-parameter gradients — and the
        unsummed slabs of the split-batch weight-gradient GEMMs — are written into it by ONE kernel (no memset, no 13
        accumulate launches, no per-layer sum(0)); otherwise this is the
        reference's ``scaled_loss.backward()`` (actor_critic.py:311-312).  The form of the step: :func:`plan_step`."""
        flat = self.flat_gradients
        roots = list(loss) if isinstance(loss, (list, tuple)) else [loss]  # several roots = the summands of the loss
        if len(roots) > 1:  # a constant summand (a hook returning a plain number) changes no gradient
            roots = [t for t in roots if isinstance(t, torch.Tensor) and t.requires_grad] or roots[:1]
        if flat is None:
            total = roots[0]
            for term in roots[1:]:
                total = total + term
            self.grad_scaler.scale(total).backward()
            return

        def differentiate(roots, units, ids, retain=False):
            with collect_split_weight_grads() as slabs:
                grads = torch.autograd.grad(roots, [flat.params[i] for i in ids], grad_outputs=units, allow_unused=True,
                                            retain_graph=retain)
            return grads, slabs

        units = [self._unit_gradient(term) for term in roots]
        plan = self.step_plan()
        # a summand evaluated on the critic's stream (hook/on_policy/value.py: the value term of the stock composition)
        branch_root = getattr(loss, "branch", None)
        if branch_root is not None and (plan.mode == ONE_PASS or len(roots) != len(loss)):
            # not differentiable network by network (shared parameters, or a summand was dropped above): join first
            torch.cuda.current_stream().wait_stream(branch_root[1])
            branch_root = None
        if branch_root is None and plan.mode != SPLIT:
            flat.assemble(*differentiate(roots, units, range(len(flat.params))))
            return
        # The critic's backward on the branch stream, the others' on the main stream, both issued from here back to back: neither
        # waits for the other (the engine would order a one-pass backward behind the stream this call is made from).  Same
        # autograd nodes, kernels and operands as the one-pass backward; a loss node both passes share is evaluated by both.
        # The streams meet once, in front of ONE assembly (JOINED); or not at all, each window assembled and then stepped where
        # its backward ran (UNJOINED, FlatAdam.step); or each window is averaged over the ranks as soon as it is assembled, the
        # critic's through the second communicator on the branch stream (SPLIT; cusrl/utils/distributed.py:145-172 reduces
        # once, behind the whole backward).
        from cusrl_amd.utils import distributed
        from cusrl_amd.utils.config import configure_distributed

        main, branch, context = torch.cuda.current_stream(), self._branch_stream, self.step_context
        split = plan.mode == SPLIT
        unjoined = plan.mode == UNJOINED and context.unjoined is not None
        multi_rank = configure_distributed()
        want_sumsq = unjoined and not multi_rank  # (several ranks: the step launches measure the averaged norm themselves)
        critic_roots, critic_units, other_roots, other_units = roots, units, roots, units
        if branch_root is not None:  # the value term is a root of its own (evaluated on `branch`): each pass takes its summands
            position = next(i for i, term in enumerate(roots) if term is branch_root[0])
            critic_roots, critic_units = [roots[position]], [units[position]]
            other_roots = [term for i, term in enumerate(roots) if i != position]
            other_units = [unit for i, unit in enumerate(units) if i != position]
        # (else — the split route — the critic's pass runs where its autograd nodes run: gradients are consumed on the stream
        # whose allocator pool they came from)
        on_branch = branch_root is not None or context.critic_stream is branch
        flat.absent = []
        if split and on_branch:
            branch.wait_stream(main)
        with torch.cuda.stream(branch if on_branch else main):
            critic_grads, critic_slabs = differentiate(critic_roots, critic_units, plan.critic_ids, retain=branch_root is None)
            if not split:
                # the critic's branch ends before the actor's: work that depends on neither — the gather of the NEXT minibatch
                # step's rows (template/graphs.py GraphedEpochs) — rides at its tail
                tail, context.branch_tail = context.branch_tail, None
                if tail is not None:
                    tail()
            if split or unjoined:
                branch_sumsq = flat.assemble(critic_grads, critic_slabs, subset=plan.critic_ids, want_sumsq=want_sumsq)
            if unjoined:
                branch_assembled = torch.cuda.Event()
                branch_assembled.record(branch)
        if split:
            # two collectives in flight on two streams need two communicators: without the second one (it could not be created,
            # or the route is torch.distributed's, which cannot be captured) the critic's window is averaged on the MAIN stream
            # behind the join below — one communicator is only ever used from one stream at a time
            inline = not torch.cuda.is_current_stream_capturing() or distributed.native_comm() is not None
            on_branch_comm = inline and distributed.branch_comm() is not None
            windows = tuple(flat.buffer[lo:hi] for lo, hi in plan.reduce_windows)
            if not on_branch:
                branch.wait_stream(main)
            if on_branch_comm:
                with torch.cuda.stream(branch):
                    distributed.branch_comm().allreduce_mean_(windows[0])
        other_grads, other_slabs = differentiate(other_roots, other_units, plan.other_ids)
        if not (split or unjoined):
            main.wait_stream(branch)  # the step's one join
            grads: list = [None] * len(flat.params)
            for i, grad in zip(plan.critic_ids + plan.other_ids, critic_grads + other_grads):
                grads[i] = grad
            other_slabs.update(critic_slabs)
            flat.assemble(grads, other_slabs)
            return
        main_sumsq = flat.assemble(other_grads, other_slabs, subset=plan.other_ids, want_sumsq=want_sumsq)
        if unjoined:
            main_assembled = torch.cuda.Event()
            main_assembled.record(main)
            main_range, branch_range = plan.ranges
            sumsq = (main_sumsq, branch_sumsq) if main_range < branch_range else (branch_sumsq, main_sumsq)  # parameter order
            flat.unjoined = UnjoinedStep(branch, branch_assembled, main_assembled, main_range, branch_range, sumsq, multi_rank)
            context.unjoined.append(flat.unjoined)
            return
        if inline:
            for window in windows[1:]:
                distributed.reduce_mean_(window)
        main.wait_stream(branch)
        if inline and not on_branch_comm:
            distributed.reduce_mean_(windows[0])
        flat.unaveraged_windows = () if inline else windows

    def _unit_gradient(self, term: torch.Tensor) -> torch.Tensor:
        """The persistent, registered ones-scalar of ``term``'s dtype and device (no ones_like per step; custom backwards
        recognise a registered scalar by identity, nn/module.py) — one per (dtype, device), for every root of a step."""
        key = (term.dtype, term.device)
        unit = self._unit_grads.get(key)
        if unit is None:
            unit = self._unit_grads[key] = register_unit_gradient(torch.ones((), dtype=term.dtype, device=term.device))
        return unit

    def step_plan(self) -> StepPlan:
        """:func:`plan_step` for this agent as it stands: computed again at every backward (and capture), so that a hook
        activated since, a changed clipping group or a changed collective route selects its form."""
        from cusrl_amd.utils import distributed
        from cusrl_amd.utils.config import CONFIG, configure_distributed

        flat = self.flat_gradients
        if flat is None:
            return StepPlan(ONE_PASS)
        critic = {id(p) for p in self.critic.parameters()}
        outside = {id(p) for p in self.actor.parameters()} | {id(p) for p in self.hook.parameters()}
        multi_rank = configure_distributed()
        return plan_step(
            None if critic & outside else [i for i, p in enumerate(flat.params) if id(p) in critic], flat.offsets,
            flat.buffer.numel(), multi_rank=multi_rank, split_allreduce=CONFIG.split_gradient_allreduce,
            native_comm=multi_rank and distributed.native_comm() is not None,
            branch_stream=getattr(self, "_branch_stream", None) is not None, flat_adam=self.flat_optimizer is not None,
            hooks=[hook for hook in self.hook if hook._active], two_window=switches.read("TWO_WINDOW_STEP"))

    @property
    def _split_plan(self) -> bool:
        """Does the per-network split of the backward apply (read by bench.py and the distributed tests)?"""
        return self.step_plan().mode == SPLIT

    @property
    def separate_value_root(self) -> bool:
        """May ``ValueLoss`` evaluate its term by its own launch on the critic's stream (a root of its own in ``_backward``)?"""
        return self._separate_value_term and self.step_plan().mode != ONE_PASS

    def _train_step(self, metadata: dict[str, Any], batch: dict[str, Any]):
        self.actor.clear_intermediate_repr()
        self.critic.clear_intermediate_repr()
        self.hook.pre_objective(metadata, batch)
        with self.autocast():
            objectives = self.hook.objective(metadata, batch)  # a9-a13
        if objectives is not None:
            # with the flat gradient buffer the summands are differentiated as separate roots (no additions launched)
            if hasattr(objectives, "terms") and self.flat_gradients is not None:
                loss = objectives.terms()
            else:
                loss = objectives.loss() if hasattr(objectives, "loss") else sum(objectives.values())
            self._zero_grad()
            self._backward(loss)
            self.grad_scaler.unscale_(self.optimizer)
            reduce_gradients(self.optimizer, self.flat_gradients)  # a14
            self.hook.pre_optim(self.optimizer)
            self.grad_scaler.step(self.optimizer)
            self.grad_scaler.update()
            self.hook.post_optim()
            self.record(**objectives)
        self.hook.post_objective(metadata, batch)

    def load_state_dict(self, state_dict: dict[str, Any]):
        super().load_state_dict(state_dict)
        if self.flat_optimizer is not None:  # torch swapped the optimizer's state tensors: fold them back in
            self.flat_optimizer.adopt_state()

    def set_iteration(self, iteration: int):
        if iteration != self.iteration:
            super().set_iteration(iteration)
            self.hook.apply_schedule(self.iteration)

    def resize_buffer(self, capacity: int):
        if self.buffer_capacity != capacity:
            self.buffer_capacity = capacity
            self.buffer.resize(capacity)

    def export(self, output_dir, name: str = "policy", *, with_environment_normalization: bool = True, action_clip=None) -> str:
        """Write the actor as a self-contained policy file ``<output_dir>/<name>.pt`` (actor_critic.py:332-418; format
        ``"cusrl_amd.policy"``, template/export.py) and return its path.  ``nn.DeployedPolicy.load`` runs it:
        ``action = policy(observation)``, ``policy.reset(done)``.  The file carries what the hooks do to an observation at
        deployment (``Hook.export_stages``, in hook order), the actor's backbone and mean head — the action is deterministic —
        and, with ``with_environment_normalization``, the spec's ``action_denormalization``; ``action_clip``: ``(lo, hi)``,
        scalars or one value per action.  An agent the stage set cannot express raises ``ValueError`` naming what was found."""
        from cusrl_amd.template.export import export_policy

        return export_policy(self, output_dir, name, with_environment_normalization=with_environment_normalization,
                             action_clip=action_clip)
