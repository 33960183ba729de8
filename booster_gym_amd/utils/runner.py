"""PPO driver (reference utils/runner.py:19-245, class `Runner`).

Same surface: `Runner(test=False)` parses the reference's 8 CLI flags (runner.py:44-54), merges them over
`envs/<task>.yaml` (:57-68), seeds (:70-80), builds env / model / Adam / buffers (:27-42), `_load` (:82-97),
`train()` (:99-215) and `play()` (:217-241).  What changed is how an iteration executes:

  rollout   per env-step: ONE fused actor+sample launch (bg_actor_sample) and ONE env launch (bg_env_step_to) that writes obs / privileged obs /
            reward / done / time-out directly into rows of the experience buffer -- no `.to(device)` copies, no per-done-env `.item()`
            (runner.py:112-121).  Beside them, on the side stream, the FIRST mini-epoch's forward passes of both networks on each step's rows as soon
            as they exist (same kernels, same weights as the update: bit-identical).
  update    per mini-epoch EIGHT launches on one stream (BG_ONE_STREAM=0: the two networks' chains as separate launches on two streams), no host sync
            inside the 20 mini-epochs (reference: 4 per mini-epoch, runner.py:175,182-184):
              forward        the three hidden layers of BOTH networks as ONE launch that shares the chip by CUs (utils/model.py MLPTrainer ->
                             bg_mlp_chain_forward_split: fp32 operands as exact three-way bf16 splits, all 9 products on the bf16 matrix pipe, fp32
                             accumulation; BG_CHAIN_SPLIT=0: the fp32-MFMA chain bg_mlp_chain_forward_group), the critic's values from the registers
                             of that launch;
              GAE            bg_critic_values_gae: time-out bootstrap, GAE scan, returns, advantage moments in one launch;
              heads + loss   output layers fused with the PPO loss and its backward (bg_critic_head_backward, bg_actor_head);
              backward-data  the hidden layers of both networks as ONE launch (bg_mlp_chain_backward_split: same arithmetic, ELU' and bias-gradient
                             sums in its epilogues; BG_CHAIN_SPLIT_BWD=0: one fp32-MFMA launch per layer);
              weight grads   all six hidden layers of both networks in one grouped launch, the same bf16-pipe arithmetic
                             (bg_mlp_weight_grad_group_split_partial; BG_WGRAD_SPLIT=0: the fp32-MFMA launch bg_mlp_weight_grad_group_partial);
              tail           two launches (bg_update_tail): the deferred fixed-order sums + the squared-norm pieces, then clip + Adam + KL learning-rate
                             rule + statistics bookkeeping + the copies of the weights the layer kernels read (bf16 planes of W, -W, W^T, -W^T).
            Whether a weight copy is current is the trainers' own record (model.WeightCopies) against ONE clock of the parameters that this runner ticks at
            every optimiser step, in invalidate() and at the start of an update() that does not start from the rollout's passes; the tail stamps what it wrote.
            The sequence is written once, on the rows of a StepRows (the whole batch, or one of runner.num_mini_batches' K-ths of it): Runner.update ->
            _whole_batch_values, then per optimiser step _step and _epoch_gradients_and_step; _epoch_on_two_streams places the same pieces on two streams.
  estimator estimator.enabled (utils/estimator.py; off by default): a third network regresses chosen privileged columns from the observations and the actor
            takes [observations | estimates].  The rollout's launch is then bg_actor_sample_est (both networks, the estimates kept in the buffer
            `estimates`), the update builds the actor's input from the stored rows, and behind the last PPO step the estimator takes its own
            supervised Adam steps (estimator.EstimatorTrainer: distillation's kernels, an optimiser and a WeightClock of its own).  No forward-ahead then.
  curiosity rnd.enabled (utils/rnd.py; off by default): random network distillation.  Behind every env step of the rollout ONE more launch
            (bg_rnd_reward) runs a fixed random target network and a trained predictor on the state the step has just written, keeps the target's
            embedding and the raw intrinsic reward in the buffer (`rnd_targets`, `intrinsic_rewards`) and adds weight / sigma x it to the step's reward
            in place; behind the last PPO step the predictor takes its own supervised Adam steps and the reward normaliser moves (rnd.RndTrainer: an
            optimiser and a WeightClock of its own).  The forward-ahead stays on: it never reads rewards.
  recurrent algorithm.rnn_hidden_size (off by default): a GRU cell in front of the actor's hidden layers.  The rollout's launch is then bg_actor_sample_gru
            on a state [N][H] carried over steps and iterations and zeroed where an env reset; the update runs the cell over the iteration's T steps
            from the state stored at the rollout's start (model.GRUTrainer: back-propagation through time, truncated there) around the trunk's
            per-layer kernels, its bias gradients as one launch (bg_gru_bias_partial) among the deferred reductions, the tail as separate launches.
            runner.num_env_mini_batches = K (off by default): K optimiser steps per mini-epoch, step k on the whole sequences of N / K envs of a fresh
            env permutation, laid out by ONE launch (bg_gather_sequences) with their rows of h0 and of the reset flags; a StepRows carries the cell
            trainer of its rows (CellRows).
  smoothness algorithm.smoothness_loss (off by default): the action-smoothness loss, a second source of partner rows for the symmetry loss's 2B-row actor
            path: rows [B, 2B) of the actor's input are every row's successor (bg_partner_rows: cut where GAE cuts, optionally interpolated with a
            fresh draw per row and mini-epoch), the output layer runs as bg_actor_head_sym on the identity action map.  No forward-ahead then.
  multi-GPU one process per GPU (torchrun), environments sharded; per mini-epoch one float64 moments all-reduce on the side stream and ONE grouped RCCL
            launch on the main stream (gradient bucket mean, loss / KL sums, log-std gradient mean) through an own communicator (utils/rccl.py) --
            SURVEY section 8e; the enqueue-order contract of the two communicators is written in utils/parallel.py.

Reference quirks kept on purpose: GAE recomputed from the current critic every mini-epoch (Q5), the
time-out reward overwrite repeated in place (Q4), KL measured with the pre-step distribution (Q6), entropy_coef < 0 (Q7).
"""
import argparse
import glob
import os
import random
import time

import types
from typing import NamedTuple, Optional

import numpy as np
import torch

from .. import _lib
from ..envs import TASKS
from .buffer import ExperienceBuffer
from .estimator import EST_WIDTH, EstimatorTrainer, check_estimator_checkpoint, estimator_cfg, estimator_enabled
from .config import load_cfg
from .obs_norm import ObsNormalizer, check_checkpoint, normalization_cfg
from .model import (ACTOR_HIDDEN, CRITIC_HIDDEN, ActorCritic, GroupedWeightGrad, GRUTrainer, MLPTrainer, NetPlan, WeightClock, check_hidden, hidden_of, pad_input,
                    plan_network, wgrad_products)
from .optim import FlatAdam
from .parallel import DataParallel
from .recorder import Recorder
from .rnd import RND_WIDTH, RndTrainer, check_rnd_checkpoint, module_seed, rnd_cfg
from .value_norm import KEY as VALUE_NORM_KEY, ValueNormalizer, check_checkpoint as check_value_checkpoint, normalize_value_of
from .utils import (actor_head_forward, actor_head_loss_backward, actor_head_sym_loss_backward, critic_head_backward, critic_head_forward, critic_values_gae,
                    critic_values_gae_norm, gae,
                    gaussian_logp, head_scratch, mirror_rows, partner_rows, reduce_group, ppo_loss_fused)


def plan_chain_split(slabs_c, slabs_a, cost_c, cost_a, cus, xcds=8):
    """How many of the `cus` one-per-CU persistent workgroups each of the two forward launches of a mini-epoch gets (Runner._plan_chain_split): the
    split that minimises the longer of the two launches, a launch costing ceil(slabs / workgroups) x its slab cost.
    Both counts are multiples of the number of XCDs (8 on MI355X: 32 CUs each).  The hardware deals the workgroups of a launch round-robin over the
    XCDs, so a count that is not a multiple puts one workgroup more on some XCDs; when both launches do that on the same XCD it holds 33 one-per-CU
    workgroups for 32 CUs and the 33rd runs its slabs after a whole persistent workgroup has retired: the launch takes twice as long.  (Seen at
    16,384 envs with 165 + 91: the critic's launch 2,464 us instead of 1,344, 111 ms per iteration instead of 86, in two of three runners built in
    one process -- which XCDs get the extra workgroups depends on the launches before; tools/probe/two_runners.py, HISTORY.md round 5.)"""
    step = xcds if xcds > 0 and cus % xcds == 0 and cus >= 2 * xcds else 1
    best = min(range(step, cus, step), key=lambda a: (max(-(-slabs_c // a) * cost_c, -(-slabs_a // (cus - a)) * cost_a),
                                                       abs(a - cus * slabs_c * cost_c / (slabs_c * cost_c + slabs_a * cost_a))))
    return best, cus - best


def hidden_widths(cfg):
    """(actor, critic) hidden widths of a config: algorithm.actor_hidden / algorithm.critic_hidden (default: the reference's), checked against the
    supported set and against the split-bf16 GEMMs if parallel.gemm_split or BG_GEMM_SPLIT selects them (model.check_hidden: ValueError)."""
    alg = cfg.get("algorithm", {}) or {}
    split = int((cfg.get("parallel", {}) or {}).get("gemm_split", 0) or 0) or MLPTrainer.SPLIT
    return check_hidden(alg.get("actor_hidden", ACTOR_HIDDEN), alg.get("critic_hidden", CRITIC_HIDDEN), split)


def actor_memory_of(cfg):
    """algorithm.actor_memory as the width H of the GRU cell in front of the actor: 0 (absent: the shipped yaml does not list it) = none.  Set by a
    recurrent distilled student's checkpoint on re-entry (distill.student_overrides).  Pure.  ValueError naming the key for any other value than 0,
    128 or 256, and with estimator.enabled."""
    H = (cfg.get("algorithm", {}) or {}).get("actor_memory", 0) or 0
    if isinstance(H, bool) or not isinstance(H, int) or H not in (0, 128, 256):
        raise ValueError(f"algorithm.actor_memory must be 0, 128 or 256 (the width of a recurrent student's GRU cell, distillation.student_memory), got {H!r}")
    if H and estimator_enabled(cfg):
        raise ValueError(f"algorithm.actor_memory = {H} is not supported with estimator.enabled: true")
    return H


RNN_WIDTHS = (128, 256)  # the widths of the GRU cell that the rollout's and the update's kernels take


def rnn_hidden_size_of(cfg, world_size=1):
    """algorithm.rnn_hidden_size (legged_gym's name; an addition of this build) as the width H of the GRU cell in front of an actor that PPO trains:
    0 (absent: the shipped yaml does not list it) = a feed-forward actor.  Pure.  ValueError naming the key for any other value than 0, 128 or 256, for
    an algorithm.rnn_type other than "gru" (the one cell there is), for an algorithm.actor_memory of another width, and, naming both keys, with every
    option a recurrent actor does not compose with: estimator.enabled, env.frame_stack above 1, terrain.actor_heights, algorithm.symmetry_loss,
    algorithm.empirical_normalization, runner.num_mini_batches above 1, more than one rank."""
    alg = cfg.get("algorithm", {}) or {}
    H = alg.get("rnn_hidden_size", 0)
    H = 0 if H is None else H
    if isinstance(H, bool) or not isinstance(H, int) or H not in (0,) + RNN_WIDTHS:
        raise ValueError(f"algorithm.rnn_hidden_size must be 0, 128 or 256 (the width of the GRU cell in front of the actor; 0 or absent: none), got {H!r}")
    kind = alg.get("rnn_type")
    if kind is not None and kind != "gru":
        raise ValueError(f"algorithm.rnn_type = {kind!r}: the cell of algorithm.rnn_hidden_size is a GRU; the key, if present, must be \"gru\"")
    if not H:
        return 0
    mem = alg.get("actor_memory", 0) or 0
    if mem and mem != H:
        raise ValueError(f"algorithm.rnn_hidden_size = {H} and algorithm.actor_memory = {mem!r} name two widths of one cell: set them equal, or one of them only")
    K = (cfg.get("runner", {}) or {}).get("num_mini_batches", 1) or 1
    refused = (("estimator.enabled: true", estimator_enabled(cfg)),
               ("env.frame_stack above 1", int((cfg.get("env", {}) or {}).get("frame_stack", 1) or 1) > 1),
               ("terrain.actor_heights: true", bool((cfg.get("terrain", {}) or {}).get("actor_heights", False))),
               ("algorithm.symmetry_loss: true", bool(alg.get("symmetry_loss", False))),
               ("algorithm.empirical_normalization: true", bool(alg.get("empirical_normalization", False))),
               ("runner.num_mini_batches above 1", not isinstance(K, bool) and isinstance(K, int) and K > 1),
               (f"more than one rank (WORLD_SIZE = {world_size})", int(world_size) > 1))
    for what, on in refused:
        if on:
            raise ValueError(f"algorithm.rnn_hidden_size = {H} is not supported with {what} (a recurrent actor reads the newest single observation, "
                             "on one rank, its update on the whole batch as sequences)")
    return H


def rnn_critic_of(cfg, world_size=1):
    """algorithm.rnn_critic (an addition of this build; absent, null or false = off: the shipped yaml does not list it) as the width H of a second GRU
    cell, in front of the critic: algorithm.rnn_hidden_size when the key is on (one width serves both cells, as in rsl_rl's ActorCriticRecurrent), else
    0.  Pure.  ValueError naming the key for a value that is no bool and, naming both keys, for true without a non-zero algorithm.rnn_hidden_size (a
    recurrent critic stands beside a recurrent actor); everything a recurrent actor does not compose with is rnn_hidden_size_of's to refuse."""
    alg = cfg.get("algorithm", {}) or {}
    on = alg.get("rnn_critic", False)
    if on is None:
        on = False
    if not isinstance(on, bool):
        raise ValueError(f"algorithm.rnn_critic must be true or false, got {on!r}")
    if not on:
        return 0
    H = rnn_hidden_size_of(cfg, world_size)
    if not H:
        raise ValueError("algorithm.rnn_critic: true needs algorithm.rnn_hidden_size: 128 or 256 (the critic's cell stands beside a recurrent actor's and has "
                         "its width)")
    return H


def checkpoint_memory_overrides(checkpoint):
    """{"algorithm.rnn_hidden_size": H} for a loaded checkpoint dict whose model carries memory.* and that is no student's (no "distillation" entry: an
    actor trained under algorithm.rnn_hidden_size; a student re-enters under distill.checkpoint_student_overrides), H from memory.weight_hh; None for
    every other checkpoint.  With critic_memory.* in the model (algorithm.rnn_critic) also "algorithm.rnn_critic": True.  What evaluate.py applies so
    that such a checkpoint evaluates without editing the yaml."""
    sd = checkpoint.get("model") or {}
    if checkpoint.get("distillation") is not None or "memory.weight_hh" not in sd:
        return None
    over = {"algorithm.rnn_hidden_size": int(sd["memory.weight_hh"].shape[1])}
    if "critic_memory.weight_hh" in sd:
        over["algorithm.rnn_critic"] = True
    return over


def symmetry_loss(cfg):
    """(on, coefficient) of the mirror-symmetry loss: algorithm.symmetry_loss (an addition of this build; absent = false) and the reference's
    algorithm.symmetric_coef, which the loss reads only when it is on."""
    alg = cfg.get("algorithm", {}) or {}
    on = alg.get("symmetry_loss", False)
    if on is None:
        on = False
    if not isinstance(on, bool):
        raise ValueError(f"algorithm.symmetry_loss must be true or false, got {on!r}")
    if not on:
        return False, 0.0
    coef = alg.get("symmetric_coef", 0.0)
    if isinstance(coef, bool) or not isinstance(coef, (int, float)) or not np.isfinite(coef) or coef < 0:
        raise ValueError(f"algorithm.symmetric_coef must be a finite number >= 0 when algorithm.symmetry_loss is on, got {coef!r}")
    return True, float(coef)


SMOOTHNESS_PAIRS = ("next", "interpolate")  # algorithm.smoothness_pairs: the modes of bg_partner_rows


def smoothness_loss(cfg):
    """(on, coefficient, pairs) of the action-smoothness loss (additions of this build; the shipped yaml lists none of them): algorithm.smoothness_loss
    (absent, null or false = off: (False, 0.0, "next"), the other two keys are then not read), algorithm.smoothness_coef (a finite number >= 0, required
    when the loss is on: nobody has measured a default) and algorithm.smoothness_pairs ("next", the default, or "interpolate").  Pure.  ValueError naming
    the key for every other value and, naming both keys, with what the loss does not compose with: algorithm.symmetry_loss (both claim rows [B, 2B) of
    the actor's batch), runner.num_mini_batches above 1, estimator.enabled (no estimate exists for the row after the last step),
    algorithm.rnn_hidden_size."""
    alg = cfg.get("algorithm", {}) or {}
    on = alg.get("smoothness_loss", False)
    if on is None:
        on = False
    if not isinstance(on, bool):
        raise ValueError(f"algorithm.smoothness_loss must be true or false, got {on!r}")
    if not on:
        return False, 0.0, SMOOTHNESS_PAIRS[0]
    coef = alg.get("smoothness_coef")
    if isinstance(coef, bool) or not isinstance(coef, (int, float)) or not np.isfinite(coef) or coef < 0:
        raise ValueError(f"algorithm.smoothness_coef must be a finite number >= 0 when algorithm.smoothness_loss is on (there is no default), got {coef!r}")
    mode = alg.get("smoothness_pairs", SMOOTHNESS_PAIRS[0])
    if not isinstance(mode, str) or mode not in SMOOTHNESS_PAIRS:
        raise ValueError(f"algorithm.smoothness_pairs must be \"next\" or \"interpolate\", got {mode!r}")
    K = (cfg.get("runner", {}) or {}).get("num_mini_batches", 1) or 1
    refused = (("algorithm.symmetry_loss: true (both losses claim rows [B, 2B) of the actor's batch)", alg.get("symmetry_loss", False) is True),
               ("runner.num_mini_batches above 1", not isinstance(K, bool) and isinstance(K, int) and K > 1),
               ("estimator.enabled: true (there is no estimate for the row after the last step)", estimator_enabled(cfg)),
               ("algorithm.rnn_hidden_size (a recurrent actor's rows are sequences)", bool(alg.get("rnn_hidden_size", 0))))
    for what, hit in refused:
        if hit:
            raise ValueError(f"algorithm.smoothness_loss: true is not supported with {what}")
    return True, float(coef), mode


def mini_batches(cfg):
    """(on, K) of runner.num_mini_batches (an addition of this build, rsl_rl's name; absent or 1 = off: (False, 1)): every mini-epoch takes K optimiser
    steps on disjoint shuffled K-ths of the batch of B = runner.horizon_length x env.num_envs rows (per rank) instead of one step on all of it.
    ValueError unless K is an integer >= 1 that divides B into whole 128-row slabs (the chained kernels store every slab in full; the grouped
    weight gradients need rows % 32 == 0 and >= 128); and, for now, with algorithm.symmetry_loss."""
    K = (cfg.get("runner", {}) or {}).get("num_mini_batches", 1)
    if K is None:
        K = 1
    if isinstance(K, bool) or not isinstance(K, int) or K < 1:
        raise ValueError(f"runner.num_mini_batches must be an integer >= 1, got {K!r}")
    if K == 1:
        return False, 1
    T, N = int(cfg["runner"]["horizon_length"]), int(cfg["env"]["num_envs"])
    B = T * N
    if B % K:
        raise ValueError(f"runner.num_mini_batches = {K} does not divide the batch of runner.horizon_length x env.num_envs = {T} x {N} = {B} rows")
    if (B // K) % 128:
        raise ValueError(f"runner.num_mini_batches = {K} gives mini-batches of {B} / {K} = {B // K} rows, which is not a multiple of 128 (the kernels work "
                         "on whole 128-row slabs)")
    if symmetry_loss(cfg)[0]:
        raise ValueError(f"runner.num_mini_batches = {K} together with algorithm.symmetry_loss is not supported: set runner.num_mini_batches to 1 or "
                         "algorithm.symmetry_loss to false")
    return True, K


def env_mini_batches(cfg):
    """(on, K) of runner.num_env_mini_batches (an addition of this build; absent, null or 1 = off: (False, 1); the shipped yaml does not list it): with
    a recurrent actor (algorithm.rnn_hidden_size) every mini-epoch takes K optimiser steps, step k on the whole T-step sequences of N / K envs of a
    fresh env permutation (rsl_rl's recurrent_mini_batch_generator; runner.num_mini_batches shuffles single rows, which a recurrence cannot run on).
    Pure.  ValueError naming the key unless K is an integer >= 1 that divides env.num_envs = N with T N / K a multiple of 128 (the critic's chained
    kernels run on the step's rows, as under runner.num_mini_batches); and, naming both keys, without algorithm.rnn_hidden_size (a feed-forward actor
    has runner.num_mini_batches) and together with runner.num_mini_batches above 1."""
    run = cfg.get("runner", {}) or {}
    K = run.get("num_env_mini_batches", 1)
    if K is None:
        K = 1
    if isinstance(K, bool) or not isinstance(K, int) or K < 1:
        raise ValueError(f"runner.num_env_mini_batches must be an integer >= 1, got {K!r}")
    if K == 1:
        return False, 1
    if not (cfg.get("algorithm", {}) or {}).get("rnn_hidden_size", 0):
        raise ValueError(f"runner.num_env_mini_batches = {K} needs a recurrent actor (algorithm.rnn_hidden_size: 128 or 256): its mini-batches are whole "
                         "sequences of envs; a feed-forward actor has the shuffle of single rows, runner.num_mini_batches")
    M = run.get("num_mini_batches", 1) or 1
    if not isinstance(M, bool) and isinstance(M, int) and M > 1:
        raise ValueError(f"runner.num_env_mini_batches = {K} together with runner.num_mini_batches = {M} is not supported: a mini-epoch is cut one way, "
                         "by envs (a recurrent actor) or by rows")
    T, N = int(run["horizon_length"]), int(cfg["env"]["num_envs"])
    if N % K:
        raise ValueError(f"runner.num_env_mini_batches = {K} does not divide env.num_envs = {N}")
    if (T * N // K) % 128:
        raise ValueError(f"runner.num_env_mini_batches = {K} gives mini-batches of runner.horizon_length x env.num_envs / {K} = {T} x {N // K} = {T * N // K} "
                         "rows, which is not a multiple of 128 (the critic's kernels work on whole 128-row slabs)")
    return True, K


class UpdatePlan(NamedTuple):
    """The kernels of one Runner.update() and of the rollout's forward-ahead (plan_update): resolved once per call, read by every branch."""
    critic: NetPlan
    actor: NetPlan
    wgrad: int          # products of the grouped weight-gradient launch: 0 = fp32 MFMA (bg_wgrad.hip), 6 / 9 = bf16 splits (bg_wgrad_split.hip)
    fused_head: bool    # output layers fused with the loss (bg_head.hip); False: library GEMMs + bg_ppo_loss
    fused_gae: bool     # critic output layer + GAE in one launch (bg_critic_values_gae)
    chain_values: bool  # ... with the values from the critic's chained forward launch
    one_stream: bool    # each of the forward and backward-data passes of both networks as ONE launch, the mini-epoch on the main stream
    defer: bool         # the small reductions behind heads and backward layers as one launch in front of the weight gradients
    fused_opt: bool     # clip + Adam + KL rule + statistics bookkeeping in one launch (bg_optimizer_step)
    one_tail: bool      # ... together with the deferred sums and the weight gradients' finish (bg_update_tail; the weight gradients partial)
    ahead: bool         # the rollout runs the first mini-epoch's forward passes
    ranks: bool         # several ranks: the exchanges run
    symmetry: bool = False  # the mirror-symmetry loss: the actor trains on 2B rows (the batch, then its mirror images) through bg_actor_head_sym
    smoothness: bool = False  # ... the same plan (symmetry = True) with the partner rows of the action-smoothness loss in rows [B, 2B) (bg_partner_rows)
    gru_group: int = 0  # a recurrent critic beside the recurrent actor, a one-stream step: 1 = both cells' forward recurrences as ONE launch, 2 = the backward ones too
    value_norm: bool = False  # algorithm.normalize_value: the whole-batch pass runs bg_critic_values_gae_norm (the critic's output is standardised)


class CellRows(NamedTuple):
    """The recurrent side of a StepRows (algorithm.rnn_hidden_size): the cell's trainer for the step's rows [T][envs], the state [envs][H] its
    recurrence starts from and the reset flags [T][envs] it reads."""
    trainer: GRUTrainer
    h0: torch.Tensor
    resets: torch.Tensor


class StepRows(NamedTuple):
    """What one optimiser step of Runner.update() reads and writes, built once per update(): the whole batch (Runner._update_begin), one of the K
    mini-batches of runner.num_mini_batches (Runner._mini_batch_begin: rows [k b, (k + 1) b) of the gathered buffers), or one of the K env-wise
    mini-batches of runner.num_env_mini_batches (Runner._env_mini_batch_begin: the same rows of the buffers bg_gather_sequences fills)."""
    ct: MLPTrainer                # the critic's and the actor's trainer
    at: MLPTrainer
    plan: UpdatePlan              # ... and the plan they run under
    rows: int                     # the rows the loss is a mean over
    wgrad: GroupedWeightGrad      # the grouped weight-gradient launch (its descriptors are static per input buffer)
    x_c: torch.Tensor             # the critic's input; the step trains on its first train_rows rows (None: all; the whole batch carries last_values' N rows behind them)
    train_rows: Optional[int]
    x_a: torch.Tensor             # the actor's input (with the symmetry loss 2 x rows: the batch, then its mirror images)
    actions: torch.Tensor
    old_mu: torch.Tensor
    old_logp: torch.Tensor
    adv: torch.Tensor
    ret: torch.Tensor
    values: torch.Tensor          # where the value head of the fused kernels writes the values of x_c's rows
    mem: Optional[CellRows] = None  # a recurrent actor: the cell around the trunk `at` on these rows (x_a: the cell's padded rows)
    cmem: Optional[CellRows] = None  # a recurrent critic: the cell around the trunk `ct` on these rows (x_c: the cell's padded rows)


RND_LOG = ("rnd/intrinsic_reward", "rnd/weight", "rnd/reward_std", "rnd/loss")  # the log scalars of rnd.enabled, in RndTrainer.log's order

TAIL_MAX_ITEMS = _lib.TAIL_MAX_BLOCKS  # blocks of sums of one bg_update_tail launch (bg_tail.hip)


def plan_update(critic, actor, rows, *, split, fused, chain, chain_split, chain_split_bwd, chain_alternate, fused_wgrad, wgrad_split, one_stream,
                defer_finish, one_launch_tail, fused_opt, fused_head, fused_gae, chain_values, rollout_forward, dp_active, symmetry=False, memory=0, smoothness=False, critic_memory=0,
                gru_group=0, value_norm=False):
    """UpdatePlan from the switches (MLPTrainer.SPLIT ... WGRAD_SPLIT and Runner._one_stream ... _rollout_forward, by the same names in lower case;
    dp.active; symmetry = algorithm.symmetry_loss) and the shapes: critic / actor = (layer widths, padded input width), rows = the batch.  Pure: no
    tensors, no device.  symmetry: the actor's passes differentiate 2 x rows rows (the batch and its mirror images) and the rollout runs no
    forward passes for the update (ahead = False: update() mirrors the batch and runs the first mini-epoch's passes itself); a plan whose output
    layers are not the fused head kernels is a ValueError (bg_actor_head_sym is the only form of the loss).  smoothness = algorithm.smoothness_loss:
    a second source of partner rows for the same 2B-row actor path, so the plan is the one of symmetry = True (its `symmetry` field included) with
    `smoothness` set, and the same ValueError without the fused heads.  memory = H > 0
    (algorithm.rnn_hidden_size): `actor` is the trunk behind the GRU cell, its input the cell's state of H columns, so it runs the per-layer kernels
    beside whatever the critic runs (as on a frame stack), without forward-ahead; the cell's gradients come out of launches that bg_update_tail's sums
    do not cover (its weight gradients' finish, its bias gradients' reduction), so the tail runs as the separate launches (one_tail = False:
    bg_reduce_group, the weight gradients with their finish, bg_optimizer_step, which takes the norm over the whole flat gradient, the cell's
    included); a plan without the fused heads or the deferred reductions is a ValueError.  critic_memory = H > 0 (algorithm.rnn_critic, with memory):
    `critic` is likewise the trunk behind the critic's cell, on the per-layer kernels, its values from the stored activations; gru_group
    (BG_GRU_GROUP): the plan's field of that name.  value_norm = algorithm.normalize_value: the plan's field of that name; the de-standardised values
    exist only inside bg_critic_values_gae_norm, so a plan without the fused heads or without the fused GAE launch is a ValueError."""
    if value_norm and not (fused_head and fused_gae):
        raise ValueError(f"{VALUE_NORM_KEY} needs " + ("the fused output layers of bg_head.hip (a critic whose last hidden layer is 128 wide, 12 actions)"
                                                       if not fused_head else "the fused GAE launch bg_critic_values_gae_norm (runner.horizon_length of 32 or less)")
                         + ": the value is de-standardised inside that launch only")
    if memory and not (fused_head and fused and defer_finish and not split):
        raise ValueError("algorithm.rnn_hidden_size needs the fused output layers of bg_head.hip, the per-layer fp32 kernels and the deferred reductions "
                         "(no parallel.gemm_split / BG_GEMM_SPLIT, BG_DEFER_FINISH=1)")
    if smoothness and not fused_head:
        raise ValueError("algorithm.smoothness_loss needs the fused output layers of bg_head.hip (bg_actor_head_sym: an actor whose last hidden layer is "
                         "128 wide with 12 actions); this plan runs the output layers as library GEMMs")
    symmetry = bool(symmetry or smoothness)
    if symmetry and not fused_head:
        raise ValueError("algorithm.symmetry_loss needs the fused output layers of bg_head.hip (bg_actor_head_sym: an actor whose last hidden layer is "
                         "128 wide with 12 actions); this plan runs the output layers as library GEMMs")
    nets = [plan_network(w, kin, r, split, fused, chain, chain_split, chain_split_bwd and fused_head, chain_alternate, fused_wgrad)
            for (w, kin), r in ((critic, rows), (actor, 2 * rows if symmetry else rows))]
    if memory and ((nets[1].fwd, nets[1].bwd) != ("layer", "layer") or not all(nets[1].grouped[:-1])):
        raise ValueError(f"algorithm.rnn_hidden_size: a batch of runner.horizon_length x env.num_envs = {rows} rows is outside the range of the layer kernels "
                         "(an even number of 64 rows or more)")
    if critic_memory and not memory:
        raise ValueError("algorithm.rnn_critic needs algorithm.rnn_hidden_size (a recurrent critic stands beside a recurrent actor)")
    if critic_memory and ((nets[0].fwd, nets[0].bwd) != ("layer", "layer") or not all(nets[0].grouped[:-1])):
        raise ValueError(f"algorithm.rnn_critic: a batch of runner.horizon_length x env.num_envs = {rows} rows is outside the range of the layer kernels "
                         "(an even number of 64 rows or more)")
    bwd_chained = all(n.bwd == "chain_split" for n in nets)
    grouped = [(co, ci) for (w, kin), n in zip((critic, actor), nets) for ci, co, g in zip((kin,) + tuple(w[1:-1]), w[1:], n.grouped) if g]
    wgrad = wgrad_products(rows, grouped, bwd_chained, split, wgrad_split)
    chain_values = fused_head and fused_gae and chain_values and nets[0].chained
    defer = fused_head and defer_finish and not split
    # bg_update_tail takes the gradient's norm from its own sums, so every gradient element must come out of them: all hidden layers' weight gradients
    # from the grouped launch, every hidden layer's bias gradient from a deferred finish (of the chained backward launch, or of a partial per-layer
    # backward launch of every layer), at most 8 finish descriptors in all
    fins = [1 if n.bwd == "chain_split" else len(w) - 3 for (w, _), n in zip((critic, actor), nets)]
    finishing = all(n.bwd == "chain_split" or n.bwd == "layer" and all(MLPTrainer.bwd_fusable(co, ci) for ci, co in zip(w[1:-2], w[2:-1]))
                    for (w, _), n in zip((critic, actor), nets))
    # ... and at most TAIL_MAX_ITEMS blocks of sums in that launch (bg_tail.hip): the weight gradients' finish (64 elements per block: 4,096 for a
    # 512 x 512 layer) and the deferred reductions (the heads' gradients and statistics, the per-layer bias gradients: 16 per block).  Beyond it
    # (two 512 x 512 layers) the sums run as their own launches in front of bg_optimizer_step.
    sums = sum((co * ci // 4 + 15) // 16 for co, ci in grouped) + sum((w[-2] * w[-1] + w[-2] + w[-1] + 15) // 16 + 32 + sum((ci + 15) // 16 for ci in w[1:-2])
                                                                       for w, _ in (critic, actor))
    one_tail = (fused_opt and one_launch_tail and defer and finishing and all(all(n.grouped[:-1]) for n in nets) and sum(fins) + 2 <= 8
                and sums <= TAIL_MAX_ITEMS and not memory)
    return UpdatePlan(nets[0], nets[1], wgrad, fused_head, fused_gae, chain_values, one_stream and chain_values and defer and bwd_chained, defer, fused_opt,
                      one_tail, rollout_forward and chain_values and nets[1].chained and not symmetry, dp_active, bool(symmetry), bool(smoothness),
                      int(gru_group) if critic_memory else 0, bool(value_norm))


class Runner:
    def __init__(self, test=False, args=None, cfg=None):
        self.test = test
        self.dp = DataParallel()
        self.world_size, self.rank, self.local_rank = self.dp.world_size, self.dp.rank, self.dp.local_rank
        if cfg is None:
            self._get_args(args)
            self._update_cfg_from_args()
        else:
            self.cfg = cfg
            self.cfg["basic"].setdefault("task", "T1")
        self.cfg["basic"]["rank"] = self.rank
        self.actor_hidden, self.critic_hidden = hidden_widths(self.cfg)  # (before anything is built: a width outside the supported set is a ValueError)
        if self.world_size > 1:  # one process per GPU: each rank simulates and learns on its own device
            self.cfg["basic"]["sim_device"] = self.cfg["basic"]["rl_device"] = f"cuda:{self.dp.device_index}"
        # algorithm.smoothness_loss: the action-smoothness loss, a second source of partner rows for the symmetry loss's 2B-row actor path (ValueError
        # before anything is built, also for what it does not compose with); False = off, the one switch every branch below reads
        self._smooth, self._smooth_coef, self._smooth_pairs = smoothness_loss(self.cfg)
        self._mini_batches = mini_batches(self.cfg)[1]  # (ValueError before anything is built; 1 = off: the one switch every branch below reads)
        # runner.num_env_mini_batches: the K steps of a mini-epoch on whole sequences of N / K envs, a recurrent actor's mini-batches (likewise; the key
        # belongs to training: play and evaluation do not read it)
        self._env_mini_batches = 1 if test else env_mini_batches(self.cfg)[1]
        # estimator.enabled: a learned state estimator in front of the actor (utils/estimator.py); None = off, the one switch every branch below reads
        self._est = estimator_cfg(self.cfg, self.world_size)
        # rnd.enabled: an intrinsic reward by random network distillation (utils/rnd.py); None = off, the one switch every branch below reads.  The
        # section belongs to training: a runner that only plays never evaluates these networks and does not read it
        self._rnd = None if test else rnd_cfg(self.cfg, self.world_size)
        # algorithm.actor_memory: a recurrent distilled student re-entering for play / evaluation / export; 0 = none, the one switch the branches below read
        self._memory = actor_memory_of(self.cfg)
        # algorithm.rnn_hidden_size: PPO on a recurrent actor; the same cell, and the one key under which a model with memory trains (a student's
        # re-entry overrides alone must not start a PPO run: its critic is untrained)
        self._rnn = rnn_hidden_size_of(self.cfg, self.world_size)
        if self._memory and not self._rnn and not test:
            raise ValueError(f"algorithm.actor_memory = {self._memory}: training is out of scope for this key, which is for a distilled student's checkpoint "
                             "under play.py, evaluate.py and export_model.py; PPO on a recurrent actor (from scratch, or fine-tuning that student) is "
                             f"algorithm.rnn_hidden_size: {self._memory} (training a recurrent student: distill.py --student_memory)")
        self._memory = self._memory or self._rnn
        # algorithm.rnn_critic: a second cell of the same width in front of the critic; 0 = a feed-forward critic, the one switch the branches below read
        self._rnn_critic = rnn_critic_of(self.cfg, self.world_size)
        if self._rnn and not test and (int((self.cfg.get("parallel", {}) or {}).get("gemm_split", 0) or 0) or MLPTrainer.SPLIT):
            raise ValueError(f"algorithm.rnn_hidden_size = {self._rnn} is not supported with parallel.gemm_split / BG_GEMM_SPLIT (the trunk behind the cell "
                             "runs the per-layer fp32 kernels): use gemm_split 0")
        self._set_seed()
        task = self.cfg["basic"]["task"]
        if task not in TASKS:
            raise NameError(f"name {task!r} is not defined")  # reference: eval(task) (runner.py:27)
        self.env = TASKS[task](self.cfg)

        self.device = self.cfg["basic"]["rl_device"]
        if torch.device(self.device) != torch.device(self.env.device):
            raise ValueError("rl_device must equal sim_device: the rollout writes simulator outputs straight into the PPO buffers")
        self.learning_rate = self.cfg["algorithm"]["learning_rate"]
        self._symmetry, self._symmetric_coef = symmetry_loss(self.cfg)
        obs_norm_on, obs_norm_eps = normalization_cfg(self.cfg)  # (ValueError for normalization_eps <= 0)
        if self._symmetry:  # (ValueError for a model without a left / right pairing or with an asymmetric default pose)
            obs_src, obs_sign, act_src, act_sign = self.env.mirror_maps()
            self._act_mirror = (act_src.tolist(), act_sign.tolist())
        est_args = {} if self._est is None else {"estimator_hidden": self._est.hidden, "estimator_cols": len(self._est.targets)}
        if self._memory:
            est_args = {"memory_hidden": self._memory}
        if self._rnn_critic:
            est_args["critic_memory_hidden"] = self._rnn_critic
        if self._rnd is not None:
            if self._rnd.width != self.env.num_obs + (self.env.num_privileged_obs if self._rnd.state == "critic" else 0):
                raise ValueError(f"rnd.state = {self._rnd.state!r}: the config's rows have {self._rnd.width} columns, the env's "
                                 f"{self.env.num_obs} + {self.env.num_privileged_obs}")
            est_args["rnd"] = (self._rnd.width, self._rnd.predictor_hidden, self._rnd.target_hidden, module_seed(self.cfg["basic"]["seed"]))
        self.model = ActorCritic(self.env.num_actions, self.env.num_obs, self.env.num_privileged_obs, self.actor_hidden, self.critic_hidden, **est_args).to(self.device)
        self.dp.broadcast_parameters(self.model)  # identical initial weights on every rank
        # algorithm.empirical_normalization: running mean / variance of the critic's input columns (the actor's are its first num_obs), applied where rows
        # enter a network and updated at the end of update(); None = off, the one switch every branch below reads
        self.obs_norm = ObsNormalizer(self.env.num_obs + self.env.num_privileged_obs, obs_norm_eps, self.device) if obs_norm_on else None
        # algorithm.normalize_value: running mean / variance of the returns; the critic's output is standardised (utils/value_norm.py).  None = off, the
        # one switch every branch below reads; also None in a runner that only plays (it never evaluates the critic)
        value_norm_on, value_norm_eps = normalize_value_of(self.cfg)  # (ValueError for anything but a bool, and for normalization_eps <= 0)
        self.value_norm = ValueNormalizer(value_norm_eps, self.device) if value_norm_on and not test else None
        self._clock = WeightClock()  # the version of the parameters, shared by every trainer over them: see invalidate()
        # ... and of the estimator's, a clock of its own: PPO's steps do not change its parameters, its steps not PPO's
        self._est_clock = WeightClock() if self._est is not None else None
        self._rnd_clock = WeightClock() if self._rnd is not None else None  # ... and of the RND predictor's, likewise
        self.invalidate()
        self.optimizer = FlatAdam(self.model.ppo_parameters(), lr=self.learning_rate)  # (critic, actor, logstd: all parameters of a model without an estimator)
        if self._est is not None:  # the estimator's own optimiser: no PPO gradient reaches it, PPO's buffer holds what it holds without the key
            self._est_opt = FlatAdam(self.model.estimator.parameters(), lr=self._est.learning_rate, max_grad_norm=self._est.max_grad_norm)
        self._rnd_trainer = None
        if self._rnd is not None:  # the predictor's own optimiser, the reward normaliser and the launch's descriptors; the target has no optimiser
            rnd_opt = FlatAdam(self.model.rnd_predictor.parameters(), lr=self._rnd.learning_rate, max_grad_norm=self._rnd.max_grad_norm)
            self._rnd_trainer = RndTrainer(self._rnd, self.model, rnd_opt, self._rnd_clock, self.cfg["runner"]["horizon_length"], self.env.num_envs, self.env.num_obs,
                                           value_norm_eps, self.device)
        self._load()
        # Resume semantics of the reference (runner.py:31-34,174-180): the restored param_group lr serves the FIRST optimiser step only; the
        # first KL adaptation then overwrites it with a value derived from self.learning_rate = the yaml value, so adaptation restarts from
        # cfg.algorithm.learning_rate, not from the checkpoint's lr.  Same here (see update()).
        self._lr_restart = bool(self.cfg["basic"].get("checkpoint"))
        # common state of the command-curriculum grid across ranks = whatever the env holds now (initial grid, or the restored one)
        self._curr_last = self.env.curriculum_prob.clone() if self.dp.active and self.cfg["commands"].get("curriculum", False) else None

        T, N = self.cfg["runner"]["horizon_length"], self.env.num_envs
        self.buffer = ExperienceBuffer(T, N, self.device)
        self.buffer.add_buffer("actions", (self.env.num_actions,))
        self.buffer.add_buffer("obses", (self.env.num_obs,), extra_rows=1)
        self.buffer.add_buffer("privileged_obses", (self.env.num_privileged_obs,), extra_rows=1)
        self.buffer.add_buffer("rewards", ())
        self.buffer.add_buffer("dones", (), dtype=torch.bool)
        self.buffer.add_buffer("time_outs", (), dtype=torch.bool)
        if self._est is not None:  # step n's 12 estimator outputs, computed from obses[n] by the estimator as it was then (rollout)
            self.buffer.add_buffer("estimates", (EST_WIDTH,))
        if self._rnd is not None:  # step n's raw rho and the target's 12 outputs on the state after step n: the predictor's labels
            self.buffer.add_buffer("intrinsic_rewards", ())
            self.buffer.add_buffer("rnd_targets", (RND_WIDTH,))
        B, A = T * N, self.env.num_actions
        dev = self.device
        # network inputs with the feature dimension zero-padded, each network on its own (pad_input: actor 47 -> 64, critic 61 -> 64, or 61 + P -> 128 /
        # 256 / 512 with the terrain height scan; with env.frame_stack = H the actor's 47 H and the critic's 47 H + 14 + P likewise) so that the first
        # layers run on the fused MFMA kernels
        no, npv = self.env.num_obs, self.env.num_privileged_obs
        E = self._est_cols = 0 if self._est is None else len(self._est.targets)  # the actor's input: the env's row and, behind it, E estimates
        self._pad_actor = pad_input(no + E) if MLPTrainer.FUSED else None
        self._pad_critic = pad_input(no + npv) if MLPTrainer.FUSED else None
        if self._pad_actor and self._pad_actor > 256 and (int((self.cfg.get("parallel", {}) or {}).get("gemm_split", 0) or 0) or MLPTrainer.SPLIT):
            raise ValueError(f"parallel.gemm_split / BG_GEMM_SPLIT runs split-bf16 layer kernels that take layer inputs of 64, 128 or 256 columns only; the "
                             f"actor's input of {no + E} observations pads to {self._pad_actor} (env.frame_stack 5 or less, without terrain.actor_heights or with fewer points of its scan, or gemm_split 0)")
        if self._pad_critic and self._pad_critic > 256 and (int((self.cfg.get("parallel", {}) or {}).get("gemm_split", 0) or 0) or MLPTrainer.SPLIT):
            raise ValueError(f"parallel.gemm_split / BG_GEMM_SPLIT runs split-bf16 layer kernels that take layer inputs of 64, 128 or 256 columns only; the "
                             f"critic's input {no} + {npv} pads to {self._pad_critic} (fewer terrain.measured_points_x / _y points, or gemm_split 0)")
        self._critic_in = torch.zeros(T + 1, N, self._pad_critic or (no + npv), device=dev)
        self._actor_in = torch.zeros(T, N, self._pad_actor, device=dev) if self._pad_actor else None
        if self._smooth:
            # the actor's input of 2B rows: the batch, then its partner rows (bg_partner_rows in update()), and the one more step of source rows that
            # the last step's partners come from: the actor's rows of obses[T]
            if not self._pad_actor or self._pad_actor > 512:
                raise ValueError(f"algorithm.smoothness_loss needs the actor's padded input of at most 512 columns (bg_partner_rows moves 16-byte pieces of "
                                 f"rows), env.num_observations = {no}" + (" pads to " + str(self._pad_actor) if self._pad_actor else " is not padded on this path"))
            self._actor_in = torch.zeros(2 * T, N, self._pad_actor, device=dev)
            self._actor_last = torch.zeros(N, self._pad_actor, device=dev)
            self._act_identity = (list(range(A)), [1.0] * A)  # the head's action map: d = mu(x') - mu(x)
            self._smooth_updates = 0  # the update counter of the draw's key (pairs "interpolate"); restarts at 0 on resume, like _mb_updates
        if self._symmetry:
            # the actor's input of 2B rows: the batch, then its mirror images (bg_mirror_rows in update(); the padded columns stay zero)
            kin = self._pad_actor or self.env.num_obs
            self._actor_in = torch.zeros(2 * T, N, kin, device=dev)
            self._obs_mirror = (obs_src.tolist() + [-1] * (kin - len(obs_src)), obs_sign.tolist() + [1.0] * (kin - len(obs_sign)))
        if self.obs_norm is not None:
            self._obs_normed = torch.zeros(N, no, device=dev)  # one step's normalised rows: what the sampling kernel reads in rollout()
            if self._symmetry:  # the mirror images of the raw batch, normalised into rows [B, 2B) of the actor's input
                self._mirror_raw = torch.zeros(B, no, device=dev)
                self._obs_mirror_raw = (obs_src.tolist(), obs_sign.tolist())
        self._adv = torch.zeros(T, N, device=dev)
        self._ret = torch.zeros(T, N, device=dev)
        # (algorithm.normalize_value: the first three of the launch's six sums; what the ranks exchange per mini-epoch stays these three)
        self._adv_sums = torch.zeros(3, dtype=torch.float64, device=dev) if self.value_norm is None else self.value_norm.sums[:3]
        self._grad_mu = torch.zeros(B, A, device=dev)
        self._grad_val = torch.zeros(B, device=dev)
        # the float64 sums of a mini-epoch that every rank needs in full: loss / KL statistics [5] and the log-std gradient [A], contiguous so that ONE
        # collective carries both (exchange (3); the log-std gradient then enters the optimiser launch in float64 and not through the fp32 bucket)
        # (with the symmetry loss a sixth statistic: the sum of squared mean asymmetries; without it the layout, and what the ranks exchange, stays five)
        # (the action-smoothness loss uses the same sixth slot: the sum of squared differences of the pairs' means)
        S = self._n_stats = 6 if self._symmetry or self._smooth else 5
        self._sums = torch.zeros(S + A, dtype=torch.float64, device=dev)
        self._stats, self._grad_logstd = self._sums[:S], self._sums[S:]
        self._stats_acc = torch.zeros(S, dtype=torch.float64, device=dev)
        self._stats_last = torch.zeros(S, dtype=torch.float64, device=dev)  # the last mini-epoch's sums (kl_mean of the log, runner.py:199)
        # False: the mini-epoch tail as separate launches (bg_adam_step, bg_adapt_lr, torch adds / fills): what the first optimiser step after a
        # checkpoint restore runs (see update()); as an attribute for the tests that compare the two forms
        self._fused_opt = True
        # ... and, single process only, the sums in front of it (weight-gradient finish, deferred reductions) as ONE launch that also leaves the squared
        # gradient norm in pieces, so that the optimiser launch need not read the whole gradient in every workgroup (bg_update_tail); False:
        # reduce_group, weight gradients + finish, optimizer_step as separate launches (what the ranks of a multi-GPU job run: the norm is the averaged gradient's)
        self._one_launch_tail = os.environ.get("BG_ONE_LAUNCH_TAIL", "1") == "1"
        self._old_logp = torch.zeros(B, device=dev)
        self._logstd_off = (self.model.logstd.grad.data_ptr() - self.optimizer.grad.data_ptr()) // 4  # position of logstd in the flat buffers
        self._actor_tr, self._critic_tr = MLPTrainer(self.model.actor, clock=self._clock), MLPTrainer(self.model.critic, clock=self._clock)
        # algorithm.rnn_hidden_size: the cell around the actor's trunk over the T steps of an iteration (model.GRUTrainer, as utils/distill.py; its bias
        # gradients as ONE launch that joins the deferred reductions) and the done flags of the previous iteration's last step; None = a feed-forward
        # actor (or a recurrent one that only plays), the one switch rollout() and update() read.  The state itself is the model's (sample_actions).
        self._mem_tr = None
        if self._rnn and not test:
            self._mem_tr = GRUTrainer(self.model.memory, self._actor_tr, T, N, clock=self._clock, bias_partial=True)
            self._last_dones = torch.zeros(N, dtype=torch.uint8, device=dev)
        # algorithm.rnn_critic: the second cell around the critic's trunk.  Its forward pass walks T + 1 steps (the row after the last step gives
        # last_values) from a state that no rollout launch advances: GRUTrainer.carry_state.  None = a feed-forward critic
        self._cmem_tr = None
        if self._rnn_critic and not test:
            if not self._pad_critic:
                raise ValueError("algorithm.rnn_critic needs the critic's zero-padded input (the fused layer kernels)")
            self._cmem_tr = GRUTrainer(self.model.critic_memory, self._critic_tr, T, N, clock=self._clock, bias_partial=True, kin=self._pad_critic, extra_steps=1)
        # BG_GRU_GROUP: both cells' recurrences of a one-stream step (runner.num_env_mini_batches) as ONE launch.  1 (the default): the forward ones
        # (bg_gru_sequence_forward_group: 0.53x the two single launches at 1,024 envs each); 2: the backward ones too (bg_gru_sequence_backward_group,
        # not the faster side: its H = 128 kernel compiles to 512 registers with spills where the single one takes 356 -- DESIGN.md section 6.21);
        # 0: single launches both ways.  Resolved into the plan like the other switches
        self._gru_group = {"0": 0, "1": 1, "2": 2}[os.environ.get("BG_GRU_GROUP", "1")]
        gs = (self.cfg.get("parallel", {}) or {}).get("gemm_split", 0)
        if gs:  # yaml switch for the split-bf16 GEMMs (process-wide, like the environment variable)
            if int(gs) not in (6, 9):
                raise ValueError(f"parallel.gemm_split must be 0, 6 or 9, got {gs!r}")
            MLPTrainer.SPLIT = int(gs)
        self._wgrad_group = GroupedWeightGrad()
        # the critic's stream goes ahead of the actor's in workgroup dispatch: its chain is the longer one and the actor's loss waits for its GAE
        # (update 23.17 -> 23.06 ms in round 2, 21.83-21.91 -> 21.55-21.65 ms in round 3 against equal priorities, tools/archive/ab_prio.sh)
        self._side_stream = torch.cuda.Stream(device=self.device, priority=-1)
        # The small fixed-order reductions behind the head / backward-layer kernels run as ONE launch in front of the weight gradients instead of
        # inside the chains, where each of them waits 20-45 us for a workgroup slot between the other network's resident GEMM workgroups (see
        # update()).  Measured in the loop (tools/ab_env.sh, 4 alternating runs of 20 iterations each): update 21.68-21.91 ms with the one launch in
        # front of the weight gradients (BG_DEFER_FINISH=1, the default), 21.99-22.04 ms with the finishes inside the chains (=0).  (On the side stream
        # beside the weight gradients it was 21.85-21.97 ms: it delays the one-workgroup-per-CU launch.)
        self._defer_finish = {"0": False, "1": True}[os.environ.get("BG_DEFER_FINISH", "1")]  # (KeyError for 2: the side-stream form is gone)
        # critic output layer + GAE in one launch (bg_critic_values_gae: horizons up to 32 steps); otherwise bg_critic_head_forward, a fill and bg_gae
        self._fused_gae = self.cfg["runner"]["horizon_length"] <= 32
        self._chain_values = True  # ... with the values from the chained forward kernel's value head (False: from the stored activations)
        # the two networks' chained forward launches of a mini-epoch share the chip by CUs (each a persistent grid over its slabs, _plan_chain_split);
        # False: one workgroup per slab, dispatched as CUs fall free
        self._split_chain_cus = os.environ.get("BG_SPLIT_CHAIN_CUS", "1") == "1"
        self._split_bwd_chain_cus = os.environ.get("BG_SPLIT_BWD_CHAIN_CUS", "1") == "1"  # ... and the two chained backward launches
        # Both networks' forward chains as ONE launch and both backward chains as ONE launch, the whole mini-epoch on the main stream (round 6): the
        # networks share the chip by CUs inside one grid exactly as the two launches did, and no kernel of the mini-epoch waits for an event of another
        # stream any more (three hand-overs on its critical path, 7-20 us each in a kernel trace).  0: two launches on two streams
        self._one_stream = os.environ.get("BG_ONE_STREAM", "1") == "1"
        self._gae_scratch = torch.zeros((3 if self.value_norm is None else 6) * ((self.env.num_envs + 15) // 16) + 1, dtype=torch.float64, device=self.device)

        # fused output layers + loss (bg_head.hip): both networks end in a 128-wide ELU layer, 12 actions / 1 value (utils/model.py); a model of
        # other widths runs the output layers as library GEMMs + bg_ppo_loss (as an attribute for the test that compares the two forms)
        self._fused_head = A == 12 and self.model.actor[-1].in_features == 128 and self.model.critic[-1].in_features == 128
        if self._smooth and not self._fused_head:
            raise ValueError("algorithm.smoothness_loss needs the fused output layers of bg_head.hip: an actor whose last hidden layer is 128 wide with 12 actions")
        if self._symmetry and not self._fused_head:
            raise ValueError("algorithm.symmetry_loss needs the fused output layers of bg_head.hip: an actor whose last hidden layer is 128 wide with 12 actions")
        if self._mem_tr is not None and not (self._fused_head and self._pad_actor == GRUTrainer.KIN):
            raise ValueError(f"algorithm.rnn_hidden_size = {self._rnn} needs the fused output layers of bg_head.hip (12 actions) and an observation of at "
                             f"most {GRUTrainer.KIN} columns (env.num_observations = {no})")
        self._old_mu = torch.zeros(B, A, device=dev)
        self._values_all = torch.zeros(B + N, device=dev)
        self._head_scratch_a, self._head_scratch_c = head_scratch(dev), head_scratch(dev)
        self._act_counter = 0
        # The forward passes of the first mini-epoch run DURING the rollout (see rollout()): 1 = on (default where the chained kernels apply), 0 = off
        # (off with the estimator: step n's estimate, a part of the actor's row, does not exist when step n's rows would be forwarded)
        self._rollout_forward = os.environ.get("BG_ROLLOUT_FORWARD", "1") == "1" and self._pad_actor is not None and N % 128 == 0 and self._est is None
        # ... the rows of this many consecutive steps per group of side-stream launches.  Every group costs the main stream one event record (2.9 us, 5.7
        # with a waiter on another queue: tools/event_cost_probe.py), and from four steps per group on the chained launches need more than the 128 CUs
        # the env step leaves idle and slow it down (110 against 102.5 us).  Same box, 20 iterations each, ms per iteration: off 24.78-24.92, one step
        # per group 24.46-24.49, two 24.39-24.41, three 24.42-24.47, four 24.55-24.66, eight 24.58-24.65 (profiles/r04_rollout_forward_ab.txt).
        self._rollout_group = max(1, int(os.environ.get("BG_ROLLOUT_FORWARD_GROUP", "2")))
        self._fwd_plan = None  # the UpdatePlan under which rollout() has left the activations / values / old mu of the whole batch in the trainers' buffers
        self.timers = {"rollout": 0.0, "update": 0.0}
        if self._mini_batches > 1:
            self._init_mini_batches()
        if self._env_mini_batches > 1:
            self._init_env_mini_batches()
        if self._symmetry or self._smooth:
            self._resolve_plan()  # (a plan the symmetric head cannot serve is a ValueError here, not at the first update)
        if self.value_norm is not None:
            if self.cfg["runner"]["horizon_length"] > 32:
                raise ValueError(f"{VALUE_NORM_KEY} needs runner.horizon_length of 32 or less, got {self.cfg['runner']['horizon_length']}: the value is "
                                 "de-standardised inside the fused GAE launch bg_critic_values_gae_norm, which scans up to 32 steps")
            self._resolve_plan()  # (ValueError for a plan without the fused heads: here, not at the first update)
        if self._est is not None:  # its supervised update (a batch outside the layer kernels' range is a ValueError here, not at the first update)
            self._est_trainer = EstimatorTrainer(self._est, self.model.estimator, self._est_opt, self._est_clock, T, N, no, dev)

    # ------------------------------------------------------------------ config / seed / checkpoint (runner.py:44-97)
    def _get_args(self, args=None):
        parser = argparse.ArgumentParser()
        parser.add_argument("--task", required=True, type=str, help="Name of the task to run.")
        parser.add_argument("--checkpoint", type=str, help="Path of the model checkpoint to load. Overrides config file if provided.")
        parser.add_argument("--num_envs", type=int, help="Number of environments to create. Overrides config file if provided.")
        parser.add_argument("--headless", type=bool, help="Run headless. Overrides config file if provided.")
        parser.add_argument("--sim_device", type=str, help="Device for physics simulation. Overrides config file if provided.")
        parser.add_argument("--rl_device", type=str, help="Device for the RL algorithm. Overrides config file if provided.")
        parser.add_argument("--seed", type=int, help="Random seed. Overrides config file if provided.")
        parser.add_argument("--max_iterations", type=int, help="Maximum number of training iterations. Overrides config file if provided.")
        self.args = parser.parse_args(args)

    def _update_cfg_from_args(self):
        self.cfg = load_cfg(self.args.task)
        for arg, val in vars(self.args).items():
            if val is not None:
                if arg == "num_envs":
                    self.cfg["env"][arg] = val
                else:
                    self.cfg["basic"][arg] = val
        if not self.test:
            self.cfg["viewer"]["record_video"] = False

    def _set_seed(self):
        if self.cfg["basic"]["seed"] == -1:
            # one draw for the whole job: terrain and the logged config.yaml must be the same on every rank (rank offsets are applied
            # where per-rank streams are wanted: T1._cfg_struct and the rollout seed)
            self.cfg["basic"]["seed"] = self.dp.broadcast_int(np.random.randint(0, 10000))
        seed = self.cfg["basic"]["seed"]
        if self.rank == 0:
            print("Setting seed: {}".format(seed))
        random.seed(seed)
        np.random.seed(seed)
        torch.manual_seed(seed)
        os.environ["PYTHONHASHSEED"] = str(seed)
        torch.cuda.manual_seed_all(seed)

    def _load(self):
        ck = self.cfg["basic"].get("checkpoint")
        if not ck:
            return
        if ck == "-1" or ck == -1:
            ck = sorted(glob.glob(os.path.join("logs", "**/*.pth"), recursive=True), key=os.path.getmtime)[-1]
            self.cfg["basic"]["checkpoint"] = ck
        print("Loading model from {}".format(ck))
        model_dict = torch.load(ck, map_location=self.device, weights_only=True)
        ck_mem = int(model_dict["model"]["memory.weight_hh"].shape[1]) if "memory.weight_hh" in model_dict["model"] else 0
        if ck_mem != getattr(self, "_memory", 0):
            raise ValueError(f"checkpoint {ck} has " + (f"a recurrent actor (memory.* of width {ck_mem})" if ck_mem else "no memory.* (its actor is not recurrent)")
                             + f", the config has algorithm.actor_memory = {getattr(self, '_memory', 0)}: set algorithm.actor_memory to {ck_mem}"
                             + (" (a student of distillation.student_memory, or an actor trained under algorithm.rnn_hidden_size, the key to train it "
                                "further under; evaluate.py and export_model.py set the width from the checkpoint)" if ck_mem else ""))
        ck_cmem = int(model_dict["model"]["critic_memory.weight_hh"].shape[1]) if "critic_memory.weight_hh" in model_dict["model"] else 0
        # (a recurrent student re-entering for fine-tuning carries an UNTRAINED feed-forward critic: under algorithm.rnn_critic the critic built here,
        # cell and trunk, stays as initialised and the student's critic.* is not loaded)
        fresh_critic = bool(getattr(self, "_rnn_critic", 0)) and not ck_cmem and model_dict.get("distillation") is not None
        if ck_cmem != getattr(self, "_rnn_critic", 0) and not fresh_critic:
            raise ValueError(f"checkpoint {ck} has " + (f"a recurrent critic (critic_memory.* of width {ck_cmem})" if ck_cmem else "no critic_memory.* (its critic "
                             "is not recurrent)") + f", the config has algorithm.rnn_critic: {'true' if getattr(self, '_rnn_critic', 0) else 'false'}: set "
                             f"algorithm.rnn_critic to {'true' if ck_cmem else 'false'} (evaluate.py sets it from the checkpoint)")
        ck_ain, a_in = int(model_dict["model"]["actor.0.weight"].shape[1]), self.model.actor[0].in_features
        est = getattr(self, "_est", None)
        check_estimator_checkpoint(ck, model_dict, est, ck_ain, a_in)  # (before the frame-stack message below can misfire on a width that differs by E)
        if not getattr(self, "test", False):  # (a runner that plays never evaluates the RND networks: it loads such a checkpoint under either setting)
            check_rnd_checkpoint(ck, model_dict, getattr(self, "_rnd", None))  # (ValueError naming rnd.enabled / rnd.state / the widths)
        scan_ck, scan_cfg = (int(model_dict["height_points"].shape[0]) if "height_points" in model_dict else 0), getattr(self.env, "num_scan_obs", 0)
        if ck_ain != a_in and ck_ain - scan_ck == a_in - scan_cfg:  # (the widths differ by the height scan in the actor's row)
            raise ValueError(f"checkpoint {ck} has an actor of {ck_ain} inputs, {scan_ck} of them the terrain height scan, the config's actor takes {a_in} "
                             f"with {scan_cfg}: terrain.actor_heights (and terrain.measured_points_x / measured_points_y, env.num_observations) must be "
                             "as in the run that saved the checkpoint")
        if ck_ain != a_in:  # (the actor's input: env.frame_stack single observations of 47)
            raise ValueError(f"checkpoint {ck} has an actor of {ck_ain} inputs, the config's actor takes {a_in} (env.num_observations = "
                             f"{self.env.num_single_obs} x env.frame_stack): env.frame_stack must be as in the run that saved the checkpoint "
                             f"({ck_ain // self.env.num_single_obs if ck_ain % self.env.num_single_obs == 0 else '?'})")
        ck_in, c_in = int(model_dict["model"]["critic.0.weight"].shape[1]), self.model.critic[0].in_features
        if fresh_critic:
            ck_in = c_in
        ex_ck, ex_cfg = list(model_dict.get("privileged_extras", [])), list(getattr(self.env, "privileged_extras", ()))
        if ex_ck != ex_cfg:  # (before the width message below: groups of equal width, feet and ground, would pass it)
            raise ValueError(f"checkpoint {ck} was saved with env.privileged_extras = {ex_ck}, the config has env.privileged_extras = {ex_cfg}: the critic's "
                             f"privileged columns differ; set env.privileged_extras (and env.num_privileged_obs) as in the run that saved the checkpoint")
        if ck_in != c_in:  # (the critic's input: observations + privileged observations, with the terrain height scan 14 + P of the latter)
            raise ValueError(f"checkpoint {ck} has a critic of {ck_in} inputs, the config's critic takes {c_in} (env.num_observations + "
                             f"env.num_privileged_obs): terrain.measure_heights and its measured_points_x / measured_points_y must be as in the run "
                             "that saved the checkpoint")
        ck_a, ck_c = hidden_of(model_dict["model"], "actor"), hidden_of(model_dict["model"], "critic")
        if (ck_a, ck_c) != (self.actor_hidden, self.critic_hidden):
            raise ValueError(f"checkpoint {ck} has actor hidden widths {list(ck_a)} and critic hidden widths {list(ck_c)}, the config "
                             f"algorithm.actor_hidden = {list(self.actor_hidden)} and algorithm.critic_hidden = {list(self.critic_hidden)}: set these to the "
                             "checkpoint's widths")
        check_checkpoint(ck, model_dict.get("obs_normalizer"), self.obs_norm)  # (ValueError naming algorithm.empirical_normalization)
        if not getattr(self, "test", False):  # (a runner that plays never evaluates the critic: it loads such a checkpoint under either setting)
            check_value_checkpoint(ck, model_dict.get("value_normalizer"), getattr(self, "value_norm", None))  # (ValueError naming algorithm.normalize_value)
        self.model.load_state_dict({k: v for k, v in model_dict["model"].items() if not (fresh_critic and k.startswith("critic."))}, strict=False)
        self.invalidate()
        try:
            self.env.curriculum_prob = model_dict["curriculum"]
        except Exception as e:
            print(f"Failed to load curriculum: {e}")
        if self.env.terrain.curriculum:  # the levels (their origins and sum follow); a checkpoint without them, or of another env count, keeps the initial draw
            try:
                lv = model_dict["terrain_levels"]
                if tuple(lv.shape) != (self.env.num_envs,):
                    raise ValueError(f"shape {tuple(lv.shape)}, the env has {self.env.num_envs} envs")
                self.env.terrain_levels = lv
            except Exception as e:
                print(f"Failed to load terrain levels: {e!r}")
        try:
            self.optimizer.load_state_dict(model_dict["optimizer"])
        except Exception as e:
            print(f"Failed to load optimizer: {e}")
        if est is not None:
            try:
                self._est_opt.load_state_dict(model_dict["estimator"]["optimizer"])
            except Exception as e:
                print(f"Failed to load the estimator's optimizer: {e}")
        if getattr(self, "_rnd_trainer", None) is not None:
            self._rnd_trainer.load_state_dict(model_dict.get("rnd") or {})

    def invalidate(self):
        """Call after changing the model's parameters or the rollout buffers by any means other than this runner's own rollout() / update() (a
        checkpoint or test that loads weights, a tool that edits buffer["obses"] / buffer["actions"]).  The contract between the two phases:
        rollout() may leave the first mini-epoch's forward passes (activations, values, old mu, old log-probabilities of every row) in the trainers'
        buffers and the weight copies that the layer kernels read current, and update() then trusts both without looking; this forgets them (the
        clock of the parameters ticks: every copy of every trainer is stale), so the next update() recomputes everything from the parameters and the
        buffers as they are."""
        self._fwd_plan = None
        self._clock.tick()
        if self._est is not None:
            self._est_clock.tick()
        if getattr(self, "_rnd_clock", None) is not None:
            self._rnd_clock.tick()

    def checkpoint_dict(self):
        d = {"model": self.model.state_dict(), "optimizer": self.optimizer.state_dict(), "curriculum": self.env.curriculum_prob}
        if getattr(self, "_est", None) is not None:  # (the network itself: "estimator.*" inside "model")
            d["estimator"] = {"targets": list(self._est.targets), "optimizer": self._est_opt.state_dict()}
        if getattr(self, "_rnd_trainer", None) is not None:  # (the networks themselves: "rnd_predictor.*" and "rnd_target.*" inside "model")
            d["rnd"] = self._rnd_trainer.state_dict()
        if self.env.terrain.curriculum:
            d["terrain_levels"] = self.env.terrain_levels
        if self.obs_norm is not None:
            d["obs_normalizer"] = self.obs_norm.state_dict()
        if getattr(self, "value_norm", None) is not None:
            d["value_normalizer"] = self.value_norm.state_dict()
        if getattr(self.env, "num_scan_obs", 0):  # terrain.actor_heights: the grid of the scan at the end of the actor's row, for whoever deploys the actor
            d["height_points"] = self.env.height_points.clone()
        if getattr(self.env, "privileged_extras", ()):  # env.privileged_extras: the groups behind the critic's 14 + P columns, in the row's order
            d["privileged_extras"] = list(self.env.privileged_extras)
        return d

    # ------------------------------------------------------------------ one PPO iteration
    def _resolve_plan(self):
        """The UpdatePlan of the switches and shapes as they are now, handed to the trainers (MLPTrainer.plan) with the critic's value head."""
        ct, at = self._critic_tr, self._actor_tr
        sw = {k.lower(): getattr(MLPTrainer, k) for k in ("SPLIT", "FUSED", "CHAIN", "CHAIN_SPLIT", "CHAIN_SPLIT_BWD", "CHAIN_ALTERNATE", "FUSED_WGRAD", "WGRAD_SPLIT")}
        sw.update((k[1:], getattr(self, k)) for k in ("_one_stream", "_defer_finish", "_one_launch_tail", "_fused_opt", "_fused_head", "_fused_gae", "_chain_values",
                                                      "_rollout_forward", "_gru_group"))
        sw["value_norm"] = self.value_norm is not None
        widths = lambda tr: (tr.layers[0].in_features,) + tuple(l.out_features for l in tr.layers)
        kin_a = self._actor_in.shape[-1] if self._actor_in is not None else self.env.num_obs + self._est_cols  # (the actor's true input width)
        if self._mem_tr is not None:  # the trunk's input is the cell's state [B][H], not the padded observation rows (those are the cell's)
            kin_a = self._memory
        kin_c = self._critic_in.shape[-1]
        cmem = self._rnn_critic if self._cmem_tr is not None else 0
        if cmem:  # likewise the critic's trunk behind its cell
            kin_c = cmem
        plan = plan_update((widths(ct), kin_c), (widths(at), kin_a), self._old_logp.numel(), dp_active=self.dp.active, symmetry=self._symmetry,
                           memory=self._memory if self._mem_tr is not None else 0, smoothness=self._smooth, critic_memory=cmem, **sw)
        ct.plan, at.plan = plan.critic, plan.actor
        c_out = ct.layers[-1]
        ct.value_head = (c_out.weight.reshape(-1), c_out.bias, self._values_all) if plan.chain_values else None
        if self._mini_batches > 1 or self._env_mini_batches > 1:
            # runner.num_mini_batches / num_env_mini_batches: the plan above serves the whole-batch passes (forward-ahead, old mu, values + GAE); the K
            # optimiser steps of a mini-epoch run a plan of their own for b = B / K rows on the second pair of trainers
            mp = self._mb_plan = plan_update((widths(ct), kin_c), (widths(at), kin_a), self._mb_rows, dp_active=self.dp.active,
                                             memory=self._memory if self._env_mini_batches > 1 else 0, critic_memory=cmem if self._env_mini_batches > 1 else 0, **sw)
            self._critic_mb.plan, self._actor_mb.plan = mp.critic, mp.actor
            self._critic_mb.value_head = (c_out.weight.reshape(-1), c_out.bias, self._mb_values) if mp.chain_values else None
        return plan

    # ------------------------------------------------------------------ runner.num_mini_batches > 1
    def _init_mini_batches(self):
        """What K = runner.num_mini_batches > 1 adds to the runner: a second pair of trainers over the same Linear modules, sized for b = B / K rows (they
        share the parameters and the .grad views of the flat Adam buffer; a trainer reallocates its workspaces and weight planes when its row count
        changes, so the whole-batch pair is never flipped to b rows), the permutation and the gathered copies of every per-row stream the steps read."""
        K, B, A, dev = self._mini_batches, self._old_logp.numel(), self.env.num_actions, self.device
        b = self._mb_rows = B // K
        self._actor_mb, self._critic_mb = MLPTrainer(self.model.actor, clock=self._clock), MLPTrainer(self.model.critic, clock=self._clock)
        # the grouped weight-gradient launch keeps its descriptors per input buffer: one per mini-batch position (static after the first mini-epoch)
        self._mb_wgrad = [GroupedWeightGrad() for _ in range(K)]
        self._perm = torch.zeros(B, dtype=torch.int32, device=dev)
        ka = self._actor_in.shape[-1] if self._actor_in is not None else self.env.num_obs
        f = lambda *shape: torch.zeros(*shape, device=dev)
        self._mb = types.SimpleNamespace(critic_in=f(B, self._critic_in.shape[-1]), actor_in=f(B, ka), actions=f(B, A), old_mu=f(B, A), old_logp=f(B), adv=f(B), ret=f(B))
        self._mb_values = f(b)
        self._mb_updates = 0  # the update counter of the permutation's key

    def permutation(self, update, epoch, out=None):
        """The permutation of [0, B) that mini-epoch `epoch` of this rank's update number `update` shuffles its rows with (bg_perm_fill), as an int32
        device tensor: keyed by (basic.seed with the rank folded in as in the rollout's action noise, update, epoch)."""
        return self._perm_fill(torch.empty_like(self._perm) if out is None else out, update, epoch)

    def env_permutation(self, update, epoch, out=None):
        """The permutation of the envs [0, N) that mini-epoch `epoch` of this rank's update number `update` cuts into runner.num_env_mini_batches
        mini-batches of whole sequences, as an int32 device tensor: the key rule of permutation(), over N in place of B."""
        return self._perm_fill(torch.empty_like(self._env_perm) if out is None else out, update, epoch)

    def _perm_fill(self, out, update, epoch):
        seed = (int(self.cfg["basic"]["seed"]) + 1000003 * (self.rank + 1)) & 0xFFFFFFFFFFFFFFFF
        _lib.check(_lib.load().bg_perm_fill(out.numel(), seed, int(update) & 0xFFFFFFFF, int(epoch), _lib.ptr(out), _lib.current_stream_ptr()), "bg_perm_fill")
        return out

    def _mini_batch_begin(self, u):
        """Once per update(): the K optimiser steps of a mini-epoch run on the mini-batch trainers under their own plan, step k on rows [k b, (k + 1) b)
        of the gathered buffers; the CU shares of their launches are sized for b-row slabs; the descriptors of the gather."""
        m, b, w = self._mb, self._mb_rows, u.whole
        u.steps = [StepRows(self._critic_mb, self._actor_mb, self._mb_plan, b, self._mb_wgrad[k], m.critic_in[r], None, m.actor_in[r], m.actions[r], m.old_mu[r],
                            m.old_logp[r], m.adv[r], m.ret[r], self._mb_values) for k, r in enumerate(slice(k * b, (k + 1) * b) for k in range(self._mini_batches))]
        self._plan_chain_split(u.steps[0].x_c, u.steps[0].x_a, self._mb_plan, self._critic_mb, self._actor_mb)
        # the whole-batch passes of this update run one network at a time (old mu; the critic's values): one workgroup per slab, no CU share
        self._critic_tr.chain_workgroups = self._actor_tr.chain_workgroups = 0
        B = u.B
        pairs = [(w.x_c[:B], m.critic_in), (w.x_a[:B], m.actor_in), (w.actions, m.actions), (w.old_mu, m.old_mu), (w.old_logp, m.old_logp), (w.adv, m.adv),
                 (w.ret, m.ret)]
        for src, dst in pairs:
            if not (src.is_contiguous() and src.dtype == torch.float32 and src.shape == dst.shape):
                raise RuntimeError(f"mini-batch gather: a stream of shape {tuple(src.shape)} does not match its buffer {tuple(dst.shape)}")
        u.gather = (_lib.GatherStream * len(pairs))(*[_lib.GatherStream(src.data_ptr(), dst.data_ptr(), src.numel() // B, 0) for src, dst in pairs])
        u.gather_keep = pairs

    def _shuffle(self, u, epoch):
        """A fresh permutation of the batch's rows and ONE gather of every per-row stream the K steps read, mini-batch after mini-batch."""
        self.permutation(self._mb_updates, epoch, out=self._perm)
        _lib.check(_lib.load().bg_gather_rows(u.B, u.B, _lib.ptr(self._perm), u.gather, len(u.gather), _lib.current_stream_ptr()), "bg_gather_rows")

    # ------------------------------------------------------------------ runner.num_env_mini_batches > 1
    def _init_env_mini_batches(self):
        """What K = runner.num_env_mini_batches > 1 adds to the runner, after _init_mini_batches: the second pair of trainers sized for b = T n rows,
        n = N / K, a second cell trainer around that pair's actor for [T][n] rows, the permutation of the envs, and the gathered copies of everything
        the steps read: the seven per-row streams, the recurrence's starting state [K][n][H] and its reset flags [K][T][n]."""
        K, A, H, dev = self._env_mini_batches, self.env.num_actions, self._memory, self.device
        T, N = self.cfg["runner"]["horizon_length"], self.env.num_envs
        B, n = T * N, N // K
        self._mb_rows = T * n
        self._actor_mb, self._critic_mb = MLPTrainer(self.model.actor, clock=self._clock), MLPTrainer(self.model.critic, clock=self._clock)
        self._mem_mb = GRUTrainer(self.model.memory, self._actor_mb, T, n, clock=self._clock, bias_partial=True)
        # algorithm.rnn_critic: likewise a second trainer of the critic's cell for [T][n] rows (a step differentiates all of its rows: no extra step)
        self._cmem_mb = None
        if self._cmem_tr is not None:
            self._cmem_mb = GRUTrainer(self.model.critic_memory, self._critic_mb, T, n, clock=self._clock, bias_partial=True, kin=self._pad_critic)
        self._mb_wgrad = [GroupedWeightGrad() for _ in range(K)]  # (descriptors per input buffer: one per mini-batch position)
        self._env_perm = torch.zeros(N, dtype=torch.int32, device=dev)
        f = lambda *shape: torch.zeros(*shape, device=dev)
        self._mb = types.SimpleNamespace(critic_in=f(B, self._critic_in.shape[-1]), actor_in=f(B, GRUTrainer.KIN), actions=f(B, A), old_mu=f(B, A), old_logp=f(B),
                                         adv=f(B), ret=f(B), h0=f(N, H), resets=torch.zeros(B, dtype=torch.uint8, device=dev),
                                         h0_c=f(N, H) if self._cmem_tr is not None else None)
        self._mb_values = f(self._mb_rows)
        self._mb_updates = 0  # the update counter of the permutation's key

    def _env_mini_batch_begin(self, u):
        """Once per update(), as _mini_batch_begin: step k runs on rows [k b, (k + 1) b) of the gathered buffers -- the T steps of the n envs
        sigma[k n : (k + 1) n], step-major -- with the cell trainer of b rows from the gathered state h0[k] and reset flags resets[k]; the descriptors
        of the gather (nine streams: seven per row, the state per env, the one-byte reset flags; with a recurrent critic a tenth, its state per env:
        the first T rows of its reset flags are the actor's)."""
        m, b, w, K, T = self._mb, self._mb_rows, u.whole, self._env_mini_batches, u.T
        n = u.N // K
        u.steps = [StepRows(self._critic_mb, self._actor_mb, self._mb_plan, b, self._mb_wgrad[k], m.critic_in[r], None, m.actor_in[r], m.actions[r], m.old_mu[r],
                            m.old_logp[r], m.adv[r], m.ret[r], self._mb_values, CellRows(self._mem_mb, m.h0[k * n : (k + 1) * n], m.resets[r].view(T, n)),
                            None if self._cmem_mb is None else CellRows(self._cmem_mb, m.h0_c[k * n : (k + 1) * n], m.resets[r].view(T, n)))
                   for k, r in enumerate(slice(k * b, (k + 1) * b) for k in range(K))]
        self._plan_chain_split(u.steps[0].x_c, u.steps[0].x_a, self._mb_plan, self._critic_mb, self._actor_mb)
        self._critic_tr.chain_workgroups = self._actor_tr.chain_workgroups = 0  # the whole-batch passes run one network at a time
        B, whole = u.B, w.mem
        streams = [(w.x_c[:B], m.critic_in, 0), (w.x_a[:B], m.actor_in, 0), (w.actions, m.actions, 0), (w.old_mu, m.old_mu, 0), (w.old_logp, m.old_logp, 0),
                   (w.adv, m.adv, 0), (w.ret, m.ret, 0), (whole.h0, m.h0, 1), (whole.resets.view(B), m.resets, 0)]
        if w.cmem is not None:
            streams.append((w.cmem.h0, m.h0_c, 1))
        for src, dst, _ in streams:
            if not (src.is_contiguous() and src.dtype == dst.dtype and src.dtype in (torch.float32, torch.uint8) and src.shape == dst.shape):
                raise RuntimeError(f"env mini-batch gather: a stream of shape {tuple(src.shape)} ({src.dtype}) does not match its buffer {tuple(dst.shape)} ({dst.dtype})")
        u.gather = (_lib.SequenceStream * len(streams))(*[_lib.SequenceStream(src.data_ptr(), dst.data_ptr(), src.numel() // src.shape[0], src.element_size(), per_env, 0)
                                                          for src, dst, per_env in streams])
        u.gather_keep = streams

    def _shuffle_envs(self, u, epoch):
        """A fresh permutation of the envs and ONE gather of everything the K steps read, mini-batch after mini-batch."""
        self.env_permutation(self._mb_updates, epoch, out=self._env_perm)
        _lib.check(_lib.load().bg_gather_sequences(u.T, u.N, self._env_mini_batches, _lib.ptr(self._env_perm), u.gather, len(u.gather), _lib.current_stream_ptr()),
                   "bg_gather_sequences")

    def rollout(self):
        """runner.py:106-121: horizon_length env steps with sampled actions, outputs written in place.

        While the simulator steps -- one wave per CU on half of the CUs, latency-bound -- the side stream evaluates what the FIRST mini-epoch of the
        update needs and what does not change until the first optimiser step: the critic's hidden layers and values (runner.py:123-125, 132) and the
        actor's hidden layers and old mu (runner.py:126-129) on each step's 4,096 rows as soon as they exist, with the kernels and weights the
        update would use (32 slabs per network and step on the idle CUs: bit-identical to the full-batch launches, asserted in
        tests/test_gpu_ppo.py), and the old log-probabilities one step behind.  update() then starts at the GAE: no old-mu pass, no forward chains
        in mini-epoch 0.  Nothing on the main stream waits for the side stream here; update()'s own hand-overs order the two."""
        buf, T = self.buffer, self.cfg["runner"]["horizon_length"]
        obses, priv = buf["obses"], buf["privileged_obses"]
        seed = int(self.cfg["basic"]["seed"]) + 1000003 * (self.rank + 1)
        plan = self._resolve_plan()
        if plan.ahead:
            N = self.env.num_envs
            self._critic_tr.prepare(self._critic_in.reshape((T + 1) * N, -1), train_rows=T * N)
            self._actor_tr.prepare(self._actor_in.reshape(T * N, -1))
        main = torch.cuda.current_stream()
        g, start = self._rollout_group, 0
        norm = self.obs_norm
        scan = getattr(self.env, "num_scan_obs", 0)  # terrain.actor_heights: the rows end with the height scan
        with torch.no_grad():
            # the default actor samples from a packed copy of its parameters: laid out here, once for the T steps and in every rollout (whatever changed
            # the parameters since the last one -- optimiser, checkpoint, broadcast -- is behind this launch on the stream); None for other architectures
            packed = self.model.pack_actor()
            mt = self._mem_tr
            if mt is not None:  # a recurrent actor: the state the update's recurrence starts from = the state as the last rollout left it
                mt.rollout_begin(self.model.memory_state(self.env.num_envs, obses.device), self._last_dones)
            cm = self._cmem_tr
            if cm is not None:  # a recurrent critic: the state its last update carried over (GRUTrainer.carry_state), the same flags
                cm.rollout_begin(cm.next_state, self._last_dones)
            rt = self._rnd_trainer
            if rt is not None:
                rt.begin_rollout()  # this iteration's weight
            for n in range(T):
                if plan.ahead and n + 1 - start >= g:
                    self._forward_rows(start, n, main)  # rows of steps start .. n: on the side stream, beside this step's launches
                    start = n + 1
                if self._est is not None:  # estimator and actor in ONE launch; the estimate the actor read is kept: the update's rows are these
                    self.model.sample_actions(obses[n], buf["actions"][n], seed, self._act_counter, est_out=buf["estimates"][n])
                elif mt is not None:  # cell and trunk in ONE launch that advances the state in place; an env the step before reset enters with a zero state
                    self.model.sample_actions(obses[n], buf["actions"][n], seed, self._act_counter, reset=mt.rollout_reset(n, self._last_dones, buf["dones"]))
                elif norm is None:
                    self.model.sample_actions(obses[n], buf["actions"][n], seed, self._act_counter, scan=scan, packed=packed)
                else:  # the buffer keeps the raw rows; the actor samples from their normalised copy (one more launch per step: bg_obs_normalize)
                    self.model.sample_actions(norm.normalize_into(obses[n], self._obs_normed), buf["actions"][n], seed, self._act_counter, scan=scan,
                                              packed=packed)
                self._act_counter += 1
                self.env.step_to(buf["actions"][n], obses[n + 1], priv[n + 1], buf["rewards"][n], buf["dones"][n], buf["time_outs"][n])
                if rt is not None:  # both RND networks on the state the step has just written, the add into its reward in place: ONE launch
                    rt.reward(obses[n + 1], priv[n + 1], buf["dones"][n], buf["rnd_targets"][n], buf["intrinsic_rewards"][n], buf["rewards"][n])
            if plan.ahead:
                self._forward_rows(start, T, main)  # ... and the observation after the last step: the critic's last_values rows
            if cm is not None:
                cm.rollout_end(buf["dones"])
            if mt is not None:
                mt.rollout_end(buf["dones"], self._last_dones)
        self._fwd_plan = plan if plan.ahead else None

    def _forward_rows(self, a, b, main):
        """Side stream: pad the observation rows of steps a .. b (b = T: the observation after the last step, critic only) into the network inputs
        and run both networks' chained forward (+ value head, + the actor's output layer = old mu) on them; old log-probabilities of the steps
        whose actions have been sampled by now.  A row block exists once the env step before it has finished: the side stream waits for the main
        stream's work enqueued so far."""
        T, N = self.cfg["runner"]["horizon_length"], self.env.num_envs
        no, npv = self.env.num_obs, self.env.num_privileged_obs
        buf, side = self.buffer, self._side_stream
        ct, at = self._critic_tr, self._actor_tr
        ba = min(b, T - 1)  # last actor step of the range
        side.wait_stream(main)
        with torch.cuda.stream(side), torch.no_grad():
            logstd = self.model.logstd.reshape(-1)
            if a == 0:  # weights may have changed since the last optimiser step by other means (checkpoint, broadcast): six small copies, off the critical path
                ct.copies.rewrite_all(); at.copies.rewrite_all()
                self._logp_done = 0
            if self._logp_done < a:  # steps of earlier calls: their actions were sampled on the main stream after their rows were enqueued here
                r0, r1 = self._logp_done * N, a * N
                gaussian_logp(self._old_mu[r0:r1], logstd, buf["actions"][self._logp_done : a].reshape(-1, self.env.num_actions), out=self._old_logp[r0:r1])
                self._logp_done = a
            if self.obs_norm is not None:  # (valid ahead of the update: the statistics change only at its end)
                self._normalize_inputs(a, b + 1, ba + 1)
            else:
                self._critic_in[a : b + 1, :, :no].copy_(buf["obses"][a : b + 1])
                self._critic_in[a : b + 1, :, no : no + npv].copy_(buf["privileged_obses"][a : b + 1])
            jobs = [(ct, a * N, (b + 1 - a) * N)]
            if a <= ba:
                if self.obs_norm is None:
                    self._actor_in[a : ba + 1, :, :no].copy_(buf["obses"][a : ba + 1])
                jobs.append((at, a * N, (ba + 1 - a) * N))
            MLPTrainer.launch_chain([tr.chain_rows_descriptor(r0, nr) for tr, r0, nr in jobs])  # ONE launch (at most 4 jobs)
            if a <= ba:
                a_out = at.layers[-1]
                actor_head_forward(at.acts[2][a * N : (ba + 1) * N], a_out.weight, a_out.bias, self._old_mu[a * N : (ba + 1) * N])
            if b == T and self._logp_done < T:  # the last call: every action has been sampled
                r0 = self._logp_done * N
                gaussian_logp(self._old_mu[r0:], logstd, buf["actions"][self._logp_done :].reshape(-1, self.env.num_actions), out=self._old_logp[r0:])
                self._logp_done = T

    def _partner_rows(self, T, epoch):
        """algorithm.smoothness_loss: rows [B, 2B) of the actor's input from rows [0, B) and the rows of the step after the last (bg_partner_rows), on the
        current stream.  The draw of pairs "interpolate" is keyed by basic.seed with the rank folded in as in permutation(), this rank's update number and
        the mini-epoch."""
        buf, seed = self.buffer, int(self.cfg["basic"]["seed"]) + 1000003 * (self.rank + 1)
        partner_rows(self._actor_in[:T], self._actor_last, buf["dones"], buf["time_outs"], self._actor_in[T:], self._smooth_pairs, seed, self._smooth_updates, epoch)

    def _normalize_inputs(self, a, b, b_actor):
        """algorithm.empirical_normalization: the padded network inputs of steps [a, b) (critic: observation and privileged block) and [a, b_actor)
        (actor) from the raw rows of the experience buffer through bg_obs_normalize, on the current stream, in place of the copies; with the
        statistics as they are (they change only at the end of update()); the padded columns stay zero."""
        buf, no, norm = self.buffer, self.env.num_obs, self.obs_norm
        ci, ai = self._critic_in, self._actor_in
        norm.normalize_into(buf["obses"][a:b], ci[a:b, :, :no])
        norm.normalize_into(buf["privileged_obses"][a:b], ci[a:b, :, no:], col0=no, dst_cols=ci.shape[-1] - no)
        if ai is not None and a < b_actor:
            norm.normalize_into(buf["obses"][a:b_actor], ai[a:b_actor], dst_cols=ai.shape[-1])

    def update(self):
        """runner.py:123-189: old log-probs, then mini_epochs full-batch optimiser steps.

        Contract with rollout(): when rollout() has run the first mini-epoch's forward passes under the plan this update resolves (`_fwd_plan`), this
        method starts from them and from the weight copies the last optimiser launch wrote -- parameters and rollout buffers must not have been changed
        in between except through `invalidate()` (which `_load` and the initial broadcast call)."""
        u = self._update_begin(self._resolve_plan())
        # K steps per mini-epoch: on shuffled rows (runner.num_mini_batches) or on the sequences of shuffled envs (runner.num_env_mini_batches), never both
        K, w = max(self._mini_batches, self._env_mini_batches), u.whole
        if self._mini_batches > 1:
            self._mini_batch_begin(u)
            shuffle = self._shuffle
        elif K > 1:
            self._env_mini_batch_begin(u)
            shuffle = self._shuffle_envs
        with torch.no_grad():
            for epoch in range(self.cfg["runner"]["mini_epochs"]):
                # this mini-epoch's hidden activations and values may be the rollout's: same kernels, same weights
                have_fwd = u.ahead and epoch == 0
                if u.plan.smoothness and self._smooth_pairs == "interpolate":  # a fresh draw per row in front of every mini-epoch's forward pass
                    self._partner_rows(u.T, epoch)
                if K == 1 and not u.plan.one_stream:
                    self._epoch_on_two_streams(u, have_fwd)  # the same pieces, the critic's on the side stream beside the actor's
                    self._epoch_gradients_and_step(u, w)
                    continue
                # Per mini-epoch: the whole-batch values, returns and advantages from the current critic; then the optimiser steps, each on its rows (K = 1:
                # one step on the whole batch; runner.num_mini_batches = K: on disjoint shuffled K-ths of it -- returns and advantages stay fixed for the
                # K steps, the KL rule moves the learning rate after every one of them; runner.num_env_mini_batches = K: likewise on the whole sequences
                # of disjoint shuffled K-ths of the envs).  Every launch on the main stream.
                hc = ha = None
                if have_fwd:
                    u.main.wait_stream(u.side)  # the rollout ran the forward passes on the side stream
                    hc, ha = w.ct.acts[2], w.at.acts[2]
                elif K == 1:
                    hc, ha = self._forward_hidden(w)  # the one step's rows are the values pass's: both networks' forward passes as its grouped launch
                hc, v_all = self._whole_batch_values(u, hc)
                if K > 1:
                    shuffle(u, epoch)
                for v in u.steps:
                    self._step(u, v, (hc, ha, v_all[: u.B]) if K == 1 else None)
                    self._epoch_gradients_and_step(u, v)
            if self.obs_norm is not None:
                # behind the last optimiser step: this iteration's T x N rows enter the statistics (row T is the next iteration's row 0), under data
                # parallelism all ranks' rows through ONE float64 exchange (tag "obs_norm", main stream, behind the last "bucket": utils/parallel.py)
                self.obs_norm.update_from(u.buf["obses"][: u.T], u.buf["privileged_obses"][: u.T], self.dp)
            if u.plan.value_norm:
                # behind the last optimiser step (and "obs_norm"): the last mini-epoch's un-normalised returns enter the statistics, all ranks' through
                # ONE float64 exchange (tag "value_norm", main stream); merge and fp32 triple in one small launch, no host read
                self.value_norm.update_from(dp=self.dp)
            if self._rnd_trainer is not None:
                # behind the last PPO optimiser step (in front of the estimator's): the predictor on the iteration's successor rows, then the reward
                # normaliser's move; the next rollout runs on both
                self._rnd_trainer.update(u.buf["obses"][1:], u.buf["privileged_obses"][1:], u.buf["dones"], u.buf["rnd_targets"], u.buf["intrinsic_rewards"])
            if self._est is not None:
                # behind the last PPO optimiser step: the next rollout runs the estimator trained on this iteration's rows
                self._est_trainer.update(u.buf["obses"][: u.T], u.buf["privileged_obses"][: u.T])
        if K > 1:
            self._mb_updates += 1
        if u.plan.smoothness:
            self._smooth_updates += 1
        return self._stats_acc

    def _update_begin(self, plan):
        """What update() does once per call: inputs of both networks, old mu / log-std / log-probabilities (runner.py:123-129) unless rollout() left them,
        zeroed accumulators, the CU split of the forward launches.  Returns the namespace the three phases of a mini-epoch share."""
        cfg, buf = self.cfg, self.buffer
        T, N = cfg["runner"]["horizon_length"], self.env.num_envs
        B, A = T * N, self.env.num_actions
        alg = cfg["algorithm"]
        act_flat = buf["actions"].reshape(B, A)
        no, npv = self.env.num_obs, self.env.num_privileged_obs
        # rollout() may have run the first mini-epoch's forward passes already (activations, values and old mu of every row are in place); they
        # serve only the plan they were computed under
        ahead, self._fwd_plan = self._fwd_plan == plan, None
        if not ahead:
            torch.cuda.current_stream().wait_stream(self._side_stream)  # a forward-ahead being discarded may still write these buffers
            self._clock.tick()  # weights may have changed outside the loop below (checkpoint, broadcast): every weight copy is stale
            if self.obs_norm is not None:
                self._normalize_inputs(0, T + 1, T)
            else:
                self._critic_in[:, :, :no].copy_(buf["obses"])
                self._critic_in[:, :, no : no + npv].copy_(buf["privileged_obses"])
                if self._actor_in is not None:
                    self._actor_in[:T, :, :no].copy_(buf["obses"][:T])
            if self._est is not None and self._actor_in is not None:
                # the estimate is an observation: the stored rows [obses | estimates[:E] | 0], so old mu and the first ratio come from what the rollout acted on
                self._actor_in[:T, :, no : no + self._est_cols].copy_(buf["estimates"][..., : self._est_cols])
            if plan.smoothness:
                # the actor's rows of obses[T], as the network sees them (padded, normalised), then rows [B, 2B): every row's successor -- pairs
                # "next": copies, once per update; "interpolate": a fresh draw in front of every mini-epoch's forward pass (update(); the old-mu
                # pass below reads rows [0, B) only)
                if self.obs_norm is not None:
                    self.obs_norm.normalize_into(buf["obses"][T], self._actor_last, dst_cols=self._actor_last.shape[-1])
                else:
                    self._actor_last[:, :no].copy_(buf["obses"][T])
                if self._smooth_pairs == "next":
                    self._partner_rows(T, 0)
            elif plan.symmetry and self.obs_norm is not None:  # rows [B, 2B): normalise(M_o x), what the policy computes on the mirrored raw observation
                mirror_rows(buf["obses"][:T].reshape(B, -1), self._mirror_raw, *self._obs_mirror_raw)
                self.obs_norm.normalize_into(self._mirror_raw, self._actor_in[T:].reshape(B, -1), dst_cols=self._actor_in.shape[-1])
            elif plan.symmetry:  # rows [B, 2B): the mirror images M_o x of the batch
                mirror_rows(self._actor_in[:T].reshape(B, -1), self._actor_in[T:].reshape(B, -1), *self._obs_mirror)
        if self._actor_in is not None:
            obs_flat = self._actor_in.reshape(-1, self._actor_in.shape[-1])
        elif self.obs_norm is not None:  # (no padded input: the per-layer library path reads the normalised rows from a copy of its own)
            obs_flat = self.obs_norm.normalize_into(buf["obses"][:T].reshape(B, -1), torch.empty(B, no, device=self.device))
        elif self._est is not None:  # (no padded input: the library path reads the concatenated rows from a copy of its own)
            obs_flat = torch.cat((buf["obses"][:T], buf["estimates"][..., : self._est_cols]), dim=-1).reshape(B, -1)
        else:
            obs_flat = buf["obses"][:T].reshape(B, -1)
        critic_all = self._critic_in.reshape((T + 1) * N, -1)  # rows [B, B+N) = the observation after the last step (last_values)
        logstd_flat = self.model.logstd.reshape(-1)
        a_out, c_out = self._actor_tr.layers[-1], self._critic_tr.layers[-1]
        with torch.no_grad():
            # old mu through the same kernels as the mini-epochs: the first ratio is exactly 1
            ha0 = None
            if ahead:
                old_mu = self._old_mu
            elif self._mem_tr is not None:  # ... the cell over the T steps from h0, then the trunk; mini-epoch 0 reuses this pass (no parameter changes in
                # between; not under runner.num_env_mini_batches: a step's rows are not these)
                ha0 = self._actor_hidden(self._actor_tr, obs_flat, self._whole_cell())
                old_mu = actor_head_forward(ha0[:B], a_out.weight, a_out.bias, self._old_mu)
            elif plan.fused_head:
                old_mu = actor_head_forward(self._actor_tr.forward_hidden(obs_flat)[:B], a_out.weight, a_out.bias, self._old_mu)
            else:
                old_mu = self._actor_tr.forward(obs_flat).clone()
            old_logstd = self.model.logstd.detach().reshape(-1).clone()
            if not ahead:
                gaussian_logp(old_mu, old_logstd, act_flat, out=self._old_logp)
        self._stats_acc.zero_()
        self._stats.zero_()
        self._grad_logstd.zero_()
        self._plan_chain_split(critic_all, obs_flat, plan)
        whole = StepRows(self._critic_tr, self._actor_tr, plan, B, self._wgrad_group, critic_all, B, obs_flat, act_flat, old_mu, self._old_logp, self._adv.view(B),
                         self._ret.view(B), self._values_all, self._whole_cell(), self._whole_critic_cell())
        # whole: the batch as the rows of one optimiser step; steps: what the steps of a mini-epoch run on (runner.num_mini_batches > 1: _mini_batch_begin)
        return types.SimpleNamespace(cfg=cfg, buf=buf, T=T, N=N, B=B, alg=alg, ahead=ahead, plan=plan, logstd_flat=logstd_flat, old_logstd=old_logstd,
                                     main=torch.cuda.current_stream(), side=self._side_stream, mirrors=None, whole=whole, steps=[whole], ha0=ha0,
                                     carry=self._cmem_tr is not None)

    # ------------------------------------------------------------------ the pieces of a mini-epoch, each on the rows of a StepRows, on the current stream
    def _whole_cell(self):
        """The CellRows of the whole batch: the cell's trainer with its own state and reset flags (None: a feed-forward actor)."""
        mt = self._mem_tr
        return None if mt is None else CellRows(mt, mt.h0, mt.resets)

    def _whole_critic_cell(self):
        """The CellRows of the whole batch's critic: its cell's trainer, over T + 1 steps, with its own state and reset flags (None: a feed-forward critic)."""
        cm = self._cmem_tr
        return None if cm is None else CellRows(cm, cm.h0, cm.resets)

    @staticmethod
    def _critic_hidden(v):
        """The critic's last hidden activations on v's rows; with a recurrent critic x_c are the cell's padded rows: the cell first (GRUTrainer.forward from
        the rows' h0 with their resets), then the trunk on h, which differentiates the first train_rows rows."""
        if v.cmem is None:
            return v.ct.forward_hidden(v.x_c, train_rows=v.train_rows)
        return v.ct.forward_hidden(v.cmem.trainer.forward(v.x_c, v.cmem.h0, v.cmem.resets), train_rows=v.train_rows)

    @staticmethod
    def _critic_backward_hidden(ct, fins, cmem):
        """The critic's backward-data pass; with a recurrent critic the trunk's, then the cell's through the T steps (truncated at h0)."""
        ct.backward_hidden(finishes=fins)
        if cmem is not None:
            cmem.trainer.backward(finishes=fins)

    @staticmethod
    def _actor_hidden(at, x, mem):
        """The actor's last hidden activations on the rows x; with a recurrent actor (mem: the rows' CellRows) x are the cell's padded [rows][64] rows:
        gi on all of them, the recurrence from the rows' h0 with their resets (GRUTrainer.forward), then the trunk on h."""
        return at.forward_hidden(x if mem is None else mem.trainer.forward(x, mem.h0, mem.resets))

    @staticmethod
    def _actor_backward_hidden(at, fins, mem):
        """The actor's backward-data pass; with a recurrent actor the trunk's, then the cell's through time (GRUTrainer.backward: truncated at h0), whose
        bias gradients join the deferred reductions."""
        at.backward_hidden(finishes=fins)
        if mem is not None:
            mem.trainer.backward(finishes=fins)

    def _forward_hidden(self, v):
        """The hidden layers of both networks on v's rows: one grouped launch, or one pass per network.  Returns their last hidden activations."""
        if v.plan.one_stream:
            return MLPTrainer.forward_hidden_group([(v.ct, v.x_c, v.train_rows), (v.at, v.x_a, None)])
        if v.plan.gru_group and v.mem is not None and v.cmem is not None:  # both cells' recurrences as ONE launch, then both trunks
            h_c, h_a = GRUTrainer.forward_group([(v.cmem.trainer, v.x_c, v.cmem.h0, v.cmem.resets), (v.mem.trainer, v.x_a, v.mem.h0, v.mem.resets)])
            return v.ct.forward_hidden(h_c, train_rows=v.train_rows), v.at.forward_hidden(h_a)
        return self._critic_hidden(v), self._actor_hidden(v.at, v.x_a, v.mem)

    def _head_values(self, v, hc):
        """The critic's values of v.x_c's rows in v.values: left there by the chained forward launch's value head (plan.chain_values: from the registers
        that hold the last activations, so that the launch between the critic's forward and the actor's loss has 400 KB to read instead of 52 MB), or
        the output layer on the stored activations hc."""
        c_out = v.ct.layers[-1]
        return v.values if v.plan.chain_values else critic_head_forward(hc, c_out.weight, c_out.bias, v.values)

    def _whole_batch_values(self, u, hc):
        """The whole-batch pass of a mini-epoch (runner.py:132-145): the critic on all (T + 1) N rows with the current weights, time-out bootstrap, GAE,
        returns, advantage moments and their exchange.  hc: the critic's last hidden activations where a forward pass has left them (the rollout's
        forward-ahead in mini-epoch 0, the grouped launch of both networks), None: the pass runs here.  Returns hc and the values of all rows."""
        v, plan, buf, alg, T, N, B = u.whole, u.plan, u.buf, u.alg, u.T, u.N, u.B
        if plan.fused_head and hc is None:
            hc = self._critic_hidden(v)
            if u.carry:  # a recurrent critic's first pass of the update, on the parameters the rollout ran on: the state the next iteration starts from
                v.cmem.trainer.carry_state()
                u.carry = False
        if plan.fused_head and plan.fused_gae:
            # output layer + timeout bootstrap + GAE + returns + advantage moments in ONE launch in front of the actor's loss
            c_out = v.ct.layers[-1]
            if plan.value_norm:  # v.values keeps the critic's standardised output u, _ret receives the standardised returns: the loss head's operands
                v_all = critic_values_gae_norm(None if plan.chain_values else hc, c_out.weight, c_out.bias, buf["rewards"], buf["dones"], buf["time_outs"],
                                               alg["gamma"], alg["lam"], v.values, self._adv, self._ret, self.value_norm.stats, self.value_norm.sums,
                                               self._gae_scratch)
            else:
                v_all = critic_values_gae(None if plan.chain_values else hc, c_out.weight, c_out.bias, buf["rewards"], buf["dones"], buf["time_outs"], alg["gamma"],
                                          alg["lam"], v.values, self._adv, self._ret, self._adv_sums, self._gae_scratch)
        else:
            v_all = self._head_values(v, hc) if plan.fused_head else v.ct.forward(v.x_c, train_rows=v.train_rows).squeeze(-1)
            gae(buf["rewards"], buf["dones"], buf["time_outs"], v_all[:B].view(T, N), v_all[B:], alg["gamma"], alg["lam"], advantages=self._adv,
                returns=self._ret, sums=self._adv_sums)
        self.dp.sum_(self._adv_sums, tag="moments")  # exchange (1)
        return hc, v_all

    # Output layers fused with the loss (bg_head.hip): per network ONE pass over the [rows][128] hidden activations gives the output, the loss terms,
    # dL/dz of the hidden layer and the output layer's gradients.  Both heads add into _stats, which the previous optimiser step zeroed (before the
    # loop for the first).  plan.defer (the default, see __init__): the small fixed-order reductions behind the head kernels and behind every backward
    # layer (output-layer and bias gradients, loss statistics: nothing a chain needs) are left as descriptors and run as ONE launch in front of the
    # weight-gradient launch (bg_reduce_group, or inside bg_update_tail) instead of inside the chains.
    @staticmethod
    def _deferred_finishes(plan):
        """(fins, fin_c, fin_a): the list the backward passes append their descriptors to and those of the critic's and the actor's head."""
        return ([], _lib.ReduceProblem(), _lib.ReduceProblem()) if plan.defer else (None, None, None)

    def _critic_loss_head(self, v, hc, values, finish):
        """The critic's output layer fused with the value loss and its backward (runner.py:148) on the last hidden activations hc."""
        ct, c_out = v.ct, v.ct.layers[-1]
        critic_head_backward(hc[: v.rows], c_out.weight, values, v.ret, ct.hidden_grad, c_out.weight.grad, c_out.bias.grad, ct.layers[-2].bias.grad, self._stats,
                             self._head_scratch_c, finish=finish)

    def _actor_loss_head(self, u, v, ha, finish):
        """The actor's output layer fused with its loss and backward (runner.py:145-161) on the last hidden activations ha: bg_actor_head, or with the
        mirror-symmetry loss bg_actor_head_sym on the 2B rows of ha (the batch, then its mirror images).  The advantages are normalised with the
        whole batch's moments."""
        at, a_out, alg = v.at, v.at.layers[-1], u.alg
        args = (ha, a_out.weight, a_out.bias, u.logstd_flat, v.actions, v.old_mu, u.old_logstd, v.old_logp, v.adv, self._adv_sums, 0.2, alg["bound_coef"],
                alg["entropy_coef"])
        outs = (at.hidden_grad, a_out.weight.grad, a_out.bias.grad, at.layers[-2].bias.grad, self._grad_logstd, self._stats, self._head_scratch_a)
        if v.plan.smoothness:  # the same head on the identity action map: d = mu(x') - mu(x)
            actor_head_sym_loss_backward(*args, self._smooth_coef, self._act_identity, *outs, finish=finish)
        elif v.plan.symmetry:
            actor_head_sym_loss_backward(*args, self._symmetric_coef, self._act_mirror, *outs, finish=finish)
        else:
            actor_head_loss_backward(*args, *outs, finish=finish)

    def _library_loss(self, u, v, mu, values):
        """Output layers as library GEMMs (plan.fused_head = False): the PPO loss of both networks' outputs and its gradients in one launch (bg_ppo_loss).
        Returns dL/d values [rows, 1] and dL/d mu, what the two backward passes start from."""
        alg, g_mu, g_val = u.alg, self._grad_mu[: v.rows], self._grad_val[: v.rows]
        ppo_loss_fused(mu, u.logstd_flat, v.actions, v.old_mu, u.old_logstd, v.old_logp, v.adv, self._adv_sums, values, v.ret, 0.2, alg["bound_coef"],
                       alg["entropy_coef"], g_mu, g_val, self._grad_logstd, self._stats)
        return g_val.view(v.rows, 1), g_mu

    def _step(self, u, v, fwd=None):
        """One optimiser step up to its backward-data passes on the rows of v, as one sequence of launches on the current stream (runner.py:147-163):
        both forward passes and the critic's values on those rows, both output layers fused with the loss, both backward-data passes -- with
        plan.one_stream each pair of passes as ONE launch.  fwd = (hc, ha, values): the last hidden activations and the critic's values where earlier
        launches have left them (K = 1: the step's rows are the values pass's).  Leaves fins / fin_c / fin_a in u for _epoch_gradients_and_step."""
        plan, ct, at = v.plan, v.ct, v.at
        fins = fin_c = fin_a = None
        if plan.fused_head:
            if fwd is None:
                hc, ha = self._forward_hidden(v)
                values = self._head_values(v, hc)
            else:
                hc, ha, values = fwd
            fins, fin_c, fin_a = self._deferred_finishes(plan)
            self._critic_loss_head(v, hc, values, fin_c)
            self._actor_loss_head(u, v, ha, fin_a)
            if plan.ranks and not plan.defer:
                self._exchange_sums()  # exchange (3)
            if plan.one_stream:
                MLPTrainer.backward_hidden_group([ct, at], fins)
            elif plan.gru_group == 2 and v.mem is not None and v.cmem is not None:  # both trunks, then both cells' recurrences as ONE launch
                ct.backward_hidden(finishes=fins)
                at.backward_hidden(finishes=fins)
                GRUTrainer.backward_group([v.cmem.trainer, v.mem.trainer], fins)
            else:
                self._critic_backward_hidden(ct, fins, v.cmem)
                self._actor_backward_hidden(at, fins, v.mem)
        else:
            g_val, g_mu = self._library_loss(u, v, at.forward(v.x_a), ct.forward(v.x_c, train_rows=v.train_rows).squeeze(-1)[: v.rows])
            self._exchange_sums()  # exchange (3)
            ct.backward(g_val)
            at.backward(g_mu)
        u.fins, u.fin_c, u.fin_a = fins, fin_c, fin_a

    def _epoch_on_two_streams(self, u, have_fwd):
        """One step on the whole batch with the critic on the side stream (plan.one_stream = False at K = 1).  Side stream: the whole-batch values pass,
        the critic's loss head and backward-data pass.  Main stream: the actor's forward pass, its loss head once the advantages are there, its
        backward-data pass.  The pieces are _step's; the hand-overs between the streams are this function's.  Leaves fins / fin_c / fin_a in u."""
        v, plan, main, side = u.whole, u.plan, u.main, u.side
        ct, at = v.ct, v.at
        side.wait_stream(main)  # parameters updated by the previous optimiser step
        with torch.cuda.stream(side):
            hc, v_all = self._whole_batch_values(u, ct.acts[2] if have_fwd else None)  # (exchange (1) on the side stream: hidden under the actor forward)
            gae_done = side.record_event()
        values = v_all[: u.B]
        fins = fin_c = fin_a = None
        if plan.fused_head:
            fins, fin_c, fin_a = self._deferred_finishes(plan)
            if have_fwd:
                ha = at.acts[2]
            elif u.ha0 is not None:  # a recurrent actor's mini-epoch 0: old mu's forward pass, run through these same launches on these parameters
                ha, u.ha0 = u.ha0, None
            else:
                ha = self._actor_hidden(at, v.x_a, v.mem)
            with torch.cuda.stream(side):
                self._critic_loss_head(v, hc, values, fin_c)
                self._critic_backward_hidden(ct, fins, v.cmem)
            main.wait_event(gae_done)  # advantages and their moments
            self._actor_loss_head(u, v, ha, fin_a)
            if plan.ranks and not plan.defer:
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    self._exchange_sums()  # exchange (3): loss / KL sums, hidden under the backward passes
            self._actor_backward_hidden(at, fins, v.mem)
        else:
            mu = at.forward(v.x_a)
            main.wait_stream(side)
            g_val, g_mu = self._library_loss(u, v, mu, values)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                self._exchange_sums()  # exchange (3): loss / KL sums, hidden under the backward passes
                ct.backward(g_val)
            at.backward(g_mu)
        u.fins, u.fin_c, u.fin_a = fins, fin_c, fin_a

    def _epoch_gradients_and_step(self, u, v):
        """Deferred reductions, all weight gradients, the exchange of the gradient over the ranks, clip + Adam + KL rule (runner.py:162-180) of the step
        on the rows of v."""
        cfg, B, alg, main, side, plan = u.cfg, v.rows, u.alg, u.main, u.side, v.plan
        fins, fin_c, fin_a, mirrors = u.fins, u.fin_c, u.fin_a, u.mirrors
        # (the first optimiser step after a checkpoint restore runs the separate launches: see __init__)
        fused_tail, one_tail = plan.fused_opt and not self._lr_restart, plan.one_tail and not self._lr_restart
        if not plan.one_stream:
            main.wait_stream(side)
        if plan.defer and not one_tail:  # the deferred reductions as one launch in FRONT of the weight gradients (one_tail: inside bg_update_tail)
            reduce_group([fin_c, fin_a] + fins)
            if plan.ranks:
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    self._exchange_sums()  # exchange (3), beside the weight gradients
        # all weight gradients after both backward chains, alone on the GPU: one launch pair for the six hidden layers (shapes outside the
        # kernel's range, or MLPTrainer.FUSED_WGRAD = False: library GEMMs, layer by layer); one_tail: their finish inside bg_update_tail
        # (a recurrent actor: the cell's two weight gradients ride in the same launch, its padded W_ih among the copies)
        trainers = (v.ct, v.at) if v.mem is None else (v.ct, v.at, v.mem.trainer)
        if v.cmem is not None:
            trainers += (v.cmem.trainer,)
        wg_partial = v.wgrad.run(trainers, plan.wgrad, one_tail)
        if plan.defer and plan.ranks:
            main.wait_stream(side)
        if one_tail and plan.ranks:
            # ranks: the sums, then ONE collective launch on this stream (gradient bucket: mean; loss / KL sums: sum; log-std gradient: mean -- exchanges
            # (2) and (3) of SURVEY 8(e)), then the optimiser launch, which takes the norm of the averaged gradient
            self.optimizer.tail_sums(wg_partial, [fin_c, fin_a] + fins)
            self.dp.exchange_tail_(self.optimizer.grad, self._stats, self._grad_logstd)
        elif not one_tail:
            self.dp.average_(self.optimizer.grad)  # exchange (2): the one collective on the critical path
        # clip + Adam + KL rule + statistics bookkeeping (and the zeroing of the accumulators for the next mini-epoch): one of FlatAdam's three forms
        opt = dict(stats=self._stats, stats_acc=self._stats_acc, stats_last=self._stats_last, kl_index=4, count=B * self.world_size,
                   desired_kl=alg["desired_kl"], grad_logstd=self._grad_logstd, ls_off=self._logstd_off)
        if fused_tail:
            # ... in ONE launch, with the copies of the weights that the layer kernels read (zero-padded first layers, transposed hidden layers):
            # written by the same launch instead of six strided torch copies inside the chains of the next mini-epoch
            if mirrors is None:
                plans = (v.ct.plan, v.at.plan, v.at.plan, v.ct.plan)  # (a cell's copies follow its trunk's plan)
                ms = [d for tr, pl in zip(trainers, plans) for d in tr.copies.descriptors(self.optimizer.flat, pl)]
                mirrors = (_lib.ParamMirror * len(ms))(*ms) if 0 < len(ms) <= 16 else None
            if one_tail and not plan.ranks:
                self.optimizer.step_tail(wg_partial, [fin_c, fin_a] + fins, mirrors=mirrors, **opt)
            else:
                self.optimizer.step_fused(mirrors=mirrors, **opt)
        else:
            # ... as separate launches (the log-std gradient's copy: behind the bucket's all-reduce, which carries a stale value in this slot);
            # the first step after a checkpoint load: see __init__
            self.optimizer.step_separate(lr_restart=cfg["algorithm"]["learning_rate"] if self._lr_restart else None, **opt)
            self._lr_restart = False
        self._clock.tick()  # the parameters have changed: every weight copy of every trainer over them is stale, but those this launch listed and wrote
        if fused_tail and mirrors is not None:
            for tr in trainers:
                tr.copies.stamp()
        u.mirrors = mirrors

    def _plan_chain_split(self, x_c, x_a, plan, ct=None, at=None):
        """ct / at: the pair of trainers whose launches are planned (default: the whole-batch pair; runner.num_mini_batches > 1: the mini-batch pair, with
        x_c / x_a one mini-batch's b rows, so that the shares are sized for b-row slabs).  x_c / x_a: the critic's / the actor's input of the full-batch forward pass (their widths, not the trainers': a trainer is allocated by its
        first pass, which may come after this).  The two networks' chains of a mini-epoch run side by side -- inside one grid (the default) or as two launches on two streams -- one workgroup
        per CU (all of its LDS).  Left to the dispatcher, equal-sized slabs of unequal cost run in lockstep rounds and the last 32 slabs run alone (370 us
        for 325 us of work per CU); here each network gets a share of the CUs whose workgroups walk its slabs (bg_mlp_chain_split::workgroups): the
        split that minimises the longer of the two, slab cost ~ flops.  Which workgroup walks which slab changes no bit of the results."""
        ct, at = ct or self._critic_tr, at or self._actor_tr
        ct.chain_workgroups = at.chain_workgroups = 0
        if not (self._split_chain_cus and plan.critic.chained and plan.actor.chained):
            return
        cus = torch.cuda.get_device_properties(self.device).multi_processor_count
        sc, sa = (x_c.shape[0] + 127) // 128, (x_a.shape[0] + 127) // 128
        if sc + sa <= cus:
            return
        cost = lambda tr, x: sum(l.weight.shape[0] * (x.shape[1] if i == 0 else l.weight.shape[1]) for i, l in enumerate(tr.layers[:3]))
        ct.chain_workgroups, at.chain_workgroups = plan_chain_split(sc, sa, cost(ct, x_c), cost(at, x_a), cus)
        fixed = os.environ.get("BG_FWD_CHAIN_CUS")  # "critic,actor": a fixed split (A/B runs)
        if fixed:
            ct.chain_workgroups, at.chain_workgroups = (int(v) for v in fixed.split(","))
        # the chained backward launches likewise (slab cost ~ flops of the two backward layers)
        ct.chain_bwd_workgroups = at.chain_bwd_workgroups = 0
        if self._split_bwd_chain_cus and plan.critic.bwd == plan.actor.bwd == "chain_split":
            bcost = lambda tr: sum(l.weight.shape[0] * l.weight.shape[1] for l in tr.layers[1:3])
            # the critic's backward differentiates the batch, the actor's the batch (and, with the symmetry loss, its mirror images: x_a's 2B rows)
            sb = (x_a.shape[0] // (2 if plan.symmetry else 1) + 127) // 128
            ct.chain_bwd_workgroups, at.chain_bwd_workgroups = plan_chain_split(sb, sa, bcost(ct), bcost(at), cus)
            fixed = os.environ.get("BG_BWD_CHAIN_CUS")  # "critic,actor": a fixed split (A/B runs)
            if fixed:
                ct.chain_bwd_workgroups, at.chain_bwd_workgroups = (int(v) for v in fixed.split(","))

    def _exchange_sums(self):
        """Exchange (3), on the current (side) stream: the loss / KL sums and the log-std gradient of all ranks in one float64 all-reduce; the gradient
        is then the mean over ranks like the bucket's."""
        self.dp.sum_(self._sums, tag="stats")
        if self.world_size > 1:
            self._grad_logstd.mul_(1.0 / self.world_size)

    def iteration(self):
        self.rollout()
        stats = self.update()
        self.buffer.roll()  # carry the last observation into row 0 of the next rollout
        return stats

    def _sync_curriculum(self):
        """Multi-rank command curriculum: sum every rank's increments of the probability grid since the last sync."""
        if not (self.dp.active and self.cfg["commands"].get("curriculum", False)):
            return
        new = self.dp.sync_grid(self.env.curriculum_prob, self._curr_last)
        self.env.curriculum_prob = new
        self._curr_last = new

    def _summarize(self, stats_acc):
        """Host-side means of the loss terms over the mini-epochs (runner.py:182-204); one device->host read (blocking: tests and tools)."""
        extra = () if self._est is None else (self._est_trainer.loss,)  # (read with the same one copy)
        if self._rnd_trainer is not None:
            extra = (self._rnd_trainer.log,) + extra
        s = torch.cat((stats_acc, self._stats_last, self.optimizer.lr.double()) + extra).cpu().tolist()
        out = self._summary_from(s)
        if self._est is not None:
            out["estimator/loss"] = s[-1]
        if self._rnd_trainer is not None:
            h = 2 * self._n_stats + 1
            out.update(zip(RND_LOG, s[h : h + 4]))
        return out

    def _summary_from(self, s):
        T, N = self.cfg["runner"]["horizon_length"], self.env.num_envs
        B, A, E, S = T * N * self.world_size, self.env.num_actions, self.cfg["runner"]["mini_epochs"], self._n_stats
        self.learning_rate = s[2 * S]
        out = {"value_loss": s[0] / (B * E), "actor_loss": s[1] / (B * E), "bound_loss": s[2] / (B * A * E), "entropy": s[3] / (B * E),
               "kl_mean": s[S + 4] / (B // max(self._mini_batches, self._env_mini_batches)), "lr": s[2 * S]}  # (the last optimiser step's KL sum: over its b = B / K rows of every rank)
        if S > 5 and self._smooth:  # mean squared difference of the actor's mean over the pairs (x, x'), before smoothness_coef
            out["smoothness_loss"] = s[5] / (B * A * E)
        elif S > 5:  # mean squared asymmetry of the actor's mean, before symmetric_coef (like bound_loss before bound_coef)
            out["symmetry_loss"] = s[5] / (B * A * E)
        return out

    # ------------------------------------------------------------------ entry points
    # The reference's loop reads several scalars per mini-epoch with .item() (runner.py:175,182-184) and so stalls the GPU twenty times per
    # iteration.  Here an iteration's scalars (loss sums, learning rate, episode statistics, curriculum levels: 45 numbers) are gathered into ONE
    # device vector and copied to pinned host memory without blocking; they are written to the log while the NEXT iteration runs, with their own
    # iteration number.  The host never waits for the GPU inside the loop, so train() runs at the speed of bench.py's timed region (which calls
    # the same train_iteration); the last iteration's scalars are flushed after the loop.
    def begin_training(self, recorder=None):
        self.recorder = recorder if recorder is not None else Recorder(self.cfg, rank=self.rank)
        obs, infos = self.env.reset()
        self.buffer["obses"][0].copy_(obs)
        self.buffer["privileged_obses"][0].copy_(infos["privileged_obs"])
        if self._mem_tr is not None:  # a recurrent actor starts (and, from a checkpoint, resumes: the state is not saved) on a reset env with a zero state
            self.model.memory_state(self.env.num_envs, obs.device).zero_()
            self._last_dones.zero_()
        if self._cmem_tr is not None:  # ... and a recurrent critic likewise
            self._cmem_tr.next_state.zero_()
        # (+1 with the terrain curriculum: the sum of this rank's terrain levels)
        # (+1 with the estimator, last: its loss rides in the iteration's one host read)
        # (+3 with algorithm.normalize_value, in front of the estimator's: the normaliser's mean, variance and count)
        self._log_vn = 2 * self._n_stats + 1 + 4 + _lib.NUM_REWARD_TERMS + 4 + (1 if self.env.terrain.curriculum else 0)
        # (+4 with rnd.enabled, behind the value normaliser's and in front of the estimator's: RND_LOG)
        self._log_rnd = self._log_vn + (3 if self.value_norm is not None else 0)
        n = self._log_rnd + (4 if self._rnd_trainer is not None else 0) + (1 if self._est is not None else 0)
        self._log_dev = torch.zeros(n, dtype=torch.float64, device=self.device)
        self._log_host = [torch.zeros(n, dtype=torch.float64).pin_memory() for _ in range(2)]
        self._log_event = [torch.cuda.Event() for _ in range(2)]
        self._log_pending = None
        self._log_obs_norm = [None, None]
        self.nonfinite_resets_total = 0.0  # over the whole run (the per-iteration accumulator is reset when it is read)

    def _flush_log(self):
        if self._log_pending is None:
            return
        slot, it = self._log_pending
        self._log_event[slot].synchronize()  # recorded one iteration ago: already complete unless the host ran a whole iteration ahead
        s = self._log_host[slot].tolist()
        self._log_pending = None
        h = 2 * self._n_stats + 1  # loss sums, the last mini-epoch's sums, learning rate
        summary = self._summary_from(s[:h])
        ne = 4 + _lib.NUM_REWARD_TERMS
        self.recorder.record_episode_statistics(self.env, self.env.reward_names, it, stats=s[h : h + ne])
        self.nonfinite_resets_total += s[h + ne - 1]
        lv = s[h + ne : h + ne + 4]
        if self.cfg["commands"].get("curriculum", False):
            self.env.mean_lin_vel_level, self.env.mean_ang_vel_level, self.env.max_lin_vel_level, self.env.max_ang_vel_level = lv
        summary.update({"curriculum/mean_lin_vel_level": self.env.mean_lin_vel_level, "curriculum/mean_ang_vel_level": self.env.mean_ang_vel_level,
                        "curriculum/max_lin_vel_level": self.env.max_lin_vel_level, "curriculum/max_ang_vel_level": self.env.max_ang_vel_level})
        if self.env.terrain.curriculum:  # this rank's envs only under data parallelism
            summary["terrain/mean_level"] = s[h + ne + 4] / self.env.num_envs
        if self.obs_norm is not None:
            summary.update(self._log_obs_norm[slot])
        if self.value_norm is not None:
            summary.update(ValueNormalizer.scalars_from(s[self._log_vn : self._log_vn + 3]))
        if self._rnd_trainer is not None:
            summary.update(zip(RND_LOG, s[self._log_rnd : self._log_rnd + 4]))
        if self._est is not None:  # the last epoch's SSE / (12 B) of the iteration's estimator update
            summary["estimator/loss"] = s[-1]
        self.recorder.record_statistics(summary, it)

    def train_iteration(self, it):
        """One pass of the reference's training loop body (runner.py:103-213): rollout, update, statistics, curriculum exchange, checkpoint."""
        stats = self.iteration()
        d, S = self._log_dev, self._n_stats
        h = 2 * S + 1
        d[0:S].copy_(stats); d[S : 2 * S].copy_(self._stats_last); d[2 * S : h].copy_(self.optimizer.lr)
        ne = 4 + _lib.NUM_REWARD_TERMS
        d[h : h + ne].copy_(self.env.episode_stats(reset=True))
        self._sync_curriculum()
        if self.cfg["commands"].get("curriculum", False):
            lin = self.env.get_field("env_curriculum_level_lin").abs().double()
            ang = self.env.get_field("env_curriculum_level_ang").abs().double()
            d[h + ne : h + ne + 4].copy_(torch.stack((lin.mean(), ang.mean(), lin.max(), ang.max())))
        if self.env.terrain.curriculum:
            d[h + ne + 4 : h + ne + 5].copy_(self.env.terrain_level_sum())
        if self.value_norm is not None:
            d[self._log_vn : self._log_vn + 3].copy_(self.value_norm.state)
        if self._rnd_trainer is not None:
            d[self._log_rnd : self._log_rnd + 4].copy_(self._rnd_trainer.log)
        if self._est is not None:
            d[-1:].copy_(self._est_trainer.loss)
        self._flush_log()  # the previous iteration's scalars: their copy finished long ago
        slot = it & 1
        self._log_host[slot].copy_(d, non_blocking=True)
        self._log_event[slot].record()
        self._log_pending = (slot, it)
        if self.obs_norm is not None:  # (host values already: written with this iteration's scalars, one iteration later)
            self._log_obs_norm[slot] = self.obs_norm.scalars()
        if (it + 1) % self.cfg["runner"]["save_interval"] == 0:
            self.recorder.save(self.checkpoint_dict(), it + 1)

    def train(self):
        self.begin_training()
        max_it = self.cfg["basic"]["max_iterations"]
        for it in range(max_it):
            self.train_iteration(it)
            if self.rank == 0:
                print("epoch: {}/{}".format(it + 1, max_it))
        self._flush_log()

    def play(self, max_steps=None, record_path=None):
        """Deterministic rollout with `dist.loc` (runner.py:217-229).  The reference's camera video (runner.py:230-241) is replaced
        by an optional .npz trajectory dump; `max_steps=None` runs until interrupted like the reference."""
        obs, infos = self.env.reset()
        traj, step = [], 0
        if self._memory:  # a recurrent student: the rollout's own launch carries its state; the done flags of a step restart the rows' memory in the next
            mean, sampled = (torch.zeros(self.env.num_envs, self.env.num_actions, device=self.device) for _ in range(2))
            self.model.reset_memory()
            done = None
        if self._est is not None:  # the rollout's own launch: its mean is the action; its sample and the estimates go to scratch tensors
            mean, sampled = (torch.zeros(self.env.num_envs, self.env.num_actions, device=self.device) for _ in range(2))
            est_scratch = torch.zeros(self.env.num_envs, EST_WIDTH, device=self.device)
        try:
            while max_steps is None or step < max_steps:
                with torch.no_grad():
                    if self.obs_norm is not None:
                        obs = self.obs_norm.normalize_into(obs, torch.empty_like(obs))
                    if self._est is not None:
                        self.model.sample_actions(obs.contiguous(), sampled, 0, step, mu_out=mean, est_out=est_scratch)
                        act = mean
                    elif self._memory:
                        self.model.sample_actions(obs.contiguous(), sampled, 0, step, mu_out=mean, reset=done)
                        act = mean
                    else:
                        act = self.model.actor(obs)
                    obs, rew, done, infos = self.env.step(act)
                if record_path is not None:
                    traj.append({"root": self.env.root_states[0].cpu().numpy(), "dof_pos": self.env.dof_pos[0].cpu().numpy(), "rew": float(rew[0])})
                step += 1
        except KeyboardInterrupt:
            pass
        if record_path is not None and traj:
            np.savez(record_path, root=np.stack([t["root"] for t in traj]), dof_pos=np.stack([t["dof_pos"] for t in traj]),
                     rew=np.array([t["rew"] for t in traj]))
        return step
