"""Actor-critic network.

Same architecture and `state_dict` key names as reference `utils/model.py:5-36` (so checkpoints and the exported
TorchScript actor interoperate): `critic.{0,2,4,6}`, `actor.{0,2,4,6}`, `logstd`; actor 47-256-128-128-12,
critic (47+14)-256-256-128-1, ELU, state-independent log-std initialised to -2.  The hidden widths are configurable
(`algorithm.actor_hidden` / `algorithm.critic_hidden`, checked by `check_hidden`): 2 to 4 hidden layers of 128, 256 or 512, the last 128 wide;
the keys keep the `Sequential` numbering (`actor.{0,2,4,6,8}` for four hidden layers).
The PPO update's GEMMs run on hand-written HIP kernels (MLPTrainer: the chained hidden layers, the grouped weight
gradients), in the form its NetPlan names, on copies of the weights that one object per trainer owns (WeightCopies: padded, transposed, bf16 planes;
each current exactly when written or stamped at the present value of the parameters' WeightClock); the rollout-time inference + sampling is one fused HIP launch
(`sample_actions` -> bg_actor_sample at the reference's widths on 47 inputs, bg_actor_sample_mlp at any other supported widths and on a
frame stack of 47 H inputs).  With estimator.enabled a third network, `estimator` (47 H -> hidden -> 12), feeds the first E of its outputs to the
actor behind the observations; the rollout runs both in one launch (bg_actor_sample_est).  An actor may be recurrent (`memory_hidden`: a distilled
student of distillation.student_memory, or PPO's own under algorithm.rnn_hidden_size): a GRU cell `memory` in front of the actor, one launch per
step as well (bg_actor_sample_gru), and GRUTrainer around the trunk's MLPTrainer in the update.
"""
import ctypes
import math
import os
from contextlib import contextmanager
from functools import partial
from types import SimpleNamespace
from typing import Callable, NamedTuple, Optional

import torch

from .. import _lib

ACTOR_HIDDEN = (256, 128, 128)
CRITIC_HIDDEN = (256, 256, 128)
# The architectures every kernel of the rollout and the update takes: 2 to 4 hidden layers, each of these widths, the last one HEAD_WIDTH wide (the
# fused output layers of bg_head.hip).  The reference's widths run the chained kernels; every other supported architecture the per-layer ones.
HIDDEN_WIDTHS = (128, 256, 512)
HIDDEN_LAYERS = (2, 4)
HEAD_WIDTH = 128
SPLIT_K = (64, 128, 256)  # layer inputs of the split-bf16 per-layer kernels (bg_mlp_split.hip)


def check_hidden(actor_hidden=ACTOR_HIDDEN, critic_hidden=CRITIC_HIDDEN, split=0):
    """The two width lists as tuples, or ValueError naming the supported set.  split: the products of the split-bf16 GEMMs in use
    (parallel.gemm_split / BG_GEMM_SPLIT; 0 = off), whose per-layer kernels take layer inputs of SPLIT_K columns only."""
    supported = (f"supported: {HIDDEN_LAYERS[0]} to {HIDDEN_LAYERS[1]} hidden layers, each of width {', '.join(map(str, HIDDEN_WIDTHS))}, "
                 f"the last one {HEAD_WIDTH} (the fused output layers)")
    out = []
    for name, h in (("algorithm.actor_hidden", actor_hidden), ("algorithm.critic_hidden", critic_hidden)):
        ok = (isinstance(h, (list, tuple)) and HIDDEN_LAYERS[0] <= len(h) <= HIDDEN_LAYERS[1]
              and all(isinstance(w, int) and not isinstance(w, bool) and w in HIDDEN_WIDTHS for w in h) and h[-1] == HEAD_WIDTH)
        if not ok:
            raise ValueError(f"{name} = {h!r} is not a supported architecture; {supported}")
        out.append(tuple(h))
    if split:
        for name, h in zip(("algorithm.actor_hidden", "algorithm.critic_hidden"), out):
            if any(w not in SPLIT_K for w in h[:-1]):
                raise ValueError(f"parallel.gemm_split / BG_GEMM_SPLIT = {split} runs split-bf16 layer kernels that take layer inputs of "
                                 f"{', '.join(map(str, SPLIT_K))} columns only; {name} = {list(h)} has a wider layer (use gemm_split 0)")
    return out[0], out[1]


def hidden_of(state_dict, net):
    """Hidden widths of network `net` ("actor" / "critic") of an ActorCritic state_dict: the output widths of its Linear layers but the last."""
    idx = sorted(int(k.split(".")[1]) for k in state_dict if k.startswith(net + ".") and k.endswith(".weight"))
    return tuple(int(state_dict[f"{net}.{i}.weight"].shape[0]) for i in idx[:-1])


def _mlp(n_in, hidden, n_out):
    layers, prev = [], n_in
    for h in hidden:
        layers += [torch.nn.Linear(prev, h), torch.nn.ELU()]
        prev = h
    layers.append(torch.nn.Linear(prev, n_out))
    return torch.nn.Sequential(*layers)


def plan_wgrad_slices(shapes, rows, workgroups=256, share_rows=True):
    """(slices, tiles per workgroup) per layer for bg_mlp_weight_grad_group: `shapes` = [(C_out, C_in padded)].  One workgroup per (group of tw
    output tiles, slice); its 4 waves cover tw tiles x ks = 4 / tw sub-ranges of the slice's rows.  Every WAVE of the launch should do the same MFMA
    work: a wave's cost is rows / (slices ks) x tile width, so slices is proportional to width / ks; the total stays within `workgroups` (one
    512-register workgroup per CU).  share_rows: layers with 2 or 4 tiles put them in one workgroup (tw = tile count), so that the waves working on
    the same rows fetch them once per CU (less input traffic, more partial-tile traffic).  Largest-remainder rounding."""
    tiles = [(co // 128) * max(1, ci // 128) for co, ci in shapes]
    width = [0.5 if ci == 64 else 1.0 for _, ci in shapes]
    tw = [(t if t in (2, 4) else 1) if share_rows else 1 for t in tiles]
    ks = [4 // t for t in tw]
    units = sum(t * c for t, c in zip(tiles, width))  # total work in (128 x 128 tile) x rows
    scale = 4.0 * workgroups / units
    ideal = [scale * c / k for c, k in zip(width, ks)]
    groups = [t // w for t, w in zip(tiles, tw)]
    # every wave should get at least one run of 16 row pairs (fp32 kernel) / two 16-row blocks (split kernel: a hard limit there): slices x ks <=
    # rows / 32.  Below 32 x ks rows one slice remains and some of its waves get an empty run, which the fp32 kernel handles (they add zeros).
    cap = [max(1, rows // (32 * k)) for k in ks]
    s = [max(1, min(cp, int(x))) for x, cp in zip(ideal, cap)]
    order = sorted(range(len(shapes)), key=lambda k: ideal[k] - int(ideal[k]), reverse=True)
    for k in order:
        if s[k] < cap[k] and sum(g * v for g, v in zip(groups, s)) + groups[k] <= workgroups:
            s[k] += 1
    return s, tw


class NetPlan(NamedTuple):
    """The kernels one network's passes run in an update (plan_network); every branch of MLPTrainer reads it (MLPTrainer.plan)."""
    fwd: str         # hidden layers: "chain_split" / "chain" (one launch: bf16 splits / fp32 MFMA), "layer_split" / "layer" (one launch per layer), "library"
    bwd: str         # backward-data of the hidden layers: "chain_split" (one launch), "layer_split" / "layer" (one launch per layer), "library"
    alternate: bool  # odd slabs of the chained split kernels accumulate the negated sums (MLPTrainer.CHAIN_ALTERNATE)
    terms: int       # products of the per-layer split kernels ("layer_split": MLPTrainer.SPLIT)
    grouped: tuple   # per layer: its weight gradient runs in the grouped launch (GroupedWeightGrad); False: library GEMMs

    @property
    def chained(self):
        return self.fwd in ("chain", "chain_split")


def plan_network(widths, kin, rows, split, fused, chain, chain_split, chain_split_bwd, alternate, fused_wgrad):
    """NetPlan of an MLP of layer widths `widths` (input, hidden..., output) whose input is zero-padded to `kin` columns and whose backward pass
    differentiates `rows` rows, under MLPTrainer's switches (SPLIT, FUSED, CHAIN, CHAIN_SPLIT, CHAIN_SPLIT_BWD, CHAIN_ALTERNATE, FUSED_WGRAD).  Pure: no
    tensors, no device.  The chained kernels take the reference's widths on a zero-padded 64-column input."""
    chainable = chain and fused and not split and kin == 64 != widths[0] and tuple(widths[1:-1]) in ((256, 128, 128), (256, 256, 128))
    per_layer = ("layer_split" if split else "layer") if fused else "library"
    fwd = ("chain_split" if chain_split else "chain") if chainable else per_layer
    bwd = "chain_split" if fwd == "chain_split" and chain_split_bwd else per_layer
    # the grouped kernel's shapes: output widths a multiple of 128, input widths 64 or a multiple of 128, an even batch of 64 rows or more
    grouped = tuple(bool(fused_wgrad and fused) and co % 128 == 0 and (ci == 64 or ci % 128 == 0) and rows % 2 == 0 and rows >= 64
                    for ci, co in zip((kin,) + tuple(widths[1:-1]), widths[1:]))
    return NetPlan(fwd, bwd, bool(alternate), int(split) if fused else 0, grouped)


INPUT_PADS = (64, 128, 256, 512)  # first-layer inputs of the per-layer fused kernels (bg_mlp.hip); the chained kernels take 64 only
WGRAD_SPLIT_SHAPES = ((256, 256), (128, 256), (128, 128), (256, 64))  # (C_out, C_in padded) that bg_wgrad_split.hip has kernels for


def pad_input(width):
    """The zero-padded input width of a network whose input has `width` features: the next of 64, 128, 256, 512 (actor 47 -> 64; critic 61 -> 64,
    61 + 187 = 248 -> 256 with the default height scan); ValueError beyond 512."""
    for p in INPUT_PADS:
        if width <= p:
            return p
    raise ValueError(f"a network input of {width} features exceeds the widest first layer of the kernels ({INPUT_PADS[-1]})")


def wgrad_products(rows, grouped, bwd_chained, split, wgrad_split):
    """Products of the grouped weight-gradient launch over the layers `grouped` = [(C_out, C_in padded)]: 0 = fp32 MFMA (bg_wgrad.hip), 6 / 9 = bf16
    splits (bg_wgrad_split.hip: its shapes, rows a multiple of 32 from 128 up; `split` everywhere, `wgrad_split` behind the chained split backward of
    every network only).  The one rule of runner.plan_update and of utils/supervised.py."""
    if rows % 32 != 0 or rows < 128 or not all(s in WGRAD_SPLIT_SHAPES for s in grouped):
        return 0
    return split or (wgrad_split if bwd_chained else 0)


def layer_descriptors(linears):
    """The bg_mlp_layer_desc array of a list of Linear layers on their current parameter storage, for the launches that take a network by descriptors
    (callers cache it behind a key of the parameters' data_ptr: an optimiser moves the storage into its flat buffer once)."""
    return (_lib.MlpLayerDesc * len(linears))(*[_lib.MlpLayerDesc(l.weight.data_ptr(), l.bias.data_ptr(), l.in_features, l.out_features) for l in linears])


class GroupedWeightGrad:
    """All deferred weight gradients of several MLPTrainers in one launch pair (bg_mlp_weight_grad_group)."""

    MAX_PROBLEMS = 8  # layers per launch (csrc/bg_wgrad.h: WG_MAX_PROBLEMS)

    def __init__(self, workgroups=None):
        self.workgroups = workgroups or MLPTrainer.WGRAD_WORKGROUPS
        # waves of a workgroup on the same rows, different tiles (plan_wgrad_slices): measured no faster alone (329.6 vs 329.2 us for the six layers) and
        # 0.3 ms slower per update in the loop (4x the partial-tile traffic for the 256 x 256 layer), so the pure split over rows stays the default
        self.share_rows = False
        self._key, self._arr, self._scratch = None, None, None
        self._more = None  # a second launch, for the problems beyond MAX_PROBLEMS
        self.timed_events = None

    def run(self, trainers, split, partial):
        """The launch of every pending weight gradient in the form the UpdatePlan names: split = 0 the fp32-MFMA kernel (bg_wgrad.hip), 6 / 9 the
        bf16-split kernel with that many products (bg_wgrad_split.hip: the waves of a workgroup share their rows through LDS, all tiles of a layer in one
        workgroup).  partial: the main kernel only (..._partial); returns (descriptor array, count) for bg_update_tail, which sums the slices inside
        the mini-epoch's last launch.  Otherwise the finished gradients are written and None is returned."""
        probs = [p for tr in trainers for p in tr.pending_wgrad_problems()]
        if not probs:
            return None
        if len(probs) > self.MAX_PROBLEMS:
            # more layers than one launch takes (two networks and two cells: 10): the first MAX_PROBLEMS here, the rest in a launch of its own
            if partial:
                raise ValueError(f"GroupedWeightGrad: {len(probs)} weight gradients do not fit the one launch whose finish bg_update_tail runs")
            if self._more is None:
                self._more = GroupedWeightGrad(self.workgroups)
            self._launch(probs[: self.MAX_PROBLEMS], split, partial)
            return self._more._launch(probs[self.MAX_PROBLEMS :], split, partial)
        return self._launch(probs, split, partial)

    def _launch(self, probs, split, partial):
        key = (split,) + tuple((g.data_ptr(), a.data_ptr(), dw.data_ptr(), g.shape[0], co, ci, cr) for g, a, dw, co, ci, cr in probs)
        if key != self._key:  # buffers are static: built once per form
            rows = probs[0][0].shape[0]
            self.split = split
            slices, tw = plan_wgrad_slices([(co, ci) for _, _, _, co, ci, _ in probs], rows, self.workgroups, share_rows=self.share_rows or bool(split))
            self._scratch = [torch.empty(sl * co * ci, dtype=torch.float32, device=probs[0][0].device) for sl, (_, _, _, co, ci, _) in zip(slices, probs)]
            arr = (_lib.WgradProblem * len(probs))()
            for k, ((g, a, dw, co, ci, cr), sl) in enumerate(zip(probs, slices)):
                arr[k].G, arr[k].A, arr[k].dW, arr[k].scratch = g.data_ptr(), a.data_ptr(), dw.data_ptr(), self._scratch[k].data_ptr()
                arr[k].M, arr[k].C_out, arr[k].C_in, arr[k].C_in_real, arr[k].slices, arr[k].tiles_per_workgroup = g.shape[0], co, ci, cr, sl, tw[k]
            self._key, self._arr, self.slices, self.tw = key, arr, slices, tw
        ev = self.timed_events
        if ev is not None:  # bench.py: HIP events on the launch stream around the launch pair
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        name = "bg_mlp_weight_grad_group" + ("_split" if split else "") + ("_partial" if partial else "")
        _lib.check(getattr(_lib.load(), name)(self._arr, len(probs), *((split,) if split else ()), _lib.current_stream_ptr()), name)
        if ev is not None:
            e1.record()
            # algorithmic flops: the REAL input columns (47 / 61 of the zero-padded 64 of the first layers)
            ev.append((e0, e1, sum(2.0 * g.shape[0] * co * cr for g, _, _, co, _, cr in probs), [(g.shape[0], co, cr) for g, _, _, co, _, cr in probs]))
        return (self._arr, len(probs)) if partial else None


class WeightClock:
    """The version of one set of parameters: one integer, shared by every trainer over those parameters (a Runner's whole-batch and mini-batch pairs, a
    Distiller's trainer) and ticked by whoever changes them -- every optimiser step, Runner.invalidate(), an update() that does not start from the
    rollout's forward passes.  A weight copy is current exactly when it was written or stamped at the clock's present value (WeightCopies)."""
    now = 0

    def tick(self):
        self.now += 1


def _write_planes(name, transpose, w, kp, out):
    """The bf16 planes of w [rows, cols] (its columns zero-padded to kp) or of its transpose into `out`, through the library's writer `name`."""
    rows, cols = w.shape
    n, k = (cols, rows) if transpose else (rows, kp)
    _lib.check(getattr(_lib.load(), name)(n, k, _lib.ptr(w), cols, rows, cols, transpose, _lib.ptr(out), _lib.current_stream_ptr()), name)


class CopyKind(NamedTuple):
    """One kind of copy of a weight matrix W [rows, cols] whose input is zero-padded to kp columns (kp = cols for every layer but the first)."""
    shape: Callable    # (rows, cols, kp) -> shape of the copy
    dtype: torch.dtype
    write: Callable    # (w, kp, out): rewrite `out` from the parameter, on the current stream
    mirror: Optional[Callable]  # (rows, cols, kp) -> (transpose, ld, pad) of its bg_param_mirror entry; None: the optimiser launch cannot write it
    read_by: tuple     # (NetPlan field, values): the plans whose kernels read it from an optimiser launch's entry


# Every copy of a weight matrix that a layer kernel reads, in the order the bg_param_mirror entries of one layer are listed; the layouts appear here only.
#   cplanes / cplanes_t  the chained split kernels': the three bf16 planes of W (of W^T), then those of -W (bg_param_mirror.pad: where the second set starts)
#   w0pad / wt           the fp32 kernels': the zero-padded first layer (the padded columns stay zero) / the transposed hidden layers of the backward
#   planes / planes_t    the per-layer split kernels': the planes of W / of W^T (bg_mlp_split.hip)
COPY_KINDS = {
    "cplanes": CopyKind(lambda r, c, kp: (2 * r * kp * 3,), torch.int16, partial(_write_planes, "bg_mlp_split_weights_pm", 0),
                        lambda r, c, kp: (2, kp, r * kp * 3), ("fwd", ("chain_split",))),
    "w0pad": CopyKind(lambda r, c, kp: (r, kp), torch.float32, lambda w, kp, out: out[:, : w.shape[1]].copy_(w),
                      lambda r, c, kp: (0, kp, 0), ("fwd", ("chain", "layer"))),
    "cplanes_t": CopyKind(lambda r, c, kp: (2 * c * r * 3,), torch.int16, partial(_write_planes, "bg_mlp_split_weights_pm", 1),
                          lambda r, c, kp: (3, r, r * c * 3), ("bwd", ("chain_split",))),
    "wt": CopyKind(lambda r, c, kp: (c, r), torch.float32, lambda w, kp, out: out.copy_(w.t()), lambda r, c, kp: (1, r, 0), ("bwd", ("layer",))),
    "planes": CopyKind(lambda r, c, kp: (r * kp * 3,), torch.int16, partial(_write_planes, "bg_mlp_split_weights", 0), None, ()),
    "planes_t": CopyKind(lambda r, c, kp: (c * r * 3,), torch.int16, partial(_write_planes, "bg_mlp_split_weights", 1), None, ()),
}


class WeightCopies:
    """Every copy of one trainer's weights that its layer kernels read (COPY_KINDS), each with the clock value at which it was last written from the
    parameter or stamped as written by the optimiser launch.  `tensors`: {(kind, layer): tensor} of the copies that exist.  Without a clock nothing is
    ever current: every `get` rewrites (a stand-alone trainer)."""

    def __init__(self, layers, clock=None, kin=None):
        self.layers, self.clock = layers, clock
        self.reset(kin)

    def reset(self, kin):
        """Forget every copy; kin: the zero-padded input width of the first layer."""
        self.kin, self.tensors, self._at, self.listed = kin, {}, {}, []

    def kp(self, i):
        return self.kin if i == 0 else self.layers[i].weight.shape[1]

    def current(self, kind, i):
        return self.clock is not None and self._at.get((kind, i)) == self.clock.now

    def _write(self, kind, i):
        COPY_KINDS[kind].write(self.layers[i].weight, self.kp(i), self.tensors[kind, i])
        self._at[kind, i] = self.clock and self.clock.now

    def get(self, kind, i):
        """The copy `kind` of layer i's weight: created (zeroed) on first use, rewritten from the parameter if and only if it is not current."""
        if (kind, i) not in self.tensors:
            w, k = self.layers[i].weight, COPY_KINDS[kind]
            self.tensors[kind, i] = torch.zeros(k.shape(*w.shape, self.kp(i)), dtype=k.dtype, device=w.device)
        if not self.current(kind, i):
            self._write(kind, i)
        return self.tensors[kind, i]

    def rewrite_all(self):
        """Rewrite every copy that exists from the parameters, current or not, on the current stream."""
        for kind, i in self.tensors:
            self._write(kind, i)

    def descriptors(self, flat, plan):
        """bg_param_mirror entries of the existing copies that the kernels of `plan` read, for the optimiser launch (bg_optimizer_step / bg_update_tail),
        which then writes them together with the parameters; `stamp()` afterwards.  flat: the optimiser's flat parameter buffer (the weights are views
        of it).  Remembers what it listed (`listed`); nothing for the "layer_split" and "library" plans, whose kernels read no copy the launch can write."""
        out, self.listed = [], []
        for i, l in enumerate(self.layers):
            off, (rows, cols) = (l.weight.data_ptr() - flat.data_ptr()) // 4, l.weight.shape
            for kind, k in COPY_KINDS.items():
                if (kind, i) in self.tensors and k.mirror is not None and getattr(plan, k.read_by[0]) in k.read_by[1]:
                    out.append(_lib.ParamMirror(off, rows, cols, *k.mirror(rows, cols, self.kp(i)), _lib.ptr(self.tensors[kind, i])))
                    self.listed.append((kind, i))
        return out

    def stamp(self):
        """The optimiser launch has just written the copies `descriptors` listed: they are the parameters of the clock's present value."""
        self._at.update((key, self.clock and self.clock.now) for key in self.listed)


@contextmanager
def timed(trainers, note, layer=None):
    """bench.py's probe: where a trainer's `timed_layer` asks for it (any value: the chained launches; `layer`: a per-layer launch it selects), a HIP
    event pair on the launch stream around the body, appended as (e0, e1) + note(trainer) to `timed_events` of every trainer given -- the same pair
    on every network of a grouped launch."""
    sel = lambda t: t is not None and (layer is None or layer == t or (isinstance(t, (tuple, list, set)) and layer in t))
    if not any(sel(tr.timed_layer) for tr in trainers):
        yield
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    yield
    e1.record()
    for tr in trainers:
        tr.timed_events.append((e0, e1) + note(tr))


def _backward_note(tr):
    """`timed`'s note of a backward-data pass: dX = G W of every hidden layer but the first (whose input gradient nobody needs), 2 B C_out C_in flops each."""
    return (tr._B, 2.0 * tr._B * sum(l.weight.shape[0] * l.weight.shape[1] for l in tr.layers[1:-1]), None, "backward")


class MLPTrainer:
    """Hand-scheduled forward / backward of one of the two ELU MLPs for the full-batch PPO update (replaces autograd for
    reference utils/runner.py:132,147,163).  Same arithmetic as torch's Linear/ELU autograd, different schedule, in the form `plan` names (a NetPlan,
    set by the runner once per rollout / update; the class attributes below are its switches):
      * forward: the three hidden layers as ONE launch, activations handed on in registers and kept for the backward (bg_mlp_chain_split.hip, the
        default; bg_mlp_chain.hip on the fp32 matrix pipe), or one fused Linear + bias + ELU launch per layer (bg_mlp.hip / bg_mlp_split.hip);
      * backward-data: dX = g W, ELU' and the bias gradients of the hidden layers as one launch (bg_mlp_chain_split_bwd.hip) or one per layer;
      * weight gradients: deferred, all hidden layers of both networks in one grouped launch (GroupedWeightGrad);
      * gradients are WRITTEN into the parameters' `.grad` views of the flat Adam buffer (no AccumulateGrad adds, no zero_grad).
    The "library" forms (torch GEMMs + bg_elu_backward_colsum, split-K bmm weight gradients) serve other widths and the tests that compare forms.
    The kernels read copies of the weights (`copies`, a WeightCopies): every pass takes them through `copies.get`, which rewrites the stale ones.
    """

    # Hidden layers with K in {64, 128, 256, 512} and N % 128 == 0 run on the hand-written fused fp32-MFMA layer (bg_mlp.hip: bias + ELU in the GEMM
    # epilogue).  Measured on MI355X at M = 98,304 (tools/mlp_probe.py): 131.8 vs 151.3 us (256x256), 63.9 vs 76.3 us (256x128), 37.5 vs 55.8 us
    # (128x128) against hipBLASLt addmm + elu_.  Other shapes, or FUSED = False (a class attribute, for the tests that compare the two forms): the
    # library GEMM + elementwise ELU.
    FUSED = True

    # Opt-in (BG_GEMM_SPLIT=9 or 6): the same layers on the bf16 matrix pipe, every fp32 operand split exactly into three bf16 numbers and all 9
    # (or the 6 largest) cross products accumulated in fp32 (bg_mlp_split.hip).  0 = the fp32 MFMA kernels.
    SPLIT = int(os.environ.get("BG_GEMM_SPLIT", "0"))
    # The grouped weight-gradient launch on the bf16 matrix pipe as well (bg_wgrad_split.hip: exact 3-way splits, all 9 products, the sub-ranges of the
    # batch alternating the sign of the accumulation; its error against float64 is 0.84-0.89 of the fp32-MFMA launch's and it is 0.4 ms per iteration
    # faster in the loop: profiles/r06_wgrad_split_*).  BG_WGRAD_SPLIT=0: the fp32-MFMA launch (bg_wgrad.hip).  Applies behind the chained split kernels
    # only (UpdatePlan.wgrad); shapes outside the split kernel's four take the fp32 launch.
    WGRAD_SPLIT = int(os.environ.get("BG_WGRAD_SPLIT", "9"))

    # The forward pass of the three hidden layers as one launch (bg_mlp_chain_forward) where the widths are the reference's (CHAIN = False: one launch
    # per layer)
    CHAIN = True

    # ... and that launch on the bf16 matrix pipe with fp32 semantics (bg_mlp_chain_split.hip: every fp32 operand the exact sum of three bf16 numbers, all
    # 9 cross products accumulated in fp32 -- 9 x 32 cycles per 32 x 32 x 16 block against 8 x 64 on the fp32 pipe, error against float64 at or below the
    # fp32-MFMA chain's).  The default; BG_CHAIN_SPLIT=0 (or CHAIN_SPLIT = False) runs the fp32-MFMA chain (bg_mlp_chain.hip).
    CHAIN_SPLIT = os.environ.get("BG_CHAIN_SPLIT", "1") == "1"
    # ... and the backward-data pass of the hidden layers as one launch of the same arithmetic (bg_mlp_chain_split_bwd.hip); BG_CHAIN_SPLIT_BWD=0: one
    # fp32-MFMA launch per layer (bg_mlp_layer_backward)
    CHAIN_SPLIT_BWD = os.environ.get("BG_CHAIN_SPLIT_BWD", "1") == "1"
    # Odd 128-row slabs of the chained split kernels accumulate the NEGATED sums (planes of -W beside the planes of W) and put the sign back where a tile
    # is finished: the bf16 MFMA's accumulator does not round to nearest, every accumulated element carries a small bias of one sign, and what is summed
    # over the rows downstream (bias gradients, weight gradients) would collect it; alternating makes it cancel.  BG_CHAIN_ALTERNATE=0: off.
    CHAIN_ALTERNATE = os.environ.get("BG_CHAIN_ALTERNATE", "1") == "1"

    # Weight gradients (the dW part of loss.backward(), runner.py:163): hand-written fp32-MFMA kernel, ALL hidden layers of both networks in one
    # launch pair after both backward chains (bg_mlp_weight_grad_group, GroupedWeightGrad).  Measured on MI355X, round 2
    # (tools/archive/ab_defer.sh, update phase per iteration): library split-K bmm + sum inside the chains 24.13 ms; the hand-written kernel one layer at a
    # time inside the chains 26.46 ms (its 512-register, 128 KB-LDS workgroups cannot share a CU with the other stream's kernels); the library
    # path deferred 24.39 ms; the grouped hand-written launch 23.01 ms = 3.77 M env-steps/s against 3.61 M.  FUSED_WGRAD = False selects the library path.
    FUSED_WGRAD = True
    WGRAD_WORKGROUPS = 256  # one 4-wave workgroup per CU

    @staticmethod
    def _fusable(k_in, n_out):
        """Shapes of the per-layer forward kernels (bg_mlp.hip, bg_mlp_split.hip)."""
        return k_in in (64, 128, 256, 512) and n_out % 128 == 0

    @staticmethod
    def bwd_fusable(c_out, c_in):
        """Shapes of the per-layer backward-data kernels (bg_mlp_layer_backward*); other layers take torch.mm + bg_elu_backward_colsum."""
        return c_out in (128, 256, 512) and c_in % 128 == 0

    # ------------------------------------------------------------------ construction and workspaces
    def __init__(self, seq, max_split=32, clock=None):
        self.layers = [m for m in seq if isinstance(m, torch.nn.Linear)]
        self.max_split = max_split
        self.x = None
        self._B = self._rows = self._kin = None
        self.timed_layer, self.timed_events = None, []
        # workgroups of the full-batch chained forward launch (0: one per slab); the runner sets it when two networks' launches share the chip
        self.chain_workgroups = 0
        self.chain_bwd_workgroups = 0  # ... of the chained backward launch
        # (weight [N3], bias [1], out [rows]): a scalar output layer evaluated by the chained forward kernel itself (the critic's values); None: not
        self.value_head = None
        self.plan = None  # the NetPlan this network's passes follow: set by the runner before each rollout / update
        # the copies of the weights that the layer kernels read; clock: the WeightClock of whoever steps the optimiser (None: rewritten on every pass)
        self.copies = WeightCopies(self.layers, clock)

    def _split(self, B):
        s = self.max_split
        while s > 1 and B % s:
            s -= 1
        return s

    def _alloc(self, rows, B, dev, k_in):
        """Static workspaces (no allocator traffic inside the update loop; safe to use from a side stream).  `rows` >= B: extra inference-only
        rows may ride along in the forward pass (the critic evaluates the T+1'th observation in the same GEMMs).  `k_in` > in_features of
        the first layer means the caller zero-padded the input columns (61 -> 64, 47 -> 64) so that the first layer, too, runs on the fused kernel."""
        self._rows, self._B, self._S, self._kin = rows, B, self._split(B), k_in
        # (rows rounded up to whole 128-row slabs: the chained forward kernel stores every slab in full)
        rows_pad = (rows + 127) // 128 * 128
        self.acts = [torch.empty(rows_pad, l.weight.shape[0], dtype=torch.float32, device=dev)[:rows] for l in self.layers]
        B_pad = (B + 127) // 128 * 128  # (whole 128-row slabs: the chained backward kernel stores every slab in full)
        self.gin = [None] + [torch.empty(B_pad, l.weight.shape[1], dtype=torch.float32, device=dev)[:B] for l in self.layers[1:]]
        self.cs = [torch.empty(((B + 127) // 128) * l.weight.shape[0], dtype=torch.float32, device=dev) for l in self.layers]
        self.dw = [None] * len(self.layers)  # slices x dW of the library weight gradients (_weight_grad), created on first use
        self.copies.reset(k_in)
        self.chain_colsum = None  # the chained backward kernel's waves leave one record of column sums per slab here
        l0 = self.layers[0]  # (padded input columns: the library weight gradient of the first layer is summed at the padded width)
        self.dw0sum = torch.empty(l0.weight.shape[0], k_in, dtype=torch.float32, device=dev) if k_in != l0.weight.shape[1] else None

    def prepare(self, x, train_rows=None):
        """Workspaces for a forward pass on x (first `train_rows` rows = the batch the backward pass differentiates) without running it."""
        B = x.shape[0] if train_rows is None else train_rows
        if self._B != B or self._rows != x.shape[0] or self._kin != x.shape[1]:
            self._alloc(x.shape[0], B, x.device, x.shape[1])
        self.x = x

    # ------------------------------------------------------------------ descriptors of the chained launches
    def _chain_split(self):
        return self.plan.fwd == "chain_split"

    def _chain_split_bwd(self):
        """Does backward_hidden run as ONE launch on the bf16 matrix pipe (bg_mlp_chain_split_bwd.hip)?  Same widths as the chained forward."""
        return self.plan.bwd == "chain_split"

    def _chain_descriptor(self):
        """bg_mlp_chain of this network's hidden layers on the input of the forward pass in progress (self.x)."""
        ls, p = self.layers, _lib.ptr
        vw, vb, vo = self.value_head if self.value_head is not None else (None, None, None)
        if vo is not None and (vo.numel() < self.x.shape[0] or vw.numel() != ls[2].weight.shape[0]):
            raise ValueError("value_head: weight [width of the last hidden layer], bias [1], output [rows]")
        if self._chain_split():
            P = [self.copies.get("cplanes", i) for i in range(3)]
            return _lib.MlpChainSplit(self.x.shape[0], self._kin, ls[0].weight.shape[0], ls[1].weight.shape[0], ls[2].weight.shape[0], int(self.chain_workgroups),
                                      int(self.plan.alternate), 0, p(self.x), p(P[0]), p(P[1]), p(P[2]), p(ls[0].bias), p(ls[1].bias), p(ls[2].bias), p(self.acts[0]), p(self.acts[1]),
                                      p(self.acts[2]), p(vw), p(vb), p(vo))
        return _lib.MlpChain(self.x.shape[0], self._kin, ls[0].weight.shape[0], ls[1].weight.shape[0], ls[2].weight.shape[0], int(self.chain_workgroups), p(self.x),
                             p(self.copies.get("w0pad", 0)), p(ls[0].bias), p(ls[1].weight), p(ls[1].bias), p(ls[2].weight), p(ls[2].bias), p(self.acts[0]),
                             p(self.acts[1]), p(self.acts[2]), p(vw), p(vb), p(vo))

    def chain_rows_descriptor(self, row0, nrows):
        """bg_mlp_chain of rows [row0, row0 + nrows) of the pass prepared by `prepare` (whole 128-row slabs: the kernel stores every slab in full):
        the same launch the full-batch forward makes, restricted to these slabs -- bit-identical outputs in the same places of the activation buffers
        (and of the value head's output; slab0 tells the kernel the place of the piece's first slab in the batch).  Used by the rollout, which
        evaluates each step's rows as soon as the simulator has produced them."""
        if row0 % 128 or nrows % 128 or row0 + nrows > self.x.shape[0]:
            raise ValueError("chain_rows_descriptor: row0 and nrows must be multiples of 128 inside the prepared batch")
        d = self._chain_descriptor()
        d.M = nrows
        d.workgroups = 0  # (a few slabs during the rollout: one workgroup each)
        d.slab0 = row0 // 128  # (which slabs accumulate the negated sums follows their place in the batch, not in this launch)
        d.X = d.X + 4 * row0 * self._kin
        d.Y1, d.Y2, d.Y3 = (y + 4 * row0 * l.weight.shape[0] for y, l in zip((d.Y1, d.Y2, d.Y3), self.layers[:3]))
        if d.v_out:
            d.v_out = d.v_out + 4 * row0
        return d

    def chain_backward_descriptor(self, g=None):
        """bg_mlp_chain_split_bwd of this network's backward-data pass from g = dL/dz of the last hidden layer (default: hidden_grad)."""
        ls, B, p = self.layers, self._B, _lib.ptr
        g = self.hidden_grad if g is None else g
        PT1, PT2 = self.copies.get("cplanes_t", 1), self.copies.get("cplanes_t", 2)
        n1, n2, n3 = ls[0].weight.shape[0], ls[1].weight.shape[0], ls[2].weight.shape[0]
        slabs = (B + 127) // 128
        if self.chain_colsum is None or self.chain_colsum.numel() < slabs * 4 * (n1 + n2):  # one record of column sums per (slab, wave)
            self.chain_colsum = torch.empty(slabs * 4 * (n1 + n2), dtype=torch.float32, device=g.device)
        self._pending_wgrad = [(2, g), (1, self.gin[2]), (0, self.gin[1])]
        return _lib.MlpChainSplitBwd(B, n1, n2, n3, int(self.chain_bwd_workgroups), int(self.plan.alternate), p(g), p(PT2), p(PT1), p(self.acts[1]), p(self.acts[0]), p(self.gin[2]),
                                     p(self.gin[1]), p(self.chain_colsum), p(ls[1].bias.grad), p(ls[0].bias.grad))

    @staticmethod
    def launch_chain(descs):
        """One launch for a list of chain descriptors of one kind (all bg_mlp_chain or all bg_mlp_chain_split); a mixed list runs as two launches."""
        lib, st = _lib.load(), _lib.current_stream_ptr()
        for kind, fn, name in ((_lib.MlpChainSplit, lib.bg_mlp_chain_forward_split, "bg_mlp_chain_forward_split"),
                               (_lib.MlpChain, lib.bg_mlp_chain_forward_group, "bg_mlp_chain_forward_group")):
            sel = [d for d in descs if isinstance(d, kind)]
            if sel:
                arr = (kind * len(sel))(*sel)
                _lib.check(fn(ctypes.addressof(arr), len(sel), st), name)

    # ------------------------------------------------------------------ forward
    @staticmethod
    def _chained_forward(trainers):
        """The chained hidden layers of every (prepared) trainer in ONE launch (bg_mlp_chain.hip / bg_mlp_chain_split.hip: activations handed on in
        registers, bit-identical to the per-layer launches).  Returns their last hidden activations."""
        descs = [tr._chain_descriptor() for tr in trainers]
        with timed(trainers, lambda tr: (tr.x.shape[0], tr._kin, tuple(l.weight.shape[0] for l in tr.layers[:3]), tr.plan.fwd)):
            MLPTrainer.launch_chain(descs)
        return [tr.acts[2] for tr in trainers]

    @staticmethod
    def forward_hidden_group(jobs):
        """jobs = [(trainer, x, train_rows), ...] (at most 4, all on the chained split kernel): `forward_hidden` of every job in ONE launch -- the
        networks share the chip by their `chain_workgroups` inside one grid instead of as launches on several streams.  Same kernel code per network,
        same slabs, same order of the sums: bit-identical to the separate launches.  Returns the last hidden activations of every job."""
        for tr, x, train_rows in jobs:
            if not tr._chain_split():
                raise ValueError("forward_hidden_group: every network must run the chained split kernel")
            tr.prepare(x, train_rows)
        return MLPTrainer._chained_forward([tr for tr, _, _ in jobs])

    def forward_hidden(self, x, train_rows=None):
        """All layers but the output layer: returns the activations of the last hidden (ELU) layer [rows, width].  The output layer then runs
        fused with the loss (bg_actor_head / bg_critic_head_*), and `backward_hidden` takes over from the gradient those kernels produce."""
        return self.forward(x, train_rows, _stop_before_output=True)

    def forward(self, x, train_rows=None, _stop_before_output=False):
        """x [rows, in (possibly zero-padded)].  The first `train_rows` rows (default: all) are the batch the backward pass differentiates."""
        self.prepare(x, train_rows)
        h, first, last = x, 0, len(self.layers) - 1
        lib, stream = _lib.load(), _lib.current_stream_ptr()
        if self.plan.chained:  # the three hidden layers: the grouped launch of one network
            first, h = 3, self._chained_forward([self])[0]
        for i in range(first, last if _stop_before_output else last + 1):
            l = self.layers[i]
            n_out, k_in = l.weight.shape
            kp = self._kin if i == 0 else k_in
            if self.plan.fwd == "layer_split" and i < last and self._fusable(kp, n_out):
                _lib.check(lib.bg_mlp_layer_forward_split(h.shape[0], kp, n_out, _lib.ptr(h), _lib.ptr(self.copies.get("planes", i)), _lib.ptr(l.bias),
                                                          _lib.ptr(self.acts[i]), 1, self.plan.terms, stream), "bg_mlp_layer_forward_split")
                h = self.acts[i]
                continue
            w = l.weight if kp == k_in else self.copies.get("w0pad", 0)  # (padded input columns: the zero-padded first layer)
            if i < last and self.plan.fwd != "library" and self._fusable(kp, n_out):
                # hand-written fp32-MFMA layer with bias + ELU in the epilogue (bg_mlp.hip)
                with timed([self], lambda tr: (h.shape[0], kp, n_out, i), layer=i):
                    _lib.check(lib.bg_mlp_layer_forward(h.shape[0], kp, n_out, _lib.ptr(h), _lib.ptr(w), _lib.ptr(l.bias), _lib.ptr(self.acts[i]), 1,
                                                        stream), "bg_mlp_layer_forward")
                h = self.acts[i]
                continue
            torch.addmm(l.bias, h, w.t(), out=self.acts[i])
            h = self.acts[i]
            if i < last:
                torch.nn.functional.elu_(h)
        return h

    # ------------------------------------------------------------------ backward
    def backward(self, grad_out):
        """grad_out [B, out] is consumed (modified in place).  Fills weight.grad / bias.grad of every layer.

        g always holds dL/dz of layer i (z = pre-activation).  For the linear output layer that is grad_out itself; going down, the fused
        kernel bg_mlp_layer_backward produces dL/dz of layer i-1 = (g W_i) * elu'(a_{i-1}) together with layer i-1's bias gradient in one
        pass; the skinny output layers (12 / 1 columns) use torch.mm + the fused ELU-backward/column-sum kernel instead."""
        last = len(self.layers) - 1
        torch.sum(grad_out, dim=0, out=self.layers[last].bias.grad)  # linear output layer: plain column sum
        self._backward_from(last, grad_out)

    @property
    def hidden_grad(self):
        """[B, width] buffer the fused head kernels write dL/dz of the last hidden layer into (input of `backward_hidden`)."""
        return self.gin[len(self.layers) - 1]

    @staticmethod
    def backward_hidden_group(trainers, finishes, g=None):
        """`backward_hidden(finishes=finishes)` of every trainer (at most 4, all on the chained split backward kernel) in ONE launch; appends one
        reduction descriptor per trainer, in the order given.  g: dL/dz of the last hidden layer of a single trainer (default: each `hidden_grad`)."""
        if not all(tr._chain_split_bwd() for tr in trainers):
            raise ValueError("backward_hidden_group: every network must run the chained split backward kernel")
        with timed(trainers, _backward_note):
            ds = [tr.chain_backward_descriptor(g) for tr in trainers]
            arr = (_lib.MlpChainSplitBwd * len(ds))(*ds)
            fins = (_lib.ReduceProblem * len(ds))()
            _lib.check(_lib.load().bg_mlp_chain_backward_split(ctypes.addressof(arr), len(ds), fins, _lib.current_stream_ptr()), "bg_mlp_chain_backward_split")
            finishes.extend(fins[k] for k in range(len(ds)))

    def backward_hidden(self, g=None, finishes=None):
        """Backward from the last hidden layer down.  g = dL/dz of that layer (default: `hidden_grad`); its bias gradient and the output
        layer's weight / bias gradients have already been written by the fused head kernel.  finishes (a list): the fused backward layers run
        without their column-sum finish and append its descriptor (_lib.ReduceProblem) instead; the caller runs them later with
        utils.reduce_group (the bias gradients are not needed before the optimiser step)."""
        if not self._chain_split_bwd():
            with timed([self], _backward_note):
                self._backward_from(len(self.layers) - 2, self.hidden_grad if g is None else g, finishes)
            return
        fins = [] if finishes is None else finishes
        self.backward_hidden_group([self], fins, g)  # the grouped launch of one network
        if finishes is None:
            from .utils import reduce_group
            reduce_group(fins)

    def _backward_from(self, start, g, finishes=None):
        lib, B, stream = _lib.load(), self._B, _lib.current_stream_ptr()
        self._pending_wgrad = []
        for i in range(start, -1, -1):
            l = self.layers[i]
            a_in = (self.acts[i - 1] if i > 0 else self.x)[:B]
            C_out, C_in = l.weight.shape
            self._pending_wgrad.append((i, g))
            if i > 0:
                below = self.layers[i - 1]
                fusable = self.bwd_fusable(C_out, C_in)
                if fusable and self.plan.bwd == "layer_split":
                    _lib.check(lib.bg_mlp_layer_backward_split(B, C_out, C_in, _lib.ptr(g), _lib.ptr(self.copies.get("planes_t", i)), _lib.ptr(a_in), _lib.ptr(self.gin[i]),
                                                               _lib.ptr(below.bias.grad), _lib.ptr(self.cs[i - 1]), self.plan.terms, stream),
                               "bg_mlp_layer_backward_split")
                elif fusable and self.plan.bwd == "layer":
                    wt = self.copies.get("wt", i)
                    if finishes is not None:
                        fin = _lib.ReduceProblem()
                        _lib.check(lib.bg_mlp_layer_backward_partial(B, C_out, C_in, _lib.ptr(g), _lib.ptr(wt), _lib.ptr(a_in), _lib.ptr(self.gin[i]),
                                                                     _lib.ptr(below.bias.grad), _lib.ptr(self.cs[i - 1]), fin, stream),
                                   "bg_mlp_layer_backward_partial")
                        finishes.append(fin)
                    else:
                        _lib.check(lib.bg_mlp_layer_backward(B, C_out, C_in, _lib.ptr(g), _lib.ptr(wt), _lib.ptr(a_in), _lib.ptr(self.gin[i]),
                                                             _lib.ptr(below.bias.grad), _lib.ptr(self.cs[i - 1]), stream), "bg_mlp_layer_backward")
                else:
                    torch.mm(g, l.weight, out=self.gin[i])
                    _lib.check(lib.bg_elu_backward_colsum(B, C_in, _lib.ptr(self.gin[i]), _lib.ptr(a_in), _lib.ptr(below.bias.grad), _lib.ptr(self.cs[i - 1]),
                                                          stream), "bg_elu_backward_colsum")
                g = self.gin[i]

    # ------------------------------------------------------------------ weight gradients
    # The backward chain computes only dL/dz; the weight gradients of all layers run afterwards, when both networks' chains are done and nothing
    # else competes for the GPU: the grouped launch (GroupedWeightGrad.run); shapes outside its range run as library GEMMs there.

    def pending_wgrad_problems(self):
        """(G, A, dW, C_out, C_in (padded), C_in_real) of every deferred weight gradient, and clears the list (for the grouped launch)."""
        out = []
        for i, g in self._pending_wgrad:
            if not self.plan.grouped[i]:  # shape outside the kernel's range: the library path, now
                self._weight_grad(i, g)
                continue
            l = self.layers[i]
            a_in = (self.acts[i - 1] if i > 0 else self.x)[: self._B]
            out.append((g, a_in, l.weight.grad, l.weight.shape[0], a_in.shape[1], l.weight.shape[1]))
        self._pending_wgrad = []
        return out

    def _weight_grad(self, i, g):
        """Library path of one layer's weight gradient: a split-K batched GEMM over S slices of the batch, then a sum."""
        B, S = self._B, self._S
        l = self.layers[i]
        a_in = (self.acts[i - 1] if i > 0 else self.x)[:B]
        C_out, C_in = l.weight.shape
        if self.dw[i] is None:
            self.dw[i] = torch.empty(S, C_out, a_in.shape[1], dtype=torch.float32, device=g.device)
        if i == 0 and self.dw0sum is not None:  # padded input columns: their gradient columns are dropped
            torch.bmm(g.view(S, B // S, C_out).transpose(1, 2), a_in.view(S, B // S, self._kin), out=self.dw[0])
            torch.sum(self.dw[0], dim=0, out=self.dw0sum)
            l.weight.grad.copy_(self.dw0sum[:, :C_in])
        else:
            torch.bmm(g.view(S, B // S, C_out).transpose(1, 2), a_in.view(S, B // S, C_in), out=self.dw[i])
            torch.sum(self.dw[i], dim=0, out=l.weight.grad)


class GRUTrainer:
    """Forward / backward of a GRU cell in front of an MLPTrainer's network over the T steps of an iteration, for the recurrent student's full-batch
    update (utils/distill.py; rsl_rl's recurrent `Distillation`: back-propagation through the iteration's steps from the stored state h0).  Rows are
    [T][N] step-major, B = T N.  Same schedule rules as MLPTrainer: no library GEMM, gradients WRITTEN into the parameters' `.grad`, the weight
    gradients deferred to the grouped launch (pending_wgrad_problems), the padded copy of W_ih in a WeightCopies under the caller's clock.
      forward(x)   gi = x W_ih^T + b_ih on all B rows (bg_mlp_layer_forward on the 64-column input), then the recurrence as ONE launch
                   (bg_gru_sequence_forward) from h0 [N][H] and resets [T][N]; returns h [B][H], the trunk's input;
      backward()   behind the trunk's backward_hidden: dh_ext = G1 W1, the gradient into the trunk's input that MLPTrainer does not produce (the
                   same layer kernel on the trunk's transposed first layer), the recurrence backwards as ONE launch (bg_gru_sequence_backward), and
                   the bias gradients = the column sums of dgi and dgh in a fixed order (bg_elu_backward_colsum without an activation).
    bias_partial (PPO on a recurrent actor, algorithm.rnn_hidden_size; False: the four launches above, distillation's): the two column sums as ONE
    launch that leaves a record per 128 rows (bg_gru_bias_partial) and a reduction descriptor for the update's deferred group (backward(finishes=)).
    The rollout's side of the state lives here too (rollout_begin / rollout_reset / rollout_end): the one statement of which state the recurrence
    starts from and which env enters which step with a zero state, for Distiller and Runner alike."""

    KIN = 64  # the zero-padded width of the cell's input rows by default (47 observations)

    def __init__(self, cell, trunk, T, N, clock=None, bias_partial=False, kin=None, extra_steps=0):
        """kin: the zero-padded width of the cell's input rows (pad_input of its real width; default KIN).  extra_steps = E: forward() walks T + E steps,
        on (T + E) N rows, and backward() differentiates the first T of them (a recurrent critic, algorithm.rnn_critic: the values of the observation
        after the last step are read, never differentiated)."""
        self.cell, self.trunk, self.T, self.N, self.H = cell, trunk, int(T), int(N), int(cell.hidden_size)
        self.bias_partial = bool(bias_partial)
        self.kin = int(kin or self.KIN)
        if self.kin not in INPUT_PADS or self.kin < cell.weight_ih.shape[1]:
            raise ValueError(f"GRUTrainer: an input of {cell.weight_ih.shape[1]} columns padded to {self.kin} (one of {INPUT_PADS}, at least the cell's input)")
        self.TF = self.T + int(extra_steps)  # the steps of the forward pass
        B, H, dev = self.T * self.N, self.H, cell.weight_ih.device
        self.B, BF = B, self.TF * self.N
        self.BF = BF
        self.copies = WeightCopies([SimpleNamespace(weight=cell.weight_ih)], clock, self.kin)
        new = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
        self.gi, self.h_prev, self.h, self.gates = new(BF, 3 * H), new(BF, H), new(BF, H), new(BF, 4 * H)
        self.dh_ext, self.dgi, self.dgh = new(B, H), new(B, 3 * H), new(B, 3 * H)
        self.h0 = new(self.N, H)                                                    # the state entering the iteration (detached)
        self.resets = torch.zeros(self.TF, self.N, dtype=torch.uint8, device=dev)   # non-zero: the state entering step t of env n is zero
        self._resets = self.resets                                                  # ... as the last forward() read them (backward() reads the same)
        self._h0 = self.h0
        self.next_state = new(self.N, H) if extra_steps else None                   # carry_state()
        self._zero_bias = new(H)
        self._cs = new((B + 127) // 128 * (6 if self.bias_partial else 3) * H)  # (bias_partial: one record [6H] per 128 rows)
        self.x = None
        self._pending = False

    # ------------------------------------------------------------------ the rollout's side of the state
    def rollout_begin(self, state, last_dones):
        """At the start of a rollout: the state [N][H] the update's recurrence starts from (detached: the gradient is truncated there) and step 0's
        reset flags = the done flags of the previous iteration's last step."""
        self.h0.copy_(state)
        self.resets[0].copy_(last_dones)

    @staticmethod
    def rollout_reset(n, last_dones, dones):
        """The reset flags [N] of step n's launch: an env that the step before reset enters with a zero state."""
        return last_dones if n == 0 else dones[n - 1]

    def rollout_end(self, dones, last_dones=None):
        """Behind the last step: the reset flags of the update's recurrence (row t = the done flags of step t - 1, for every step the forward pass
        walks), and the last step's done flags for the next iteration's step 0 (last_dones = None: another cell's call keeps them)."""
        if self.TF > 1:
            self.resets[1:].copy_(dones[: self.TF - 1])
        if last_dones is not None:
            last_dones.copy_(dones[self.T - 1])

    def carry_state(self):
        """A cell that no rollout launch advances (extra_steps: the critic's): the state the next iteration starts from is this cell's output on step
        T - 1, taken from a forward pass on the parameters the rollout ran on (the update's first, before any optimiser step), on the current stream
        right behind that pass.  It enters step T, and the next iteration's step 0, through that step's reset flags.  rollout_begin(next_state, ...)
        then starts the next iteration from it."""
        self.next_state.copy_(self.h[(self.T - 1) * self.N : self.T * self.N])

    # ------------------------------------------------------------------ the update's passes
    def _input_side(self, x, h0, resets):
        """gi = x W_ih^T + b_ih on all rows of the forward pass; returns the recurrence's problem (bg_gru_forward_problem) on this trainer's buffers."""
        lib, st, p, c, H = _lib.load(), _lib.current_stream_ptr(), _lib.ptr, self.cell, self.H
        self.x = x
        h0, self._resets = self.h0 if h0 is None else h0, self.resets if resets is None else resets
        if h0.shape != self.h0.shape or self._resets.shape != self.resets.shape or self._resets.dtype != torch.uint8 or not (h0.is_contiguous() and self._resets.is_contiguous()):
            raise ValueError(f"GRUTrainer.forward: h0 {tuple(h0.shape)} / resets {tuple(self._resets.shape)} are not contiguous [{self.N}][{H}] / uint8 [{self.TF}][{self.N}]")
        if x.shape != (self.BF, self.kin) or not x.is_contiguous():
            raise ValueError(f"GRUTrainer.forward: x {tuple(x.shape)} is not contiguous [{self.BF}][{self.kin}]")
        self._h0 = h0
        _lib.check(lib.bg_mlp_layer_forward(self.BF, self.kin, 3 * H, p(x), p(self.copies.get("w0pad", 0)), p(c.bias_ih), p(self.gi), 0, st), "bg_mlp_layer_forward")
        return _lib.GruForwardProblem(self.TF, self.N, p(self.gi), p(h0), p(self._resets), p(c.weight_hh), p(c.bias_hh), p(self.h_prev), p(self.h), p(self.gates))

    def forward(self, x, h0=None, resets=None):
        """h0 [N][H] / resets [T][N] uint8: the state the recurrence starts from and the reset flags it (and the backward pass behind it) reads, where
        they are not this trainer's own (an env-wise mini-batch: rows of the runner's gathered buffers)."""
        q = self._input_side(x, h0, resets)
        _lib.check(_lib.load().bg_gru_sequence_forward(q.T, q.N, self.H, q.gi, q.h0, q.reset, q.W_hh, q.b_hh, q.h_prev, q.h, q.gates, _lib.current_stream_ptr()),
                   "bg_gru_sequence_forward")
        return self.h

    @staticmethod
    def forward_group(jobs):
        """jobs = [(trainer, x, h0, resets), ...] (1 to 4 cells of one width): `forward` of every job with the recurrences as ONE launch
        (bg_gru_sequence_forward_group: the single launches' code per cell, bit-identical outputs).  Returns every job's h."""
        qs = [tr._input_side(x, h0, resets) for tr, x, h0, resets in jobs]
        arr = (_lib.GruForwardProblem * len(qs))(*qs)
        _lib.check(_lib.load().bg_gru_sequence_forward_group(arr, len(qs), jobs[0][0].H, _lib.current_stream_ptr()), "bg_gru_sequence_forward_group")
        return [tr.h for tr, _, _, _ in jobs]

    def _trunk_side(self):
        """dh_ext = G1 W1 behind the trunk's backward_hidden; returns the backward recurrence's problem (bg_gru_backward_problem)."""
        lib, st, p, c, H, tr = _lib.load(), _lib.current_stream_ptr(), _lib.ptr, self.cell, self.H, self.trunk
        g1, l0 = tr.gin[1], tr.layers[0]  # dL/dz of the trunk's first layer [B][out], behind backward_hidden
        _lib.check(lib.bg_mlp_layer_forward(self.B, l0.weight.shape[0], H, p(g1), p(tr.copies.get("wt", 0)), p(self._zero_bias), p(self.dh_ext), 0, st),
                   "bg_mlp_layer_forward")
        return _lib.GruBackwardProblem(self.T, self.N, p(self.dh_ext), p(self.gates), p(self.h_prev), p(self._resets), p(c.weight_hh), p(self.dgi), p(self.dgh), None)

    def _bias_side(self, finishes):
        lib, st, p, c, H = _lib.load(), _lib.current_stream_ptr(), _lib.ptr, self.cell, self.H
        self._pending = True
        if self.bias_partial:
            _lib.check(lib.bg_gru_bias_partial(self.B, H, p(self.dgi), p(self.dgh), p(self._cs), st), "bg_gru_bias_partial")
            fin = self.bias_finish()
            if finishes is not None:
                finishes.append(fin)
            else:
                from .utils import reduce_group
                reduce_group([fin])
            return
        for g, b in ((self.dgi, c.bias_ih), (self.dgh, c.bias_hh)):
            _lib.check(lib.bg_elu_backward_colsum(self.B, 3 * H, p(g), None, p(b.grad), p(self._cs), st), "bg_elu_backward_colsum")

    def backward(self, finishes=None):
        """finishes (a list; bias_partial only): receives the descriptor of the bias gradients' reduction, for the caller's deferred group; None: it
        runs here, as a bg_reduce_group of its own.  Differentiates the first T steps of the forward pass."""
        q = self._trunk_side()
        _lib.check(_lib.load().bg_gru_sequence_backward(q.T, q.N, self.H, q.dh_ext, q.gates, q.h_prev, q.reset, q.W_hh, q.dgi, q.dgh, None, _lib.current_stream_ptr()),
                   "bg_gru_sequence_backward")
        self._bias_side(finishes)

    @staticmethod
    def backward_group(trainers, finishes=None):
        """`backward(finishes)` of every trainer (1 to 4 cells of one width) with the recurrences as ONE launch (bg_gru_sequence_backward_group)."""
        qs = [tr._trunk_side() for tr in trainers]
        arr = (_lib.GruBackwardProblem * len(qs))(*qs)
        _lib.check(_lib.load().bg_gru_sequence_backward_group(arr, len(qs), trainers[0].H, _lib.current_stream_ptr()), "bg_gru_sequence_backward_group")
        for tr in trainers:
            tr._bias_side(finishes)

    def bias_finish(self):
        """The bg_reduce_problem behind bg_gru_bias_partial: the records [ceil(B / 128)][6H] added up into bias_ih.grad | bias_hh.grad."""
        c, H, fin = self.cell, self.H, _lib.ReduceProblem()
        fin.partial, fin.groups, fin.record, fin.n_out = self._cs.data_ptr(), (self.B + 127) // 128, 6 * H, 6 * H
        fin.out[0], fin.out[1], fin.n[0], fin.n[1] = c.bias_ih.grad.data_ptr(), c.bias_hh.grad.data_ptr(), 3 * H, 3 * H
        return fin

    def pending_wgrad_problems(self):
        """(G, A, dW, C_out, C_in (padded), C_in_real) of the cell's two weight gradients, for the grouped launch (GroupedWeightGrad.run): on the B rows
        the backward pass differentiated."""
        if not self._pending:
            return []
        self._pending, c, H, B = False, self.cell, self.H, self.B
        return [(self.dgi, self.x[:B], c.weight_ih.grad, 3 * H, self.kin, c.weight_ih.shape[1]), (self.dgh, self.h_prev[:B], c.weight_hh.grad, 3 * H, H, H)]


class EstimatorActor(torch.nn.Module):
    """What export_model.py scripts for a checkpoint with a state estimator: actor(cat(x, estimator(x)[:, :E])) on rows x of 47 H observations -- the
    deploy contract stays "47 H floats in, 12 out"."""

    def __init__(self, actor, estimator, estimator_cols):
        super().__init__()
        self.actor, self.estimator, self.estimator_cols = actor, estimator, int(estimator_cols)

    def forward(self, x):
        return self.actor(torch.cat((x, self.estimator(x)[..., : self.estimator_cols]), dim=-1))


class RecurrentActor(torch.nn.Module):
    """What export_model.py scripts for a recurrent student (distillation.student_memory): forward(obs [B][47]) -> [B][12] advances the hidden state,
    a buffer this module owns (zero at first and again whenever B changes), by one GRU step and returns the actor's mean on the new state; reset()
    (an exported method) zeroes it: call it where the robot's episode starts."""

    def __init__(self, memory, actor):
        super().__init__()
        self.memory, self.actor, self.hidden = memory, actor, int(memory.hidden_size)
        self.register_buffer("h", torch.zeros(0, self.hidden))

    def forward(self, x):
        if self.h.shape[0] != x.shape[0]:
            self.h = torch.zeros(x.shape[0], self.hidden, dtype=x.dtype, device=x.device)
        self.h = self.memory(x, self.h)
        return self.actor(self.h)

    @torch.jit.export
    def reset(self):
        self.h = torch.zeros_like(self.h)


class ActorCritic(torch.nn.Module):
    """estimator_hidden (estimator.enabled, utils/estimator.py; None = without, exactly the reference's parameters in the reference's order): a third
    network `estimator`, num_obs -> estimator_hidden -> 12, registered behind `logstd`; the actor then takes num_obs + estimator_cols inputs, the
    observations and the first estimator_cols = E of the estimator's 12 outputs.  num_obs stays the env's row (47 H): what callers pass as `obs`.
    memory_hidden = H > 0 (a recurrent student, distillation.student_memory; 0 = without, today's parameters in today's order): a
    torch.nn.GRUCell(num_obs, H) `memory`, registered last, and the actor takes the H values of its new state instead of the observations.
    critic_memory_hidden = H > 0 (a recurrent critic, algorithm.rnn_critic; 0 = without, today's parameters in today's order): a
    torch.nn.GRUCell(num_obs + num_privileged_obs, H) `critic_memory`, registered behind `memory`, and the critic's first layer takes the H values of
    its state instead of the rows.  Its state belongs to whoever walks the rows (the runner's update); est_value on single rows raises.
    rnd = (state width, predictor_hidden, target_hidden, seed) (rnd.enabled, utils/rnd.py; None = without, today's parameters in today's order and
    today's draws of the global generator): two more networks, `rnd_predictor` and `rnd_target`, registered last; nothing of this class evaluates them."""

    def __init__(self, num_act, num_obs, num_privileged_obs, actor_hidden=ACTOR_HIDDEN, critic_hidden=CRITIC_HIDDEN, estimator_hidden=None, estimator_cols=0,
                 memory_hidden=0, critic_memory_hidden=0, rnd=None):
        super().__init__()
        self.memory_hidden = int(memory_hidden or 0)
        self.critic_memory_hidden = int(critic_memory_hidden or 0)
        if self.memory_hidden and estimator_hidden is not None:
            raise ValueError("memory_hidden: a recurrent actor with a state estimator is not supported")
        self.actor_hidden, self.critic_hidden = tuple(actor_hidden), tuple(critic_hidden)
        self.estimator_hidden = None if estimator_hidden is None else tuple(estimator_hidden)
        self.estimator_cols = int(estimator_cols) if estimator_hidden is not None else 0
        if estimator_hidden is not None and not 1 <= self.estimator_cols <= _lib.NUM_DOFS:
            raise ValueError(f"estimator_cols = {estimator_cols!r}: 1 to {_lib.NUM_DOFS} of the estimator's outputs enter the actor")
        self.critic = _mlp(self.critic_memory_hidden or num_obs + num_privileged_obs, self.critic_hidden, 1)
        self.actor = _mlp(self.memory_hidden or num_obs + self.estimator_cols, self.actor_hidden, num_act)
        self.logstd = torch.nn.parameter.Parameter(torch.full((1, num_act), fill_value=-2.0), requires_grad=True)
        if estimator_hidden is not None:
            self.estimator = _mlp(num_obs, self.estimator_hidden, _lib.NUM_DOFS)
        if self.memory_hidden:
            self.memory = torch.nn.GRUCell(num_obs, self.memory_hidden)
        if self.critic_memory_hidden:
            self.critic_memory = torch.nn.GRUCell(num_obs + num_privileged_obs, self.critic_memory_hidden)
        if rnd is not None:
            self._add_rnd(*rnd)
        self._memory_state, self._gru_key, self._gru_descs = None, None, None
        self._sample_key, self._sample_layers = None, None
        self._est_key, self._est_layers = None, None
        self._packed = None  # pack_actor()

    @property
    def has_estimator(self):
        return self.estimator_hidden is not None

    def _add_rnd(self, width, predictor_hidden, target_hidden, seed):
        """rnd.enabled (utils/rnd.py): `rnd_predictor` and `rnd_target`, width -> hidden -> 12, registered last.  Built with the global generator's
        state put back behind them and initialised (torch.nn.Linear's rule: uniform in +- 1 / sqrt(fan_in), weights and biases) from a generator
        of their own seeded with `seed`, so every other draw of the process is as without them.  The target is never trained: no gradients."""
        with torch.random.fork_rng(devices=[]):
            self.rnd_predictor = _mlp(width, tuple(predictor_hidden), _lib.NUM_DOFS)
            self.rnd_target = _mlp(width, tuple(target_hidden), _lib.NUM_DOFS)
        g = torch.Generator().manual_seed(int(seed))
        with torch.no_grad():
            for net in (self.rnd_predictor, self.rnd_target):
                for m in net:
                    if isinstance(m, torch.nn.Linear):
                        bound = 1.0 / math.sqrt(m.in_features)
                        m.weight.uniform_(-bound, bound, generator=g)
                        m.bias.uniform_(-bound, bound, generator=g)
        for p in self.rnd_target.parameters():
            p.requires_grad_(False)

    def ppo_parameters(self):
        """What PPO's optimiser holds: critic, actor, logstd in the module's order (all parameters of a model without an estimator); the estimator's
        and the RND predictor's are stepped by optimisers of their own, the RND target's by none."""
        return [p for n, p in self.named_parameters() if not n.startswith(("estimator.", "rnd_predictor.", "rnd_target."))]

    def actor_input(self, obs):
        """The actor's row of observation rows: obs itself, or [obs | the first E of the estimator's outputs]."""
        if not self.has_estimator:
            return obs
        return torch.cat((obs, self.estimator(obs)[..., : self.estimator_cols]), dim=-1)

    def reset_memory(self):
        """Zero the hidden state that sample_actions carries for a model with memory (with env.reset()); nothing to do without one."""
        if self._memory_state is not None:
            self._memory_state.zero_()

    def memory_state(self, N, device):
        """The hidden state [N][H] that sample_actions advances in place: created (zero) on first use and when N or the device changes."""
        if self._memory_state is None or self._memory_state.shape[0] != N or self._memory_state.device != torch.device(device):
            self._memory_state = torch.zeros(N, self.memory_hidden, dtype=torch.float32, device=device)
        return self._memory_state

    def act(self, obs):
        if self.memory_hidden:
            raise ValueError("act: a model with memory is stateful; sample_actions carries its hidden state (the rollout of PPO on a recurrent actor, "
                             "algorithm.rnn_hidden_size, and of a recurrent student's play)")
        mean = self.actor(self.actor_input(obs))
        return torch.distributions.Normal(mean, torch.exp(self.logstd).expand_as(mean))

    def est_value(self, obs, privileged_obs):
        if self.critic_memory_hidden:
            raise ValueError("est_value: a critic with memory is stateful; the update walks the iteration's rows from the state it carries "
                             "(algorithm.rnn_critic)")
        return self.critic(torch.cat((obs, privileged_obs), dim=-1)).squeeze(-1)

    # ---- fused rollout inference (reference runner.py:109-111: dist = model.act(obs); act = dist.sample())
    def _sample_params(self):
        lin = [m for m in self.actor if isinstance(m, torch.nn.Linear)]
        return lin, [t for l in lin for t in (l.weight, l.bias)] + [self.logstd]

    def pack_actor(self):
        """The actor's parameters as bg_actor_sample reads them (bg_actor_pack: one small launch on the current stream into a buffer this model keeps),
        or None where the architecture samples through bg_actor_sample_mlp, which reads the parameters themselves.  The packed copy is a snapshot:
        whoever passes it to sample_actions packs again after anything that may have changed a parameter (the rollout: at its start, every iteration)."""
        lin, w = self._sample_params()
        if self.actor_hidden != ACTOR_HIDDEN or lin[0].in_features != _lib.NUM_OBS or self.has_estimator or self.memory_hidden:
            return None
        if not w[0].is_cuda:
            raise RuntimeError("pack_actor runs a HIP kernel and needs CUDA parameters")
        for t in w:
            if not t.is_contiguous():
                raise RuntimeError("pack_actor needs contiguous parameters")
        if self._packed is None or self._packed.device != w[0].device:
            self._packed = torch.empty(_lib.ACTOR_PACKED_FLOATS, dtype=torch.float32, device=w[0].device)
        _lib.check(_lib.load().bg_actor_pack(*[_lib.ptr(t) for t in w], _lib.ptr(self._packed), _lib.current_stream_ptr()), "bg_actor_pack")
        return self._packed

    def sample_actions(self, obs, actions_out, seed, counter, mu_out=None, scan=0, packed=None, est_out=None, reset=None):
        """One launch: the actor's mean and a Gaussian sample around it.  The reference's widths on 47 inputs run bg_actor_sample (its widths built
        into the kernel) on a packed copy of the parameters: `packed` from pack_actor() where the caller knows that no parameter has changed since
        (the rollout packs once for its 24 steps), else packed here, one more small launch.  Every other architecture, and every actor on a frame stack
        (47 H inputs, env.frame_stack), runs bg_actor_sample_mlp (widths from descriptors, the weights read from the parameters themselves); both draw
        the same noise for the same seed and counter.  scan = P (terrain.actor_heights): the rows end with the height scan's P values behind the 47 H
        observations (bg_actor_sample_mlp_scan, the same kernel).  A model with an estimator runs bg_actor_sample_est, both networks in one launch:
        obs has the env's 47 H columns and est_out [N][12] (required) receives the estimator's 12 means, the first E of which the actor has read.
        A model with memory runs bg_actor_sample_gru on a state tensor [N][H] it owns (zero on first use and when N changes; reset_memory() zeroes
        it), updated in place; reset [N] (bool or uint8, optional): the rows whose state is read as zero, the env's done flags of the step before."""
        if not obs.is_cuda:
            raise RuntimeError("sample_actions runs the fused HIP actor kernel and needs CUDA tensors")
        lin, w = self._sample_params()
        for t in w + [obs, actions_out]:
            if not t.is_contiguous():
                raise RuntimeError("sample_actions needs contiguous tensors")
        if self.has_estimator:
            return self._sample_actions_est(obs, actions_out, seed, counter, mu_out, scan, est_out, lin, w)
        if self.memory_hidden:
            return self._sample_actions_gru(obs, actions_out, seed, counter, mu_out, scan, reset, lin, w)
        if self.actor_hidden == ACTOR_HIDDEN and lin[0].in_features == _lib.NUM_OBS:
            if packed is None:
                packed = self.pack_actor()
            _lib.check(_lib.load().bg_actor_sample(obs.shape[0], _lib.ptr(obs), _lib.ptr(packed), int(seed), int(counter), _lib.ptr(mu_out),
                                                   _lib.ptr(actions_out), _lib.current_stream_ptr()), "bg_actor_sample")
            return actions_out
        if obs.shape[-1] != lin[0].in_features:  # (the kernel takes the row stride from the first layer's descriptor)
            raise ValueError(f"sample_actions: observations of {obs.shape[-1]} columns, the actor takes {lin[0].in_features}")
        key = tuple(t.data_ptr() for t in w)
        if key != self._sample_key:  # descriptors of the current parameter storage (the optimiser moves it into its flat buffer once)
            self._sample_layers, self._sample_key = layer_descriptors(lin), key
        if scan:
            _lib.check(_lib.load().bg_actor_sample_mlp_scan(obs.shape[0], _lib.ptr(obs), len(lin), self._sample_layers, int(scan), _lib.ptr(self.logstd), int(seed),
                                                            int(counter), _lib.ptr(mu_out), _lib.ptr(actions_out), _lib.current_stream_ptr()),
                       "bg_actor_sample_mlp_scan")
            return actions_out
        _lib.check(_lib.load().bg_actor_sample_mlp(obs.shape[0], _lib.ptr(obs), len(lin), self._sample_layers, _lib.ptr(self.logstd), int(seed), int(counter),
                                                   _lib.ptr(mu_out), _lib.ptr(actions_out), _lib.current_stream_ptr()), "bg_actor_sample_mlp")
        return actions_out

    def _sample_actions_est(self, obs, actions_out, seed, counter, mu_out, scan, est_out, lin, w):
        """sample_actions of a model with an estimator: ONE launch (bg_actor_sample_est) runs the estimator on obs, writes its 12 means to est_out and
        samples from the actor on [obs | the first E means]."""
        elin = [m for m in self.estimator if isinstance(m, torch.nn.Linear)]
        if scan:
            raise ValueError("sample_actions: a model with an estimator takes no height scan in the actor's row (terrain.actor_heights)")
        if est_out is None:
            raise ValueError("sample_actions: a model with an estimator needs est_out, a [N][12] tensor for the estimator's means (a scratch tensor for "
                             "callers that do not keep them)")
        if (not est_out.is_cuda or not est_out.is_contiguous() or est_out.dtype != torch.float32 or tuple(est_out.shape) != (obs.shape[0], _lib.NUM_DOFS)):
            raise ValueError(f"sample_actions: est_out must be a contiguous float32 CUDA tensor of shape [{obs.shape[0]}][{_lib.NUM_DOFS}]")
        if obs.shape[-1] != elin[0].in_features:
            raise ValueError(f"sample_actions: observations of {obs.shape[-1]} columns, the estimator takes {elin[0].in_features}")
        ew = [t for l in elin for t in (l.weight, l.bias)]
        for t in ew:
            if not t.is_contiguous():
                raise RuntimeError("sample_actions needs contiguous tensors")
        key = tuple(t.data_ptr() for t in w + ew)
        if key != self._est_key:  # descriptors of the current parameter storage of both networks
            self._est_layers, self._est_key = (layer_descriptors(elin), layer_descriptors(lin)), key
        ed, ad = self._est_layers
        _lib.check(_lib.load().bg_actor_sample_est(obs.shape[0], _lib.ptr(obs), len(elin), ed, self.estimator_cols, len(lin), ad, _lib.ptr(self.logstd), int(seed),
                                                   int(counter), _lib.ptr(est_out), _lib.ptr(mu_out), _lib.ptr(actions_out), _lib.current_stream_ptr()),
                   "bg_actor_sample_est")
        return actions_out

    def gru_descriptor(self):
        """bg_gru_desc of `memory` on its current parameter storage."""
        m = self.memory
        return _lib.GruDesc(m.weight_ih.data_ptr(), m.weight_hh.data_ptr(), m.bias_ih.data_ptr(), m.bias_hh.data_ptr(), m.input_size, m.hidden_size)

    def _sample_actions_gru(self, obs, actions_out, seed, counter, mu_out, scan, reset, lin, w):
        """sample_actions of a model with memory: ONE launch (bg_actor_sample_gru) advances the state this model keeps and samples from the actor on it."""
        if scan:
            raise ValueError("sample_actions: a model with memory takes no height scan in the actor's row (terrain.actor_heights)")
        N, m = obs.shape[0], self.memory
        if obs.shape[-1] != m.input_size:
            raise ValueError(f"sample_actions: observations of {obs.shape[-1]} columns, the memory takes {m.input_size}")
        if reset is not None:
            if reset.dtype == torch.bool:
                reset = reset.view(torch.uint8)
            if reset.dtype != torch.uint8 or not reset.is_cuda or not reset.is_contiguous() or reset.numel() != N:
                raise ValueError(f"sample_actions: reset must be a contiguous bool or uint8 CUDA tensor of {N} entries")
        mw = [m.weight_ih, m.weight_hh, m.bias_ih, m.bias_hh]
        for t in mw:
            if not t.is_contiguous():
                raise RuntimeError("sample_actions needs contiguous tensors")
        h = self.memory_state(N, obs.device)
        key = tuple(t.data_ptr() for t in w + mw)
        if key != self._gru_key:
            self._gru_descs, self._gru_key = (self.gru_descriptor(), layer_descriptors(lin)), key
        gd, layers = self._gru_descs
        _lib.check(_lib.load().bg_actor_sample_gru(N, _lib.ptr(obs), obs.shape[-1], gd, len(lin), layers, _lib.ptr(self.logstd), int(seed), int(counter),
                                                   _lib.ptr(reset), _lib.ptr(h), _lib.ptr(h), _lib.ptr(mu_out), _lib.ptr(actions_out), _lib.current_stream_ptr()),
                   "bg_actor_sample_gru")
        return actions_out
