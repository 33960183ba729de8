"""The supervised update, written once for the distilled student (utils/distill.py) and the state estimator (utils/estimator.py)."""
import torch

from .. import _lib
from .model import GroupedWeightGrad, GRUTrainer, MLPTrainer, plan_network, wgrad_products
from .utils import head_scratch, reduce_group


class SupervisedTrainer:
    """Trains a 12-output MLP, optionally behind a GRU cell, onto [B][12] targets with full-batch steps and no library GEMM; the epoch loop, the loss
    normalisation and what becomes of the statistics stay with the callers.  Owns the MLPTrainer over `net` under `clock` (the WeightClock of the
    parameters `optimizer` steps), with `cell` the GRUTrainer around it over `steps` steps of rows / steps envs each (the network then reads the cell's
    state), the grouped weight-gradient launch, the head's scratch and `stats` (float64: a step's squared errors; with n_stats = 2 the squared mean
    asymmetries behind them).  `rows` is what the hidden layers run on (twice the targets' rows with a symmetry loss), `kin` the zero-padded width
    of the input, `name` what the ValueErrors start with."""

    def __init__(self, name, net, optimizer, clock, rows, kin, cell=None, steps=None, n_stats=1):
        self.name, self.optimizer, self.clock, self.rows, self.kin = name, optimizer, clock, int(rows), int(kin)
        self.mlp = MLPTrainer(net, clock=clock)
        self.gru = GRUTrainer(cell, self.mlp, steps, self.rows // steps, clock=clock) if cell is not None else None
        self.wgrad = GroupedWeightGrad()
        dev = self.mlp.layers[0].weight.device
        self.head_scratch = head_scratch(dev)
        self.stats = torch.zeros(n_stats, dtype=torch.float64, device=dev)
        self.plan, self.wgrad_terms = None, 0

    def resolve_plan(self):
        """The network's NetPlan of MLPTrainer's switches as they are now (process-wide: a caller that lets them change re-resolves) and the products
        of its grouped weight-gradient launch; ValueError where a pass would fall to a library GEMM or a layer's weight gradient is not grouped."""
        tr, rows, kin, sw = self.mlp, self.rows, self.kin, MLPTrainer
        widths = (tr.layers[0].in_features,) + tuple(l.out_features for l in tr.layers)
        if self.gru is not None:  # the network's input is the cell's state [rows][H]: the per-layer fp32 kernels (the chains take a 64-column input only)
            plan = plan_network(widths, self.gru.H, rows, 0, True, False, False, False, False, True)
        else:
            plan = plan_network(widths, kin, rows, sw.SPLIT, sw.FUSED, sw.CHAIN, sw.CHAIN_SPLIT, sw.CHAIN_SPLIT_BWD, sw.CHAIN_ALTERNATE, sw.FUSED_WGRAD)
        if "library" in (plan.fwd, plan.bwd) or not all(plan.grouped[:-1]):
            raise ValueError(f"{self.name}: a batch of {rows} rows (from runner.horizon_length x env.num_envs) is outside the range of the layer kernels (an "
                             "even number of 64 rows or more)")
        shapes = [(co, ci) for ci, co in zip((kin,) + widths[1:-2], widths[1:-1])]
        # by runner.plan_update's rule: the bf16 splits behind the chained split backward only; the cell's weight gradients run the fp32 form
        self.wgrad_terms = 0 if self.gru is not None else wgrad_products(rows, shapes, plan.bwd == "chain_split", sw.SPLIT, sw.WGRAD_SPLIT)
        self.plan = tr.plan = plan
        return plan

    def step(self, x, target, symmetry=None):
        """One optimiser step of sum |net(x) - target|^2 / (12 B) on the B rows of `target`; symmetry = (coef, (act_src, act_sign)): x holds 2B rows,
        the batch and behind it its mirror images, and the loss carries coef x the squared mean asymmetry (bg_distill_head_sym).  Leaves the step's
        sums in `stats`, writes none of the trainers' weight copies and ticks the clock, so the next pass rewrites them."""
        tr, gru, B, p = self.mlp, self.gru, target.shape[0], _lib.ptr
        out, hid = tr.layers[-1], tr.layers[-2]
        self.stats.zero_()
        h = tr.forward_hidden(x if gru is None else gru.forward(x))
        fin, fins = _lib.ReduceProblem(), []
        name = "bg_distill_head_partial" if symmetry is None else "bg_distill_head_sym_partial"
        sym_args = () if symmetry is None else (symmetry[0], *symmetry[1])
        _lib.check(getattr(_lib.load(), name)(B, p(h), p(out.weight), p(out.bias), p(target), *sym_args, None, p(tr.hidden_grad), p(out.weight.grad),
                                              p(out.bias.grad), p(hid.bias.grad), p(self.stats), p(self.head_scratch), fin, _lib.current_stream_ptr()), name)
        tr.backward_hidden(finishes=fins)
        if gru is not None:
            gru.backward()  # (no finishes list: the cell's backward in its four-launch form, the bias gradients' column sums among them)
        self.wgrad.run((tr,) if gru is None else (tr, gru), self.wgrad_terms, False)
        reduce_group([fin] + fins)
        self.optimizer.step()
        self.clock.tick()
