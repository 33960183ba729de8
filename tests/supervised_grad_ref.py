"""The gradient of one optimiser step of SupervisedTrainer.step (utils/supervised.py: the distilled student's and the state estimator's one update),
restated in float64 autograd on the step's own inputs -- TEST INFRASTRUCTURE, not a test file; the sibling of tests/update_grad_ref.py.

record_supervised_steps(sup)     records, around every call of sup.step, what the step's gradient is a function of and the gradient the step left
                                 in FlatAdam.grad in front of bg_adam_step.  It changes no switch and no plan (asserted).
supervised_gradients_f64(...)    evaluates the loss SupervisedTrainer.step's docstring states on such a record with torch autograd and returns
                                 {name: gradient}.

Names: the network's parameters are "net.<index in the Sequential>.weight" / ".bias" (Linear layers alternate with ELUs: 0, 2, 4, ...), a cell's are
"memory.weight_ih" / "weight_hh" / "bias_ih" / "bias_hh" -- derived from the trainer itself, so the one recorder serves Distiller (student.actor,
student.memory) and EstimatorTrainer (model.estimator) alike."""
import contextlib

import torch


def trained_names(sup):
    """{name: parameter} of what sup.optimizer steps, in the optimiser's order; every tensor of the optimiser must be one of the trainer's."""
    named = []
    if sup.gru is not None:
        named += [("memory." + k, p) for k, p in sup.gru.cell.named_parameters()]
    for i, l in enumerate(sup.mlp.layers):
        named += [(f"net.{2 * i}.weight", l.weight), (f"net.{2 * i}.bias", l.bias)]
    by_id = {id(p): k for k, p in named}
    assert all(id(p) in by_id for p in sup.optimizer.params) and len(sup.optimizer.params) == len(named), "the optimiser holds other tensors than the trainer's"
    return {by_id[id(p)]: p for p in sup.optimizer.params}


def net_factory(sup):
    """make_net for a trainer's network: model._mlp's constructor call on the widths of its layers."""
    from booster_gym_amd.utils.model import _mlp

    ls = sup.mlp.layers
    return lambda: _mlp(ls[0].in_features, [l.out_features for l in ls[:-1]], ls[-1].out_features)


def cell_factory(sup):
    """make_cell for a trainer's GRU cell, None without one."""
    if sup.gru is None:
        return None
    c = sup.gru.cell
    return lambda: torch.nn.GRUCell(c.input_size, c.hidden_size)


@contextlib.contextmanager
def record_supervised_steps(sup):
    """`with record_supervised_steps(sup) as steps: distiller.update()` -- steps: one dict per optimiser step, in order:
      params     {name: clone} of the tensors sup.optimizer.params holds in front of the step (trained_names)
      x, target  the step's input rows [rows (x 2 with a symmetry loss)][padded width] and its targets [rows][12]
      symmetry   None, or (coef, act_src [12] int64, act_sign [12] float64): the arguments bg_distill_head_sym_partial read
      rows       target.shape[0], the B of the loss's 1 / (12 B)
      h0, resets   with a cell only: sup.gru.h0 [N][H] and sup.gru.resets uint8 [T][N], what the step's recurrence starts from
      plan, wgrad_terms   sup.plan and sup.wgrad_terms as the step ran under them
      grads      {name: clone} of the parameters' .grad views of FlatAdam.grad in front of bg_adam_step (no form of the step writes the clipped
                 gradient back, so this is the complete unclipped one)
      clip_sqnorm   FlatAdam._gnorm behind the step: the squared norm the clip divided by
      stats      a clone of sup.stats behind the step (float64: the squared errors; with a symmetry loss the squared mean asymmetries behind them)."""
    from booster_gym_amd.utils.model import MLPTrainer

    steps, opt = [], sup.optimizer
    switches = lambda: {k: getattr(MLPTrainer, k) for k in ("FUSED", "SPLIT", "WGRAD_SPLIT", "CHAIN", "CHAIN_SPLIT", "CHAIN_SPLIT_BWD", "CHAIN_ALTERNATE", "FUSED_WGRAD")}
    before = switches()
    assert "step" not in vars(sup) and "step" not in vars(opt), "a recorder is already installed"
    inner, opt_step = sup.step, opt.step

    def recorded(x, target, symmetry=None):
        names = trained_names(sup)
        rec = dict(params={k: p.detach().clone() for k, p in names.items()}, x=x.clone(), target=target.clone(), rows=int(target.shape[0]),
                   plan=sup.plan, wgrad_terms=sup.wgrad_terms, symmetry=None)
        if symmetry is not None:
            coef, (src, sign) = symmetry
            rec["symmetry"] = (float(coef), torch.tensor([int(v) for v in src], dtype=torch.long), torch.tensor([float(v) for v in sign], dtype=torch.float64))
        if sup.gru is not None:
            rec.update(h0=sup.gru.h0.clone(), resets=sup.gru.resets.clone())

        def spy():
            assert "grads" not in rec, "the step called the optimiser twice"
            rec["grads"] = {k: p.grad.clone() for k, p in names.items()}
            opt_step()
            rec["clip_sqnorm"] = opt._gnorm.clone().sum()

        opt.step = spy
        try:
            inner(x, target, symmetry)
        finally:
            del opt.step
        assert "grads" in rec, "the step did not call the optimiser"
        assert sup.plan == rec["plan"] and sup.wgrad_terms == rec["wgrad_terms"], "the plan changed inside the step"
        rec["stats"] = sup.stats.clone()
        steps.append(rec)

    sup.step = recorded
    try:
        yield steps
    finally:
        del sup.step  # (the instance attribute: the class's method is back)
        assert "step" not in vars(opt) and switches() == before, "the recorder changed a switch"


def _mirror_actions(mu, act_src, act_sign):
    return mu[:, act_src.to(mu.device)] * act_sign.to(device=mu.device, dtype=mu.dtype)


def supervised_gradients_f64(record, make_net, make_cell=None, *, dtype=torch.float64, mean_rows=None, detach_mirrored_original=False, hidden_bias_scale=1.0,
                             bptt=True, aux=None):
    """The gradient of the step's loss at the recorded parameters, by torch autograd.  The loss is SupervisedTrainer.step's, B = record["rows"]:
      cloning term     sum |net(x[:B, :k]) - target|^2 / (12 B)
      symmetric term   record["symmetry"] = (coef, act_src, act_sign): + coef sum |net(x[B:2B, :k]) - M_a net(x[:B, :k])|^2 / (12 B), M_a the action
                       mirror (tests/test_gpu_distill_symmetry._check_one_symmetric_iteration's term on the rows the step read)
      a cell           (h0 / resets in the record, make_cell given): x is [T][N][padded 64] step-major, the cell over the T steps from h0 with a zero
                       state behind a reset, the network on every state (update_grad_ref.recurrent_means, test_gpu_distill_memory._loss_f64)
    k = the in_features of the network (of the cell); the padding columns of x must be zero.  make_net() / make_cell() build the network (a Sequential
    whose state_dict keys are the record's "net." names) and the GRUCell, which are cast to `dtype` and loaded with the recorded parameters.
    dtype = torch.float32: the same loss as torch's own fp32 autograd computes it, the fp32 twin.
    WRONG references, for sensitivity controls:
      mean_rows                  another B in the loss's 1 / (12 B) (the padded row count: a scale error)
      detach_mirrored_original   M_a net(x[:B]) detached in the symmetric term: no gradient through the original half
      hidden_bias_scale          every hidden layer's bias gradient multiplied (2: a column sum finished twice)
      bptt = False               the state detached between steps: no back-propagation through time
    aux: a dict that receives "cloning_loss", "symmetric_loss" (the mean squared asymmetry, without coef; None without the term), "loss" and, with
    symmetry, "cloning_grads" / "symmetric_grads": the gradient of each term alone (the symmetric one with its coef).  Returns {name: gradient} in `dtype`."""
    B, dev, x, target, sym = record["rows"], record["x"].device, record["x"], record["target"], record["symmetry"]
    recurrent = "h0" in record
    assert recurrent == (make_cell is not None) and not (recurrent and sym is not None)
    net = make_net().to(device=dev, dtype=dtype)
    net.load_state_dict({k[len("net."):]: v.to(dtype) for k, v in record["params"].items() if k.startswith("net.")})
    named = [("net." + k, p) for k, p in net.named_parameters()]
    cell = None
    if recurrent:
        cell = make_cell().to(device=dev, dtype=dtype)
        cell.load_state_dict({k[len("memory."):]: v.to(dtype) for k, v in record["params"].items() if k.startswith("memory.")})
        named = [("memory." + k, p) for k, p in cell.named_parameters()] + named
    assert sorted(k for k, _ in named) == sorted(record["params"]), "the record holds other parameters than the networks built"
    named = [(k, dict(named)[k]) for k in record["params"]]  # (the record's order)
    k_in = cell.input_size if recurrent else net[0].in_features
    A = target.shape[1]
    assert target.shape[0] == B and x.shape[0] == (2 * B if sym is not None else B), (tuple(x.shape), tuple(target.shape), B)
    assert not x[:, k_in:].any(), "the padding columns of the network input must be zero"
    x, y = x[:, :k_in].to(dtype), target.to(dtype)
    denom = float(A * (B if mean_rows is None else mean_rows))
    if recurrent:
        h0, resets = record["h0"].to(dtype), record["resets"]
        T, n = resets.shape
        assert T * n == B and tuple(h0.shape) == (n, cell.hidden_size)
        xs, h, mus = x.reshape(T, n, -1), h0, []
        for t in range(T):
            h = cell(xs[t], h * (1 - resets[t].to(dtype)).view(n, 1))
            mus.append(net(h))
            if not bptt:
                h = h.detach()
        mu = torch.cat(mus)
    else:
        mu = net(x[:B])
    cloning = ((mu - y) ** 2).sum() / denom
    terms, symmetric = [cloning], None
    if sym is not None:
        coef, act_src, act_sign = sym
        mirrored = _mirror_actions(mu.detach() if detach_mirrored_original else mu, act_src, act_sign)
        symmetric = ((net(x[B:]) - mirrored) ** 2).sum() / denom
        terms.append(coef * symmetric)
    params = [p for _, p in named]
    if aux is not None:
        aux.update(cloning_loss=cloning.item(), symmetric_loss=None if symmetric is None else symmetric.item(), loss=sum(t.item() for t in terms))
        if sym is not None:
            for key, term in zip(("cloning_grads", "symmetric_grads"), terms):
                gs = torch.autograd.grad(term, params, retain_graph=True, allow_unused=True)
                aux[key] = {k: (torch.zeros_like(p) if g is None else g.detach().clone()) for (k, p), g in zip(named, gs)}
    sum(terms).backward()
    grads = {k: p.grad.detach().clone() for k, p in named}
    if hidden_bias_scale != 1.0:
        last = max(int(k.split(".")[1]) for k in grads if k.startswith("net."))
        for k in grads:
            if k.startswith("net.") and k.endswith(".bias") and int(k.split(".")[1]) != last:
                grads[k] = grads[k] * hidden_bias_scale
    return grads
