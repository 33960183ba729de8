"""Configurable hidden widths on the GPU: the width-generic fused rollout actor (bg_actor_sample_mlp) against a float64 forward and against
bg_actor_sample's noise, the kernel choice at the default widths, whole PPO updates of other architectures against the reference loop on HIP
kernels only, and a train / save / reload / play round trip."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARCHS = [(512, 256, 128), (128, 128), (512, 512, 256, 128)]


def _actor_f64(model, obs):
    h = obs.double()
    lin = [m for m in model.actor if isinstance(m, torch.nn.Linear)]
    for i, l in enumerate(lin):
        h = h @ l.weight.double().t() + l.bias.double()
        if i + 1 < len(lin):
            h = torch.nn.functional.elu(h)
    return h


def _zero_output_layer(model):
    with torch.no_grad():
        model.actor[-1].weight.zero_(); model.actor[-1].bias.zero_()


@pytest.mark.parametrize("hidden", ARCHS)
def test_generic_actor_kernel_matches_float64_and_draws_bg_actor_sample_noise(hidden):
    from booster_gym_amd.utils.model import ActorCritic

    torch.manual_seed(11)
    model = ActorCritic(12, 47, 14, actor_hidden=hidden).to(DEV)
    default = ActorCritic(12, 47, 14).to(DEV)
    with torch.no_grad():
        model.logstd.copy_(torch.linspace(-2.5, 0.5, 12, device=DEV).view(1, 12))
        default.logstd.copy_(model.logstd)
    seed, counter = 1234567, 17
    for n in (100, 4096, 16384):
        obs = torch.randn(n, 47, device=DEV)
        mu_buf, act_buf = torch.full((n + 16, 12), 7.0, device=DEV), torch.full((n + 16, 12), 7.0, device=DEV)
        mu, act = mu_buf[:n], act_buf[:n]
        model.sample_actions(obs, act, seed, counter, mu_out=mu)
        ref = _actor_f64(model, obs)
        err = (mu.double() - ref).abs().max().item()
        assert err <= 2e-5 * max(1.0, ref.abs().max().item()), (hidden, n, err)
        assert torch.all(mu_buf[n:] == 7.0) and torch.all(act_buf[n:] == 7.0), "rows past N were written"
        # the noise: with the output layer zeroed, mu is exactly 0 in both kernels and the actions ARE exp(logstd) * noise
        zm, zd = ActorCritic(12, 47, 14, actor_hidden=hidden).to(DEV), ActorCritic(12, 47, 14).to(DEV)
        zm.load_state_dict(model.state_dict()); zd.load_state_dict(default.state_dict())
        _zero_output_layer(zm); _zero_output_layer(zd)
        a_new, a_old = torch.empty(n, 12, device=DEV), torch.empty(n, 12, device=DEV)
        zm.sample_actions(obs, a_new, seed, counter)
        zd.sample_actions(obs, a_old, seed, counter)
        assert torch.equal(a_new, a_old), "the generic kernel's noise differs from bg_actor_sample's"
        scaled_noise = a_old
        # ... and with the real output layer, actions - mu = exp(logstd) * the same noise (up to the rounding of mu + that product)
        assert torch.allclose(act - mu, scaled_noise, rtol=0, atol=4 * torch.finfo(torch.float32).eps * (1 + mu.abs().max().item())), (hidden, n)
        z = scaled_noise / torch.exp(model.logstd.detach())
        if n >= 4096:
            assert abs(z.mean().item()) < 0.02 and abs(z.std().item() - 1.0) < 0.02
    # argument checks on the host
    from booster_gym_amd import _lib

    lib = _lib.load()
    descs = (_lib.MlpLayerDesc * 3)(_lib.MlpLayerDesc(1, 1, 47, 384), _lib.MlpLayerDesc(16, 16, 384, 128), _lib.MlpLayerDesc(16, 16, 100, 12))
    o = torch.zeros(4, 47, device=DEV)
    assert lib.bg_actor_sample_mlp(4, _lib.ptr(o), 3, descs, _lib.ptr(o), 0, 0, None, _lib.ptr(o), None) == -4 and b"chain" in lib.bg_last_error()
    assert lib.bg_actor_sample_mlp(4, _lib.ptr(o), 2, descs, _lib.ptr(o), 0, 0, None, _lib.ptr(o), None) == -4


def _runner(n, actor_hidden=None, critic_hidden=None, **over):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.runner import Runner

    o = {"env.num_envs": n, "terrain.type": "plane"}
    if actor_hidden is not None:
        o["algorithm.actor_hidden"] = list(actor_hidden)
    if critic_hidden is not None:
        o["algorithm.critic_hidden"] = list(critic_hidden)
    o.update(over)
    return Runner(cfg=load_cfg("T1", o))


def _count_calls(monkeypatch, names):
    from booster_gym_amd import _lib

    lib, counts = _lib.load(), {k: 0 for k in names}
    for name in names:
        fn = getattr(lib, name)

        def wrap(*a, _fn=fn, _name=name):
            counts[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, wrap)
    return counts


@pytest.mark.parametrize("actor_hidden,critic_hidden", [(None, None), ((512, 256, 128), (512, 512, 256, 128))])
def test_rollout_kernel_and_plan_follow_the_widths(monkeypatch, actor_hidden, critic_hidden):
    """Default widths: the rollout still calls bg_actor_sample and resolves today's chained plan; other widths: bg_actor_sample_mlp and the per-layer
    plan."""
    r = _runner(128, actor_hidden, critic_hidden)
    obs, infos = r.env.reset()
    r.buffer["obses"][0].copy_(obs); r.buffer["privileged_obses"][0].copy_(infos["privileged_obs"])
    counts = _count_calls(monkeypatch, ["bg_actor_sample", "bg_actor_sample_mlp"])
    r.rollout()
    torch.cuda.synchronize()
    T = r.cfg["runner"]["horizon_length"]
    plan = r._resolve_plan()
    if actor_hidden is None:
        assert counts == {"bg_actor_sample": T, "bg_actor_sample_mlp": 0}
        assert plan.critic.fwd == plan.actor.fwd == "chain_split" and plan.critic.bwd == plan.actor.bwd == "chain_split"
        assert plan.chain_values and plan.one_stream and plan.one_tail and plan.ahead and plan.wgrad == 9
    else:
        assert counts == {"bg_actor_sample": 0, "bg_actor_sample_mlp": T}
        assert plan.critic.fwd == plan.actor.fwd == "layer" and plan.critic.bwd == plan.actor.bwd == "layer"
        assert not plan.chain_values and not plan.ahead and plan.fused_head and plan.wgrad == 0
        assert all(plan.critic.grouped[:-1]) and all(plan.actor.grouped[:-1])
    assert torch.isfinite(r.buffer["actions"]).all()


def _assert_same_adam_steps(name, p, q, start):
    """As in test_gpu_ppo: all but 0.5 % of the elements within 2 % of the distance the tensor's parameters moved, none further than twice that."""
    moved = (q - start).abs().max().item()
    d = (p - q).abs()
    off = (d > 0.02 * moved + 2e-6).float().mean().item()
    assert off <= 0.005 and d.max().item() <= 2.0 * moved + 2e-6, (name, off, d.max().item(), moved)


def _raise(*a, **k):
    raise AssertionError("library GEMM in the update")


@pytest.mark.parametrize("actor_hidden,critic_hidden", [((512, 256, 128), (512, 256, 128)), ((512, 512, 256, 128), (512, 512, 256, 128))])
def test_update_of_other_widths_matches_reference_loop_without_library_gemms(monkeypatch, actor_hidden, critic_hidden):
    """Runner.rollout() + update() (256 envs, 3 mini-epochs) against oracle/ppo_ref.ppo_update_reference on a copy of the model, as
    test_gpu_ppo.test_full_update_matches_reference_loop: parameters, logged losses, learning rate.  torch.mm / addmm / matmul / F.linear raise
    during update(): every GEMM of the update runs on the HIP kernels."""
    from booster_gym_amd.utils.model import ActorCritic
    from oracle.ppo_ref import ppo_update_reference

    E, T = 3, 24
    r = _runner(256, actor_hidden, critic_hidden, **{"runner.mini_epochs": E})
    obs, infos = r.env.reset()
    r.buffer["obses"][0].copy_(obs); r.buffer["privileged_obses"][0].copy_(infos["privileged_obs"])
    r.rollout()
    ref_model = ActorCritic(12, 47, 14, actor_hidden, critic_hidden).to(DEV)
    ref_model.load_state_dict(r.model.state_dict())
    b = r.buffer
    rewards_ref = b["rewards"].clone()
    stats_ref, lr_ref = ppo_update_reference(ref_model, torch.optim.Adam(ref_model.parameters(), lr=1e-5), b["obses"][:T].clone(), b["privileged_obses"][:T].clone(),
                                             b["actions"].clone(), rewards_ref, b["dones"].clone(), b["time_outs"].clone(), b["obses"][T].clone(),
                                             b["privileged_obses"][T].clone(), mini_epochs=E, learning_rate=1e-5)
    p_start = {k: p.detach().clone() for k, p in r.model.named_parameters()}
    with monkeypatch.context() as m:
        for mod, name in ((torch, "mm"), (torch, "addmm"), (torch, "matmul"), (torch, "bmm"), (torch.nn.functional, "linear")):
            m.setattr(mod, name, _raise)
        acc = r.update()
        torch.cuda.synchronize()
    summ = r._summarize(acc)
    for (k, p), (k2, q) in zip(r.model.named_parameters(), ref_model.named_parameters()):
        assert k == k2
        _assert_same_adam_steps(k, p, q, p_start[k])
        assert torch.allclose(p, q, rtol=1e-3, atol=2e-6), (k, (p - q).abs().max().item())
    assert torch.allclose(b["rewards"], rewards_ref, atol=1e-5)
    for k in ("value_loss", "actor_loss", "bound_loss", "entropy", "kl_mean"):
        assert abs(summ[k] - stats_ref[k]) <= 2e-4 * max(1.0, abs(stats_ref[k])), (k, summ[k], stats_ref[k])
    assert abs(summ["lr"] - lr_ref) < 1e-9
    # the optimiser launch kept every weight copy the layer kernels read current (zero-padded first layers, transposed hidden layers)
    trs = (r._critic_tr, r._actor_tr)
    ms = [m for tr in trs for m in tr.copies.descriptors(r.optimizer.flat, tr.plan)]
    current = [tr.copies.current(*key) for tr in trs for key in tr.copies.listed]
    assert len(ms) == len(actor_hidden) + len(critic_hidden) <= 16 and len(current) == len(ms) and all(current)


def test_train_save_reload_play_and_checkpoint_width_mismatch(tmp_path):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.recorder import Recorder
    from booster_gym_amd.utils.runner import Runner

    over = {"env.num_envs": 128, "terrain.type": "plane", "runner.mini_epochs": 2, "algorithm.actor_hidden": [512, 256, 128]}
    cfg = load_cfg("T1", over)
    r = Runner(cfg=cfg)
    r.begin_training(Recorder(cfg, root=str(tmp_path / "logs"), rank=0))
    for it in range(2):
        r.train_iteration(it)
    r._flush_log()
    torch.cuda.synchronize()
    assert torch.isfinite(r.optimizer.flat).all()
    ck = str(tmp_path / "model_2.pth")
    torch.save(r.checkpoint_dict(), ck)
    sd = {k: v.clone() for k, v in r.model.state_dict().items()}
    del r
    p = Runner(test=True, cfg=load_cfg("T1", dict(over, **{"basic.checkpoint": ck})))
    for k, v in p.model.state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert p.play(max_steps=10) == 10
    del p
    with pytest.raises(ValueError) as e:
        Runner(test=True, cfg=load_cfg("T1", {"env.num_envs": 128, "terrain.type": "plane", "basic.checkpoint": ck}))
    msg = str(e.value)
    assert "[512, 256, 128]" in msg and "[256, 128, 128]" in msg and "[256, 256, 128]" in msg and "algorithm.actor_hidden" in msg
