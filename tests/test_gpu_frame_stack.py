"""The actor's observation history on the GPU (env.frame_stack): bg_obs_stack against a stack built on the host from the frame_stack: 1 env's outputs
(bitwise: the kernel only copies), a ragged env count through step_to, the rollout actor's wide first layer (bg_actor_sample_mlp) against a float64
forward, and the Runner's update, checkpoint, export and symmetry loss with a 141-input actor.  The default path stays today's."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = 187
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ov(n, H=1, **over):
    ov = {"env.num_envs": n, "basic.sim_device": DEV, "basic.rl_device": DEV}
    if H != 1:
        ov.update({"env.frame_stack": H, "env.num_observations": 47 * H})
    ov.update(over)
    return ov


def _env(n, H=1, **over):
    from booster_gym_amd.envs import T1
    from booster_gym_amd.utils.config import load_cfg

    return T1(load_cfg("T1", _ov(n, H, **over)))


def _actions(n, k, amp=0.6):
    g = torch.Generator(device="cpu").manual_seed(1000 + k)
    return ((torch.rand(n, 12, generator=g) * 2 - 1) * amp).to(DEV)


class HostStack:
    """humanoid-gym's rule restated: the row is the last H single observations, oldest first, newest last; an env that was reset has H - 1 zero frames
    and its new observation."""

    def __init__(self, n, H):
        self.hist = torch.zeros(n, H, 47, device=DEV)

    def push(self, obs, done=None):
        self.hist = torch.cat([self.hist[:, 1:], obs.reshape(-1, 1, 47)], dim=1)
        if done is None:  # reset-all
            self.hist[:, :-1] = 0.0
        else:
            self.hist[done.bool(), :-1] = 0.0
        return self.hist.reshape(self.hist.shape[0], -1).clone()


CASES = [(2, {}), (5, {"sim.state_dtype": "fp16"}), (10, {"parallel.exact_still_count": True}),
         (5, {"terrain.curriculum": True, "terrain.measure_heights": True, "env.num_privileged_obs": 14 + P})]


@pytest.mark.parametrize("H,over", CASES)
def test_history_is_exact(H, over):
    n = 192
    e1, eh = _env(n, 1, **over), _env(n, H, **over)
    assert (eh.num_single_obs, eh.frame_stack, eh.num_obs) == (47, H, 47 * H) and tuple(eh.obs_buf.shape) == (n, 47 * H)
    assert (e1.num_single_obs, e1.frame_stack, e1.num_obs) == (47, 1, 47) and tuple(e1.obs_buf.shape) == (n, 47)
    host = HostStack(n, H)
    for rep in range(2):  # (the second reset-all forgets the frame of the first)
        o1, x1 = e1.reset()
        oh, xh = eh.reset()
        torch.cuda.synchronize()
        assert torch.equal(oh, host.push(o1)) and torch.equal(oh[:, -47:], o1) and not oh[:, :-47].any()
        assert torch.equal(x1["privileged_obs"], xh["privileged_obs"])
    resets = 0
    for k in range(100):
        if k == 40:  # some robots lying on their side: reset at the end of this step, in both envs alike
            for e in (e1, eh):
                root = e.root_states.cpu().numpy().copy()
                root[:32, 2] -= 0.4
                root[:32, 3:7] = [np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5)]
                e.set_field("root_states", torch.from_numpy(root).float())
        a = _actions(n, k)
        o1, r1, d1, x1 = e1.step(a)
        oh, rh, dh, xh = eh.step(a)
        torch.cuda.synchronize()
        assert torch.equal(r1, rh) and torch.equal(d1, dh), k
        assert torch.equal(x1["time_outs"], xh["time_outs"]) and torch.equal(x1["privileged_obs"], xh["privileged_obs"]), k
        assert torch.equal(oh[:, -47:], o1), k
        assert torch.equal(oh, host.push(o1, d1)), k
        resets += int(d1.sum())
    assert resets >= 32, resets
    assert oh[:, :47].abs().sum() > 0  # (the oldest frame is in use by now)


@pytest.mark.parametrize("H", [3, 10])
def test_ragged_env_count_and_step_to_write_every_row_and_nothing_past_n(H):
    n = 1000
    e1, eh = _env(n, 1), _env(n, H)
    host = HostStack(n, H)
    o1, _ = e1.reset()
    oh, _ = eh.reset()
    assert torch.equal(oh, host.push(o1))
    rew, done, tout = torch.empty(n, device=DEV), torch.empty(n, dtype=torch.bool, device=DEV), torch.empty(n, dtype=torch.bool, device=DEV)
    priv = torch.empty(n, 14, device=DEV)
    for k in range(3):
        a = _actions(n, k, 0.3)
        o1, _, d1, _ = e1.step(a)
        big = torch.full((n + 7, 47 * H), float("nan"), device=DEV)  # a different destination at every step, as the rows of a rollout buffer
        eh.step_to(a, big[:n], priv, rew, done, tout)
        torch.cuda.synchronize()
        assert torch.isfinite(big[:n]).all() and torch.isnan(big[n:]).all(), k
        assert torch.equal(done, d1) and torch.equal(big[:n], host.push(o1, d1)), k
    with pytest.raises(RuntimeError, match="obs of 1000 x"):
        eh.step_to(a, torch.empty(n, 47, device=DEV), priv, rew, done, tout)


# ------------------------------------------------------------------ the rollout actor
def _actor_f64(model, obs):
    x = obs.double()
    lin = [m for m in model.actor if isinstance(m, torch.nn.Linear)]
    for i, l in enumerate(lin):
        x = x @ l.weight.double().t() + l.bias.double()
        if i + 1 < len(lin):
            x = torch.where(x > 0, x, torch.expm1(x))
    return x


def _zero_output_layer(model):
    with torch.no_grad():
        model.actor[-1].weight.zero_(); model.actor[-1].bias.zero_()


@pytest.mark.parametrize("hidden", [(256, 128, 128), (512, 256, 128)])
@pytest.mark.parametrize("H", [2, 4, 5, 10])
def test_rollout_actor_of_a_stack_matches_float64_and_draws_bg_actor_sample_noise(monkeypatch, H, hidden):
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.model import ActorCritic

    torch.manual_seed(11 + H)
    K = 47 * H
    model = ActorCritic(12, K, 14, actor_hidden=hidden).to(DEV)
    default = ActorCritic(12, 47, 14).to(DEV)
    with torch.no_grad():
        model.logstd.copy_(torch.linspace(-2.5, 0.5, 12, device=DEV).view(1, 12))
        default.logstd.copy_(model.logstd)
    lib, calls = _lib.load(), []
    fn = lib.bg_actor_sample_mlp
    monkeypatch.setattr(lib, "bg_actor_sample_mlp", lambda *a: (calls.append(1), fn(*a))[1])
    seed, counter = 1234567, 17
    for n in (100, 4096, 16384):
        obs = torch.randn(n, K, device=DEV)
        mu_buf, act_buf = torch.full((n + 16, 12), 7.0, device=DEV), torch.full((n + 16, 12), 7.0, device=DEV)
        mu, act = mu_buf[:n], act_buf[:n]
        calls.clear()
        model.sample_actions(obs, act, seed, counter, mu_out=mu)
        assert len(calls) == 1  # (the reference's widths, too, run the width-generic kernel on a stack)
        ref = _actor_f64(model, obs)
        err = (mu.double() - ref).abs().max().item()
        print(f"H {H} hidden {hidden} n {n}: max error {err:.3e}, |ref|max {ref.abs().max().item():.3f}")
        assert err <= 2e-5 * max(1.0, ref.abs().max().item()), (H, hidden, n, err)
        assert torch.all(mu_buf[n:] == 7.0) and torch.all(act_buf[n:] == 7.0), "rows past N were written"
        # the noise: with the output layer zeroed, mu is exactly 0 in both kernels and the actions ARE exp(logstd) * noise
        zm, zd = ActorCritic(12, K, 14, actor_hidden=hidden).to(DEV), ActorCritic(12, 47, 14).to(DEV)
        zm.load_state_dict(model.state_dict()); zd.load_state_dict(default.state_dict())
        _zero_output_layer(zm); _zero_output_layer(zd)
        a_new, a_old = torch.empty(n, 12, device=DEV), torch.empty(n, 12, device=DEV)
        zm.sample_actions(obs, a_new, seed, counter)
        zd.sample_actions(obs[:, :47].contiguous(), a_old, seed, counter)
        assert torch.equal(a_new, a_old), "the generic kernel's noise differs from bg_actor_sample's"
        assert torch.allclose(act - mu, a_old, rtol=0, atol=4 * torch.finfo(torch.float32).eps * (1 + mu.abs().max().item())), (H, hidden, n)
    # the existing argument errors stay; a first layer that is not 47 H wide, or wider than 470, is one of them
    o = torch.zeros(4, 47 * 11, device=DEV)
    for k_in in (48, 100, 47 * 11):
        descs = (_lib.MlpLayerDesc * 3)(_lib.MlpLayerDesc(16, 16, k_in, 128), _lib.MlpLayerDesc(16, 16, 128, 128), _lib.MlpLayerDesc(16, 16, 128, 12))
        assert fn(4, _lib.ptr(o), 3, descs, _lib.ptr(o), 0, 0, None, _lib.ptr(o), None) == -4 and b"chain" in lib.bg_last_error(), k_in
    with pytest.raises(ValueError, match="observations of 47 columns"):
        model.sample_actions(torch.zeros(4, 47, device=DEV), torch.zeros(4, 12, device=DEV), 0, 0)


def _runner(n, H=3, **over):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.runner import Runner

    ov = _ov(n, H, **{"terrain.type": "plane"})
    ov.update(over)
    return Runner(cfg=load_cfg("T1", ov))


def _start(r):
    obs, infos = r.env.reset()
    r.buffer["obses"][0].copy_(obs); r.buffer["privileged_obses"][0].copy_(infos["privileged_obs"])


def test_weights_loaded_from_outside_reach_the_rollout_actor():
    """load_state_dict + Runner.invalidate() after a rollout and an update (every weight copy the update's kernels keep exists by then): the next
    sample's means are the new weights'."""
    from booster_gym_amd.utils.model import ActorCritic

    r = _runner(128, 3, **{"runner.mini_epochs": 2})
    _start(r)
    r.iteration()
    torch.manual_seed(5)
    other = ActorCritic(12, 141, 14).to(DEV)
    obs = torch.randn(128, 141, device=DEV)
    mu, act = torch.empty(128, 12, device=DEV), torch.empty(128, 12, device=DEV)
    r.model.sample_actions(obs, act, 1, 2, mu_out=mu)
    before = _actor_f64(r.model, obs)
    assert (mu.double() - before).abs().max().item() <= 2e-5 * max(1.0, before.abs().max().item())
    r.model.load_state_dict(other.state_dict())
    r.invalidate()
    r.model.sample_actions(obs, act, 1, 2, mu_out=mu)
    ref = _actor_f64(other, obs)
    assert (ref - before).abs().max().item() > 1e-2  # (the two sets of weights do differ)
    assert (mu.double() - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())
    _start(r)
    r.iteration()  # ... and the update's kernels pick them up as well
    torch.cuda.synchronize()
    assert torch.isfinite(r.optimizer.flat).all()


# ------------------------------------------------------------------ the update
def _assert_same_adam_steps(name, p, q, start):
    """As in test_gpu_ppo: all but 0.5 % of the elements within 2 % of the distance the tensor's parameters moved, none further than twice that."""
    moved = (q - start).abs().max().item()
    d = (p - q).abs()
    off = (d > 0.02 * moved + 2e-6).float().mean().item()
    assert off <= 0.005 and d.max().item() <= 2.0 * moved + 2e-6, (name, off, d.max().item(), moved)


def _raise(*a, **k):
    raise AssertionError("library GEMM in the update")


def test_update_with_a_stack_matches_reference_loop_without_library_gemms(monkeypatch):
    """Runner.rollout() + update() (256 envs, 3 mini-epochs, H = 3) against oracle/ppo_ref.ppo_update_reference on a copy of the model, with the
    tolerances of test_gpu_network_widths.test_update_of_other_widths_matches_reference_loop_without_library_gemms."""
    from booster_gym_amd.utils.model import ActorCritic
    from oracle.ppo_ref import ppo_update_reference

    E, T = 3, 24
    r = _runner(256, 3, **{"runner.mini_epochs": E})
    assert r.model.actor[0].in_features == 141 and r.model.critic[0].in_features == 155
    assert r._actor_in.shape[-1] == 256 and r._critic_in.shape[-1] == 256
    _start(r)
    r.rollout()
    plan = r._resolve_plan()
    assert plan.actor.fwd == "layer" and plan.actor.bwd == "layer" and plan.critic.fwd == "layer" and not plan.ahead and plan.fused_head
    assert all(plan.actor.grouped[:-1]) and all(plan.critic.grouped[:-1])
    ref_model = ActorCritic(12, 141, 14).to(DEV)
    ref_model.load_state_dict(r.model.state_dict())
    b = r.buffer
    assert tuple(b["obses"].shape) == (T + 1, 256, 141)
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
        print(f"{k}: max |p - q| {(p - q).abs().max().item():.3e}, moved {(q - p_start[k]).abs().max().item():.3e}")
        _assert_same_adam_steps(k, p, q, p_start[k])
        assert torch.allclose(p, q, rtol=1e-3, atol=2e-6), (k, (p - q).abs().max().item())
    assert torch.allclose(b["rewards"], rewards_ref, atol=1e-5)
    for k in ("value_loss", "actor_loss", "bound_loss", "entropy", "kl_mean"):
        print(f"{k}: {summ[k]!r} against {stats_ref[k]!r}")
        assert abs(summ[k] - stats_ref[k]) <= 2e-4 * max(1.0, abs(stats_ref[k])), (k, summ[k], stats_ref[k])
    assert abs(summ["lr"] - lr_ref) < 1e-9


# ------------------------------------------------------------------ checkpoint, play, export, symmetry loss
class _Rec:
    def __init__(self):
        self.stats = {}

    def record_episode_statistics(self, env, names, it, stats=None):
        pass

    def record_statistics(self, summary, it):
        self.stats[it] = dict(summary)

    def save(self, d, it):
        return None


def _train(r, iters):
    rec = _Rec()
    r.begin_training(recorder=rec)
    for it in range(iters):
        r.train_iteration(it)
    r._flush_log()
    torch.cuda.synchronize()
    return rec


def test_train_save_reload_play_export_and_checkpoint_width_mismatch(tmp_path):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.model import ActorCritic
    from booster_gym_amd.utils.runner import Runner

    r = _runner(128, 3, **{"runner.mini_epochs": 2})
    rec = _train(r, 2)
    assert len(rec.stats) == 2 and all(np.isfinite(float(v)) for s in rec.stats.values() for v in s.values())
    assert torch.isfinite(r.optimizer.flat).all()
    ck = str(tmp_path / "model_2.pth")
    torch.save(r.checkpoint_dict(), ck)
    sd = {k: v.clone() for k, v in r.model.state_dict().items()}
    del r
    p = Runner(test=True, cfg=load_cfg("T1", _ov(128, 3, **{"terrain.type": "plane", "basic.checkpoint": ck})))
    for k, v in p.model.state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert p.play(max_steps=10) == 10
    del p
    with pytest.raises(ValueError, match=r"141 inputs.*takes 47.*env\.frame_stack"):
        _runner(128, 1, **{"basic.checkpoint": ck})
    r1 = _runner(128, 1)
    ck1 = str(tmp_path / "model_h1.pth")
    torch.save(r1.checkpoint_dict(), ck1)
    del r1
    with pytest.raises(ValueError, match=r"47 inputs.*takes 141.*env\.frame_stack"):
        _runner(128, 3, **{"basic.checkpoint": ck1})

    # export_model.py, from the default config: the actor's input width comes from the checkpoint
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    subprocess.run([sys.executable, os.path.join(ROOT, "export_model.py"), "--task=T1", f"--checkpoint={ck}"], cwd=str(tmp_path), env=env, check=True,
                   timeout=300)
    actor = torch.jit.load(str(tmp_path / "deploy" / "models" / "T1.pt"), map_location="cpu")
    assert tuple(actor(torch.zeros(3, 141)).shape) == (3, 12)
    m = ActorCritic(12, 141, 14)
    m.load_state_dict({k: v.cpu() for k, v in sd.items()})
    x = torch.linspace(-1, 1, 3 * 141).reshape(3, 141)
    assert torch.allclose(actor(x), m.actor(x), atol=1e-6)


def test_symmetry_loss_with_a_stack():
    r = _runner(256, 3, **{"algorithm.symmetry_loss": True, "runner.mini_epochs": 2})
    assert len(r._obs_mirror[0]) == 256 and r._obs_mirror[0][47:94] == [47 + s for s in r._obs_mirror[0][:47]]
    # bg_mirror_rows on the 256 padded columns: frame k of the mirrored row is the single observation's map of frame k, the padding stays zero
    from booster_gym_amd.utils.utils import mirror_rows

    x = torch.randn(300, 256, device=DEV)
    y = torch.full_like(x, float("nan"))
    mirror_rows(x, y, *r._obs_mirror)
    src1, sign1 = torch.tensor(r._obs_mirror[0][:47], device=DEV), torch.tensor(r._obs_mirror[1][:47], device=DEV)
    for k in range(3):
        assert torch.equal(y[:, 47 * k : 47 * (k + 1)], sign1 * x[:, 47 * k : 47 * (k + 1)][:, src1]), k
    assert not y[:, 141:].any()
    rec = _train(r, 1)
    s = rec.stats[0]
    assert "symmetry_loss" in s and all(np.isfinite(float(v)) for v in s.values())


def test_gemm_split_with_a_wide_stack_is_a_value_error():
    with pytest.raises(ValueError, match=r"gemm_split.*actor's input of 282.*env\.frame_stack"):
        _runner(128, 6, **{"parallel.gemm_split": 9})


# ------------------------------------------------------------------ the default path
def test_default_path_keeps_its_kernels_and_plan(monkeypatch):
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.runner import Runner

    cfg = load_cfg("T1", {"env.num_envs": 128, "terrain.type": "plane"})
    del cfg["env"]["frame_stack"]  # the key absent, as in a yaml written before it existed
    r = Runner(cfg=cfg)
    assert r.env.frame_stack == 1 and tuple(r.env.obs_buf.shape) == (128, 47) and r.env._cfg_c.frame_stack == 1
    _start(r)
    lib, counts = _lib.load(), {"bg_actor_sample": 0, "bg_actor_sample_mlp": 0}
    for name in counts:
        def wrap(*a, _fn=getattr(lib, name), _name=name):
            counts[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, wrap)
    r.rollout()
    torch.cuda.synchronize()
    T = r.cfg["runner"]["horizon_length"]
    plan = r._resolve_plan()
    assert counts == {"bg_actor_sample": T, "bg_actor_sample_mlp": 0}
    assert plan.critic.fwd == plan.actor.fwd == "chain_split" and plan.critic.bwd == plan.actor.bwd == "chain_split"
    assert plan.chain_values and plan.one_stream and plan.one_tail and plan.ahead and plan.wgrad == 9
    assert torch.isfinite(r.buffer["actions"]).all()
