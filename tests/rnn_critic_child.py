"""Child process of tests/test_gpu_rnn_critic.py: one PPO iteration with algorithm.rnn_critic at N = 64, T = 8, runner.num_env_mini_batches = 2 under
the BG_GRU_GROUP of its environment; prints how often each of the recurrences' entry points ran and the SHA-256 over parameters and Adam's moments."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import torch

    from booster_gym_amd import _lib
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.runner import Runner
    from test_gpu_distill import _Rec

    names = ("bg_gru_sequence_forward", "bg_gru_sequence_backward", "bg_gru_sequence_forward_group", "bg_gru_sequence_backward_group")
    lib, counts = _lib.load(), {k: 0 for k in names}
    for name in names:
        def wrap(*a, _fn=getattr(lib, name), _name=name):
            counts[_name] += 1
            return _fn(*a)
        setattr(lib, name, wrap)
    dev = "cuda:0"
    cfg = load_cfg("T1", {"env.num_envs": 64, "terrain.type": "plane", "basic.sim_device": dev, "basic.rl_device": dev, "runner.horizon_length": 8,
                          "runner.mini_epochs": 2, "algorithm.rnn_hidden_size": 128, "algorithm.rnn_critic": True, "runner.num_env_mini_batches": 2,
                          "rewards.episode_length_s": 0.13})
    r = Runner(cfg=cfg)
    r.begin_training(recorder=_Rec())
    for it in range(2):
        r.train_iteration(it)
    r._flush_log()
    torch.cuda.synchronize()
    o, h = r.optimizer, hashlib.sha256()
    for t in list(r.model.state_dict().values()) + [o.flat, o.exp_avg, o.exp_avg_sq, o.lr, r._cmem_tr.next_state]:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    assert bool(torch.isfinite(o.flat).all())
    print("counts", " ".join(str(counts[k]) for k in names))
    print("sha256", h.hexdigest())


if __name__ == "__main__":
    main()
