"""Timing of the gait record (README "Evaluation", evaluation.gait); writes profiles/gait_time.txt.

  python tools/gait_time.py [reps=300] [pairs=3] [num_envs=4096] [loop_steps=300] [out=profiles/gait_time.txt] [parent=DIR]
      (1) the launch: on a plane and on the height field, in one process each terrain: HIP events around `reps` back-to-back bg_env_gait_step launches
          on a running record (no robot finished: the done flags are cleared), around `reps` bg_env_eval_step launches and around reps / 3 env steps,
          the sides alternating, `pairs` times: us per launch, the bytes a gait launch moves (from the code) and its share of the float4-copy rate;
      (2) the evaluation loop on the packaged reference actor (tests/golden/t1_actor.npz), plane, `loop_steps` steps, evaluation.gait on against off,
          one Evaluator after the other, the sides alternating, `pairs` times: env-steps/s;
      with parent=DIR, a built checkout of the parent commit:
      (3) bench.py --gpus 1 --steps 20 --warmup 5 of this tree and of the parent in alternating processes, `pairs` pairs: env-steps/s;
      (4) the SHA-256 over parameters and Adam moments after two default iterations, this tree against the parent, each in a process of its own.
  python tools/gait_time.py digest ROOT     prints (4)'s SHA for the tree at ROOT (the mode (4) starts)."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "digest" else ROOT)
import numpy as np
import torch

COPY_TBS = 6.29  # a float4 copy on this part, TB/s (README "Mini-batches")
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def _orders(p, keys):
    return keys if p % 2 == 0 else tuple(reversed(keys))


def _events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def gait_launch_bytes(n, fp16=False):
    """What one bg_gait_step launch moves with every robot running, from the kernel: 60 record planes read and 59 written (STATE is not), 45 field
    planes read (12 actions, 12 torques, 2 + 2 + 3, 2 contact flags, 2 vertical forces, 6 foot coordinates; with the fp16 slab the 12 actions and
    3 commands are 2 bytes), the done flag; on a height field 2 x 4 int16 on top (not counted: they hit a few cache lines per wave)."""
    half = 15 if fp16 else 0
    return n * (4 * (60 + 59) + 4 * (45 - half) + 2 * half + 1)


def launch(reps, pairs, N):
    from booster_gym_amd.envs import T1
    from booster_gym_amd.utils.config import load_cfg

    for terrain in ("plane", "trimesh"):
        env = T1(load_cfg("T1", {"env.num_envs": N, "terrain.type": terrain}))
        g = torch.Generator(device="cpu").manual_seed(0)
        act = (torch.rand(N, 12, generator=g) * 0.2 - 0.1).to(env.device)
        env.reset()
        for _ in range(20):
            env.step(act)
        env.reset_buf.zero_()  # nobody finishes: every launch below does the whole rule for every robot
        gait, rec = env.gait_begin(), env.eval_begin()
        sides = (("gait", lambda: env.gait_step(gait, 5), reps), ("eval", lambda: env.eval_step(rec, 5), reps), ("env", lambda: env.step(act), max(reps // 3, 1)))
        for name, fn, r in sides:
            _events(fn, 10)
        env.reset_buf.zero_()
        gait, rec = env.gait_begin(), env.eval_begin()
        b = gait_launch_bytes(N)
        for q in range(pairs):
            us = {}
            for name, fn, r in _orders(q, sides):
                if name != "env":
                    env.reset_buf.zero_()
                us[name] = _events(fn, r)
            torch.cuda.synchronize()
            running = int((gait[0] == 0).sum())
            say(f"{terrain}, {N} envs: bg_env_gait_step {us['gait']:.2f} us, bg_env_eval_step {us['eval']:.2f} us, env step {us['env']:.1f} us per call "
                f"(host-enqueued, back to back); a gait launch moves {b / 1e6:.2f} MB = {b / us['gait'] * 1e-6:.3f} TB/s = "
                f"{b / us['gait'] * 1e-6 / COPY_TBS * 100:.1f} % of the {COPY_TBS} TB/s float4-copy rate ({b / COPY_TBS * 1e-6:.2f} us at that rate); "
                f"gait / eval = {us['gait'] / us['eval']:.2f}, gait / env step = {us['gait'] / us['env']:.4f}; records still running {running} of {N}")
        del env


def loop(pairs, N, steps):
    from booster_gym_amd.utils.evaluate import Evaluator

    with np.load(os.path.join(ROOT, "tests", "golden", "t1_actor.npz")) as W:
        actor = {k: W[k] for k in W.files}
    for q in range(pairs):
        res = {}
        for on in _orders(q, (False, True)):
            ev = Evaluator(actor=actor, overrides={"env.num_envs": N, "terrain.type": "plane", "evaluation.gait": on})
            ev.run(steps)
            res[on] = N * steps / ev.loop_s
            del ev
        say(f"evaluation loop, reference actor, plane, {N} envs, {steps} steps: key off {res[False]:,.0f} env-steps/s, key on {res[True]:,.0f} env-steps/s, "
            f"on / off = {res[True] / res[False]:.4f}")


class _Rec:
    def record_episode_statistics(self, env, names, it, stats=None):
        pass

    def record_statistics(self, summary, it):
        pass

    def save(self, d, it):
        pass


def digest(N=4096):
    """SHA-256 over parameters and Adam moments after two iterations of the default config (of whichever tree is first on sys.path)."""
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.runner import Runner

    cfg = load_cfg("T1", {"env.num_envs": N})
    cfg["runner"]["save_interval"] = 10 ** 9
    r = Runner(cfg=cfg)
    r.begin_training(recorder=_Rec())
    for it in range(2):
        r.train_iteration(it)
    r._flush_log()
    torch.cuda.synchronize()
    o, h = r.optimizer, hashlib.sha256()
    for t in list(r.model.state_dict().values()) + [o.flat, o.exp_avg, o.exp_avg_sq]:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def against_parent(parent, pairs, N):
    trees = (("this tree", ROOT), ("parent", os.path.abspath(parent)))
    vals = {name: [] for name, _ in trees}
    for q in range(pairs):
        val = {}
        for name, root in _orders(q, trees):
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=root, check=True, capture_output=True, text=True, timeout=180).stdout
            val[name] = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])["value"]
            vals[name].append(val[name])
        say(f"bench.py --gpus 1 --steps 20 --warmup 5, pair {q}: this tree {val['this tree']:.0f} env-steps/s, parent {val['parent']:.0f} env-steps/s, "
            f"this / parent = {val['this tree'] / val['parent']:.4f}")
    p, t = vals["parent"], vals["this tree"]
    say(f"the parent's own spread across its {pairs} runs: {(max(p) - min(p)) / np.mean(p) * 100:.2f} % of its mean; this tree's mean / the parent's mean = "
        f"{np.mean(t) / np.mean(p):.4f}")
    sha = {name: subprocess.run([sys.executable, os.path.abspath(__file__), "digest", root], cwd=root, check=True, capture_output=True, text=True, timeout=180).stdout.split()[-1]
           for name, root in trees}
    say(f"sha256 over parameters and Adam moments after two default iterations at {N} envs: this tree {sha['this tree']}, parent {sha['parent']}: "
        + ("equal" if sha["this tree"] == sha["parent"] else "DIFFERENT"))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "digest":
        print(digest())
        sys.exit(0)
    pos = [x for x in sys.argv[1:] if "=" not in x]
    named = dict(x.split("=", 1) for x in sys.argv[1:] if "=" in x)
    reps, pairs, N, steps = (int(pos[i]) if len(pos) > i else d for i, d in enumerate((300, 3, 4096, 300)))
    out = named.get("out", os.path.join(ROOT, "profiles", "gait_time.txt"))
    say(f"# tools/gait_time.py {reps} {pairs} {N} {steps} on {torch.cuda.get_device_name(0)}")
    launch(reps, pairs, N)
    loop(pairs, N, steps)
    if named.get("parent"):
        against_parent(named["parent"], pairs, N)
    else:
        say("bench.py against the parent commit and the SHA-256 against the parent: not measured in this run (no parent=DIR given)")
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("written " + out)
