"""runner.num_mini_batches under data parallelism: two ranks (gloo backend, both on the one GPU of the test box) of 64 envs each, E = 2 mini-epochs of
K = 2 steps.  Both ranks must end with identical parameters, and they must match the torch restatement of the reference loop with the K-step inner
loop (tests/test_gpu_mini_batches.py) on the UNION of the rollouts, whose mini-batch k is the concatenation of the ranks' mini-batches k."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def _worker(rank, world, port, q):
    try:
        _worker_body(rank, world, port, q)
    except BaseException as ex:  # the parent fails fast with the real error instead of a queue time-out
        import traceback

        q.put(("error", rank, "".join(traceback.format_exception(type(ex), ex, ex.__traceback__))))
        raise


def _worker_body(rank, world, port, q):
    os.environ.update(WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      BG_DIST_BACKEND="gloo", BG_LOCAL_DEVICE="0")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import torch.distributed as dist

    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.model import ActorCritic
    from booster_gym_amd.utils.runner import Runner
    from test_gpu_mini_batches import compare_with_reference, device_batches, reference_update_with_mini_batches

    E, K, n = 2, 2, 64
    cfg = load_cfg("T1", {"env.num_envs": n, "terrain.type": "plane", "runner.mini_epochs": E, "runner.num_mini_batches": K})
    r = Runner(cfg=cfg)
    assert r.world_size == 2 and r.rank == rank and r._mini_batches == K
    obs, infos = r.env.reset()
    r.buffer["obses"][0].copy_(obs); r.buffer["privileged_obses"][0].copy_(infos["privileged_obs"])
    r.rollout()
    T = cfg["runner"]["horizon_length"]
    sd0 = {k: v.detach().clone() for k, v in r.model.state_dict().items()}
    b = r.buffer

    def gather(t, dim):
        parts = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(parts, t.contiguous())
        return torch.cat(parts, dim=dim)

    full = {k: gather(b[k].to(torch.uint8) if b[k].dtype == torch.bool else b[k], 1) for k in ("obses", "privileged_obses", "actions", "rewards", "dones", "time_outs")}
    # the ranks shuffle independently: row i = t n + e of rank r is row t (world n) + r n + e of the union; step k of the union = the ranks' steps k
    own = device_batches(r, E, K)
    to_union = lambda idx, rk: (idx // n) * (world * n) + rk * n + idx % n
    batches = []
    for e in range(E):
        steps = []
        for k in range(K):
            every = gather(own[e][k].view(1, -1), 0)  # [world][b]
            steps.append(torch.cat([to_union(every[rk], rk) for rk in range(world)]))
        batches.append(steps)
    assert not torch.equal(gather(own[0][0].view(1, -1), 0)[0], gather(own[0][0].view(1, -1), 0)[1])  # (the rank keys the permutation)
    p_start = {k: p.detach().clone() for k, p in r.model.named_parameters()}
    acc = r.update()
    flat = torch.cat([p.detach().reshape(-1) for p in r.model.parameters()])
    other = gather(flat.view(1, -1), 0)
    ref_model = ActorCritic(12, 47, 14).to(r.device)
    ref_model.load_state_dict(sd0)
    stats_ref, lr_ref = reference_update_with_mini_batches(ref_model, torch.optim.Adam(ref_model.parameters(), lr=1e-5), full["obses"][:T], full["privileged_obses"][:T],
                                                           full["actions"], full["rewards"].clone(), full["dones"].bool(), full["time_outs"].bool(), full["obses"][T],
                                                           full["privileged_obses"][T], batches)
    assert r.optimizer.step_count == E * K
    compare_with_reference(r, ref_model, stats_ref, lr_ref, p_start, acc)
    moved = float((flat - torch.cat([sd0[k].reshape(-1) for k, _ in r.model.named_parameters()])).abs().max())
    q.put((rank, float((other[0] - other[1]).abs().max()), moved))
    r.dp.shutdown()


def _free_port():
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_update_with_mini_batches_equals_the_reference_on_the_union():
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = []
        for _ in procs:
            item = q.get(timeout=300)
            if item[0] == "error":
                pytest.fail(f"rank {item[1]} raised:\n{item[2]}")
            res.append(item)
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:  # never leave a rank behind holding the GPU, the port and a blocked collective
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
    for rank, rank_diff, moved in res:
        assert rank_diff == 0.0, "ranks diverged"
        assert moved > 1e-6, "parameters did not change"
