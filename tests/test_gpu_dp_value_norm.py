"""algorithm.normalize_value under data parallelism: two ranks (gloo backend, both on the one GPU of the test box, as tests/test_gpu_dp.py) each
simulate 64 envs and run one update under the key.  Both ranks must end with the same parameters and the same normaliser, the normaliser must hold
the float64 statistics of the UNION of both ranks' last-mini-epoch returns, and the exchange tagged "value_norm" must be the last one of the update,
on the main stream, once."""
import math
import os
import sys

import pytest
import torch

from test_gpu_dp import _free_port
from test_value_norm import merge_f64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(rank, world, port, q):
    try:
        _worker_body(rank, world, port, q)
    except BaseException as ex:  # the parent fails fast with the real error instead of a queue time-out
        import traceback

        q.put(("error", rank, "".join(traceback.format_exception(type(ex), ex, ex.__traceback__))))
        raise


def _worker_body(rank, world, port, q):
    os.environ.update(WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      BG_DIST_BACKEND="gloo", BG_LOCAL_DEVICE="0", BG_DP_LOG_ORDER="1")
    sys.path.insert(0, ROOT)
    import torch.distributed as dist

    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.runner import Runner

    E, n = 2, 64
    r = Runner(cfg=load_cfg("T1", {"env.num_envs": n, "terrain.type": "plane", "runner.mini_epochs": E, "algorithm.normalize_value": True}))
    assert r.world_size == 2 and r.rank == rank and r.value_norm is not None
    obs, infos = r.env.reset()
    r.buffer["obses"][0].copy_(obs); r.buffer["privileged_obses"][0].copy_(infos["privileged_obs"])
    r.rollout()
    stats0 = r.value_norm.stats.double().tolist()
    del r.dp.order_log[:]
    r.update()
    torch.cuda.synchronize()

    def gather(t):
        parts = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(parts, t.contiguous())
        return torch.stack(parts)

    flat = gather(torch.cat([p.detach().reshape(-1) for p in r.model.parameters()]))
    states = gather(r.value_norm.state)
    triples = gather(r.value_norm.stats)
    R = (gather(r._ret).double() * stats0[1] + stats0[0]).reshape(-1).cpu().numpy()  # both ranks' returns of the last mini-epoch, in reward units
    q.put((rank, float((flat[0] - flat[1]).abs().max()), bool(torch.equal(states[0], states[1]) and torch.equal(triples[0], triples[1])),
           r.value_norm.state.tolist(), [float(R.sum()), float((R * R).sum()), float(R.size)], list(r.dp.order_log), r.cfg["runner"]["horizon_length"] * n))
    r.dp.shutdown()


def test_two_ranks_merge_the_returns_of_both():
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
    assert res[0][5] == res[1][5], "the ranks enqueued their exchanges in different orders"
    for rank, rank_diff, same_norm, state, sums, order, rows in res:
        assert rank_diff == 0.0 and same_norm, "ranks diverged"
        assert sums[2] == 2 * rows and state[2] == 2 * rows  # every rank's rows, once
        want = merge_f64((0.0, 1.0, 0.0), sums)
        rel = max(abs(g - w) / abs(w) for g, w in zip(state, want))
        print(f"rank {rank}: normaliser {state}, float64 statistics of both ranks' returns {[float(w) for w in want]}: {rel:.3e}")
        assert rel <= 1e-6 and math.isfinite(state[0])
        tags = [t for t, _ in order]
        assert tags.count("value_norm") == 1 and order[-1] == ("value_norm", "main") and tags[-2] == "bucket" and tags.count("moments") == 2, order
