"""combine_episode_stats over two gloo ranks: each rank takes the statistics of its own env shard, one all_gather of
(n, S, Q, min, max) per key makes the all-rank statistics on both, and they are those of the concatenated entries."""
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

T, N = 16, 40          # per rank
FIELDS = ('n', 'S', 'mean', 'Q', 'std', 'min', 'max')


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard(rank, empty_rank):
    """the (T, N) tensors of one rank; `empty_rank` never finishes an episode inside the call (max_ep_len > T)"""
    rng = np.random.default_rng(100 + rank)
    f = np.float32
    done = (rng.random((T, N)) < (0.0 if rank == empty_rank else 0.2)).astype(f)
    return dict(rew=(rng.normal(size=(T, N)) + 3.0 * rank).astype(f), cost=rng.random((T, N)).astype(f), done=done,
                val=rng.normal(size=(T, N)).astype(f))


def _worker(rank, world, port, empty_rank, q):
    try:
        sys.path.insert(0, ROOT)
        os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                          MASTER_PORT=str(port))
        from guardx_amd import dist as gxd
        from guardx_amd.epstats import combine_episode_stats, episode_stats
        gxd.init_from_env(backend="gloo")
        d = _shard(rank, empty_rank)
        own = episode_stats(*[torch.from_numpy(d[k]) for k in ('rew', 'cost', 'done')], val=torch.from_numpy(d['val']),
                            gamma=0.99, max_ep_len=T + 4)
        both = combine_episode_stats(own)
        flat = {k: {f: float(v[f]) for f in FIELDS} for k, v in both.items() if isinstance(v, dict) and 'mean' in v}
        flat['cost_sum'], flat['n_episodes'] = float(both['cost_sum']), int(both['n_episodes'])
        flat['own_n'] = float(own['EpRet']['n'])
        gxd.barrier()
        q.put(("ok", rank, flat))
        torch.distributed.destroy_process_group()
    except Exception:  # noqa: BLE001
        import traceback
        q.put(("fail", rank, traceback.format_exc()))
        raise


@pytest.mark.timeout(300)
@pytest.mark.parametrize("empty_rank", [None, 1])
def test_two_ranks_combine_to_the_statistics_of_all_entries(empty_rank):
    import epstats64 as e64
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, empty_rank, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(world):
        tag, rank, flat = q.get(timeout=240)
        assert tag == "ok", flat
        got[rank] = flat
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    same = lambda a, b: a == b or (math.isnan(a) and math.isnan(b))   # noqa: E731
    own_n = [got[r].pop('own_n') for r in range(world)]
    assert (own_n[1] == 0) == (empty_rank == 1) and own_n[0] > 0
    for k in got[0]:                                                  # identical on both ranks, bit for bit
        if isinstance(got[0][k], dict):
            assert all(same(got[0][k][f], got[1][k][f]) for f in FIELDS), k
        else:
            assert got[0][k] == got[1][k], k
    # the entries of both shards, rank after rank, from the restatement of the learner loop
    logs = []
    for r in range(world):
        d = _shard(r, empty_rank)
        logs.append(e64.learner_loop(d['rew'], d['cost'], d['done'], max_ep_len=T + 4, gamma=0.99, val=d['val'])[0])
    assert set(got[0]) == {'EpRet', 'EpCost', 'EpLen', 'EpCostRet', 'VVals', 'cost_sum', 'n_episodes'}
    assert got[0]['n_episodes'] == sum(len(lg['env']) for lg in logs)
    costs = [c for lg in logs for c in lg['cost_env']]
    assert abs(got[0]['cost_sum'] - math.fsum(costs)) <= e64.sum_bound(costs)
    for k in ('EpRet', 'EpCost', 'EpLen', 'EpCostRet', 'VVals'):
        x = e64.logged([v for lg in logs for v in lg[k]])
        want, g = e64.stats64(x), got[0][k]
        n = len(x)
        assert g['n'] == n and g['min'] == want['min'] and g['max'] == want['max'], k
        # S: each rank's float64 sum and the sum of the two are one float64 summation of all n entries in some order
        bS = e64.sum_bound(x)
        assert abs(g['S'] - want['S']) <= bS, k
        dm = bS / n + e64.U * abs(want['mean'])
        assert abs(g['mean'] - want['mean']) <= dm, k
        # Q: per rank sum (x - m_r)^2 + n_r (m_r - m)^2 = sum (x - m)^2 exactly, in exact arithmetic, for any m; in float64 a
        # sum of about n terms of total sum (x - m)^2 (every term within a few u of its exact value), with means m_r, m off
        # by at most dm each: d/dm moves it by 2 |dm| sum |x - m| + n dm^2 per mean
        dev = math.fsum(abs(v - want['mean']) for v in x)
        bQ = (n + 8) * e64.U * want['Q'] + 3 * (2 * dm * dev + n * dm * dm)
        assert abs(g['Q'] - want['Q']) <= bQ, (k, g['Q'] - want['Q'], bQ)
        # std = sqrt(Q / n): the relative error of Q halves, plus the division's and the root's rounding
        assert abs(g['std'] - want['std']) <= want['std'] * (0.5 * bQ / want['Q'] + 3 * e64.U), k


def test_a_world_of_one_returns_its_input():
    from guardx_amd.epstats import combine_episode_stats, episode_stats
    d = _shard(0, None)
    own = episode_stats(*[torch.from_numpy(d[k]) for k in ('rew', 'cost', 'done')])
    assert combine_episode_stats(own) is own
