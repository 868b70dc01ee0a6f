"""Cost of episode_stats (guardx_amd.epstats, libguardx_epstats.so) next to the collection phase it follows.

    python tools/bench_epstats.py [--env-num 2000] [--T 200] [--reps 20] [--warmup 5]

Goal_Point_8Hazards, num_steps = T (the bench's epoch), the (64, 64)-tanh actor-critic: rollout_policy, then on its
result gae_rollout and episode_stats (with VVals and EpCostRet, i.e. the whole of it; also without val and gamma), each
timed alone with HIP events after --warmup calls, the median of --reps.  Prints one JSON line with the three times in
microseconds and the statistics call's share of the rollout (DESIGN.md asks for under 10 %).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env-num", type=int, default=2000)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    from guardx_amd import Engine
    from guardx_amd.epstats import episode_stats
    from guardx_amd.rollout_buffer import gae_rollout
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import task_config

    def net(D, out, h, seed):
        torch.manual_seed(seed)
        return torch.nn.Sequential(torch.nn.Linear(D, h), torch.nn.Tanh(), torch.nn.Linear(h, h), torch.nn.Tanh(),
                                   torch.nn.Linear(h, out))

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3, r       # us

    def median(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        return statistics.median(timed(fn)[0] for _ in range(args.reps))

    N, T = args.env_num, args.T
    E = Engine(task_config(N, seed=1, num_steps=T), n_candidates=200000)
    E.reset()
    D, A = E.obs_flat_size, E.action_space.shape[0]
    p = Engine.pack_actor_critic(mu_net=net(D, A, 64, 0), v_net=net(D, 1, 64, 1), log_std=torch.full((A,), -0.5)).cuda()
    rollout = median(lambda: E.rollout_policy(p, T))
    out = E.rollout_policy(p, T)
    gae = median(lambda: gae_rollout(out['rew'], out['val'], out['done']))
    full = median(lambda: episode_stats(out, gamma=0.99))
    plain = median(lambda: episode_stats(out, val=False))
    n_ep = int(episode_stats(out)['n_episodes'])
    E.close()
    print(json.dumps(dict(tool="bench_epstats", env_num=N, T=T, reps=args.reps, warmup=args.warmup,
                          device=torch.cuda.get_device_name(0), episodes=n_ep, rollout_policy_us=round(rollout, 1),
                          gae_rollout_us=round(gae, 1), episode_stats_us=round(full, 1),
                          episode_stats_no_val_no_gamma_us=round(plain, 1),
                          episode_stats_pct_of_rollout=round(100 * full / rollout, 2))), flush=True)


if __name__ == "__main__":
    main()
