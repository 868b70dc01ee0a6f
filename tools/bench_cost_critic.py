"""Cost of the cost-critic pass of rollout_policy(..., cost_critic=) (guardx_amd.critic, libguardx_critic.so).

    python tools/bench_cost_critic.py [--env-num 2000] [--T 200] [--reps 5]

For the Point and the Ant at hidden widths 64, 128 and 256 (actor and cost critic of the same width): rollout_policy
with and without cost_critic, alternated in one process, and the critic pass alone over the same T N + N rows; HIP
events, warm-up, the median of --reps repetitions.  Prints one JSON line: per case the three times, the pass's share of
the rollout, and its share of the FP32 peak (157.3 TFLOPS = 78.6 T FMA/s) from the FMA count h D + h^2 + h per row.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FMA = 157.3e12 / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env-num", type=int, default=2000)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    from guardx_amd import Engine
    from guardx_amd.critic import critic_values
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import task_config, ANT

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

    N, T = args.env_num, args.T
    cases = []
    for robot, extra in (("point", {}), ("ant", ANT)):
        for h in (64, 128, 256):
            E = Engine(task_config(N, seed=1, num_steps=1000, **extra), n_candidates=200000)
            E.reset()
            D, A = E.obs_flat_size, E.action_space.shape[0]
            p = Engine.pack_actor_critic(mu_net=net(D, A, h, 0), v_net=net(D, 1, h, 1),
                                         log_std=torch.full((A,), -0.5)).cuda()
            vc = Engine.pack_critic(net(D, 1, h, 2)).cuda()
            for _ in range(args.warmup):
                E.rollout_policy(p, T)
                out = E.rollout_policy(p, T, cost_critic=vc)
            rows = torch.cat([out['obs'].reshape(T * N, D), out['obs_last']])
            for _ in range(args.warmup):
                critic_values(vc, rows)
            torch.cuda.synchronize()
            t_plain, t_cost, t_pass = [], [], []
            for _ in range(args.reps):
                t_plain.append(timed(lambda: E.rollout_policy(p, T))[0])
                t_cost.append(timed(lambda: E.rollout_policy(p, T, cost_critic=vc))[0])
                t_pass.append(timed(lambda: critic_values(vc, rows))[0])
            plain, cost, cpass = (statistics.median(x) for x in (t_plain, t_cost, t_pass))
            M = (T + 1) * N
            fma = M * (h * D + h * h + h)
            cases.append(dict(robot=robot, D=D, hidden=h, rows=M, rollout_us=round(plain, 1),
                              rollout_with_vc_us=round(cost, 1), pass_us=round(cpass, 1),
                              added_pct=round(100 * (cost - plain) / plain, 1),
                              pass_pct_of_rollout=round(100 * cpass / plain, 1),
                              pass_fp32_peak_pct=round(100 * fma / (cpass * 1e-6) / PEAK_FMA, 1)))
            E.close()
    print(json.dumps(dict(tool="bench_cost_critic", env_num=N, T=T, reps=args.reps, device=torch.cuda.get_device_name(0),
                          cases=cases)), flush=True)


if __name__ == "__main__":
    main()
