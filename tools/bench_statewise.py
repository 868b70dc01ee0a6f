"""Rate of Engine.rollout_statewise (SCPO's collection loop on the device, guardx_amd/statewise.py).

    python tools/bench_statewise.py [--env-num 2000] [--T 200] [--reps 5]

For the Point and the Ant at hidden widths 64 and 256 (the three networks of the same width), alternated in one process:
  statewise      rollout_statewise: two launches per control step
  stepwise_cpo   rollout_policy(..., cost_critic=) under set_policy_impl(3) on the D-input networks: the existing
                 two-launch form plus its batched cost-critic pass -- the like-for-like ceiling
  torch_loop     what an SCPO user has without this path: ac.step(o_aug) in torch + env.step + env.reset_done + the
                 vectorised M update, per control step
Device-synchronised wall time, warm-up, the median of --reps repetitions.  Prints one JSON line: env-steps/s per form.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env-num", type=int, default=2000)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    import torch.nn as nn
    from guardx_amd import Engine
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import task_config, ANT

    def net(D, out, h, seed, tail=()):
        torch.manual_seed(seed)
        return nn.Sequential(nn.Linear(D, h), nn.Tanh(), nn.Linear(h, h), nn.Tanh(), nn.Linear(h, out), *tail)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t

    N, T = args.env_num, args.T
    cases = []
    for robot, extra in (("point", {}), ("ant", ANT)):
        for h in (64, 256):
            cfg = task_config(N, seed=1, num_steps=1000, **extra)
            Es, Ec, El = (Engine(cfg, n_candidates=200000) for _ in range(3))
            Ec.set_policy_impl(3)
            for e in (Es, Ec, El):
                e.reset()
            D, A = Es.obs_flat_size, Es.action_space.shape[0]
            log_std = torch.full((A,), -0.5)
            mu_a, v_a, vc_a = net(D + 1, A, h, 0), net(D + 1, 1, h, 1), net(D + 1, 1, h, 2, (nn.Softplus(),))
            p_a = Engine.pack_actor_critic(mu_net=mu_a, v_net=v_a, log_std=log_std).cuda()
            vc_sp = Engine.pack_critic(vc_a, output='softplus', device='cuda')
            p_d = Engine.pack_actor_critic(mu_net=net(D, A, h, 0), v_net=net(D, 1, h, 1), log_std=log_std).cuda()
            vc_d = Engine.pack_critic(net(D, 1, h, 2), device='cuda')
            mu_a, v_a, vc_a = mu_a.cuda(), v_a.cuda(), vc_a.cuda()
            std = log_std.exp().cuda()

            def torch_loop():
                # scpo.py:640-720 with the per-env Python loop of :647-654 vectorised
                o = El._obs
                M = torch.zeros(N, 1, device='cuda')
                first = torch.ones(N, dtype=torch.bool, device='cuda')
                o_aug = torch.cat((o, M), 1)
                with torch.no_grad():
                    for _ in range(T):
                        mu = mu_a(o_aug)
                        a = mu + std * torch.randn_like(mu)
                        logp = (-((a - mu) ** 2) / (2 * std * std) - std.log() - 0.9189385332046727).sum(-1)
                        v, vc = v_a(o_aug).squeeze(-1), vc_a(o_aug).squeeze(-1)
                        _, r, d, info = El.step(a)
                        cost = info['cost']
                        inc = torch.where(first, cost, (cost - M[:, 0]).clamp_min(0))
                        Mn = torch.where(first, cost, M[:, 0] + inc)
                        o = El.reset_done()
                        fin = d > 0
                        M = torch.where(fin, torch.zeros_like(Mn), Mn).unsqueeze(1)
                        first = fin
                        o_aug = torch.cat((o, M), 1)
                return logp, v, vc

            forms = (("statewise", lambda: Es.rollout_statewise(p_a, T, cost_critic=vc_sp)),
                     ("stepwise_cpo", lambda: Ec.rollout_policy(p_d, T, cost_critic=vc_d)),
                     ("torch_loop", torch_loop))
            for _ in range(args.warmup):
                for _, fn in forms:
                    fn()
            times = {k: [] for k, _ in forms}
            for _ in range(args.reps):
                for k, fn in forms:
                    times[k].append(timed(fn))
            case = dict(robot=robot, D=D, hidden=h)
            for k, ts in times.items():
                case[k + "_Msteps_s"] = round(N * T / statistics.median(ts) / 1e6, 2)
                case[k + "_spread_pct"] = round(100 * (max(ts) - min(ts)) / statistics.median(ts), 1)
            cases.append(case)
            for e in (Es, Ec, El):
                e.close()
    print(json.dumps(dict(tool="bench_statewise", env_num=N, T=T, reps=args.reps, device=torch.cuda.get_device_name(0),
                          cases=cases)), flush=True)


if __name__ == "__main__":
    main()
