"""Rate of Engine.rollout_safelayer (the safety-layer learner's collection loop on the device, guardx_amd/safelayer.py).

    python tools/bench_safelayer.py [--env-num 2000] [--T 200] [--reps 5]

For the Point and the Ant at hidden widths 64 and 256 (the three networks of the same width), alternated in one process:
  safelayer        rollout_safelayer(correct=True): two launches per control step
  stepwise_policy  rollout_policy under set_policy_impl(3): the existing two-launch form -- the floor that two networks
                   and no correction cost
  torch_loop       what a safelayer user has without this path: ac.step(o) in torch + safety_correction in torch +
                   env.step + env.reset_done, per control step
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

    def net(D, out, h, seed):
        torch.manual_seed(seed)
        return nn.Sequential(nn.Linear(D, h), nn.Tanh(), nn.Linear(h, h), nn.Tanh(), nn.Linear(h, out))

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
            Es, Ep, El = (Engine(cfg, n_candidates=200000) for _ in range(3))
            Ep.set_policy_impl(3)
            for e in (Es, Ep, El):
                e.reset()
            D, A = Es.obs_flat_size, Es.action_space.shape[0]
            log_std = torch.full((A,), -0.5)
            mu_n, v_n, g_n = net(D, A, h, 0), net(D, 1, h, 1), net(D, A, h, 2)
            p = Engine.pack_actor_critic(mu_net=mu_n, v_net=v_n, log_std=log_std).cuda()
            gp = Engine.pack_g_net(g_n, device='cuda', act_dim=A)
            mu_n, v_n, g_n = mu_n.cuda(), v_n.cuda(), g_n.cuda()
            std = log_std.exp().cuda()

            def torch_loop():
                # safelayer.py:514-581 with safety_correction (safelayer_core.py:169-190) in its vectorised general form
                o = El._obs
                prev_c = torch.zeros(N, device='cuda')
                with torch.no_grad():
                    for _ in range(T):
                        mu = mu_n(o)
                        a = mu + std * torch.randn_like(mu)
                        logp = (-((a - mu) ** 2) / (2 * std * std) - std.log() - 0.9189385332046727).sum(-1)
                        v = v_n(o).squeeze(-1)
                        g = g_n(o)
                        pred = (g * a).sum(-1) + prev_c
                        mult = torch.relu(pred / ((g * g).sum(-1) + 1e-8))
                        a_safe = torch.where((pred > 0).unsqueeze(1), (a - mult.unsqueeze(1) * g).clamp(-1, 1), a)
                        _, r, d, info = El.step(a_safe)
                        o = El.reset_done()
                        prev_c = torch.where(d > 0, torch.zeros_like(d), info['cost'])
                return logp, v

            forms = (("safelayer", lambda: Es.rollout_safelayer(p, T, g_net=gp)),
                     ("stepwise_policy", lambda: Ep.rollout_policy(p, T)),
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
            for e in (Es, Ep, El):
                e.close()
    print(json.dumps(dict(tool="bench_safelayer", env_num=N, T=T, reps=args.reps, device=torch.cuda.get_device_name(0),
                          cases=cases)), flush=True)


if __name__ == "__main__":
    main()
