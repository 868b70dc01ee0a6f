"""Rate of Engine.rollout_lpg (the LPG learner's collection loop on the device, guardx_amd/lpg.py).

    python tools/bench_lpg.py [--env-num 2000] [--T 200] [--reps 5] [--delta 0] [--grad-scale 1]

For the Point and the Ant at hidden widths 64 and 256 (the three networks of the same width), alternated in one process:
  lpg              rollout_lpg(correct=True, delta): two launches per control step
  stepwise_policy  rollout_policy under set_policy_impl(3): the existing two-launch form -- the floor that two networks
                   and no correction cost
  torch_loop       what an LPG user has without this path: ac.step(o) with Q(o, a) in torch + the reference's
                   safety_correction (a second c_net forward, a third at the zero action with an autograd backward of
                   its mean, three device-to-host copies and the projection in float64 numpy, lpg_core.py:171-198) +
                   env.step + env.reset_done, per control step
Device-synchronised wall time, warm-up, the median of --reps repetitions.  Prints one JSON line: env-steps/s per form with
its spread, and the share of corrected rows (lam > 0) of the device path.  --grad-scale defaults to 1 here (the library's
default is the reference's 1 / env_num, with which almost every lam is clipped to 0; the cost does not depend on it).
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
    ap.add_argument("--delta", type=float, default=0.0)
    ap.add_argument("--grad-scale", type=float, default=1.0)
    args = ap.parse_args()
    import numpy as np
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
            mu_n, v_n = net(D, A, h, 0), net(D, 1, h, 1)
            c_n = nn.Sequential(*net(D + A, 1, h, 2), nn.Softplus())
            p = Engine.pack_actor_critic(mu_net=mu_n, v_net=v_n, log_std=log_std).cuda()
            qp = Engine.pack_q_critic(c_n, device='cuda')
            mu_n, v_n, c_n = mu_n.cuda(), v_n.cuda(), c_n.cuda()
            std = log_std.exp().cuda()
            delta, gs = args.delta, args.grad_scale

            def safety_correction(o, act, q_init):
                # lpg_core.py:171-198 restated with grad_scale in place of the mean's 1 / N and lam on every component
                pred = c_n(torch.cat((o, act), 1)).squeeze(-1)
                act_0 = torch.zeros_like(act).requires_grad_()
                c_n.zero_grad()
                pred_0 = c_n(torch.cat((o, act_0), 1)).squeeze(-1)
                (pred_0.sum() * gs).backward()
                out = act.clone()
                index = np.where(pred.detach().cpu().numpy() > delta)
                G = act_0.grad.cpu().numpy()[index]
                act_np = act.detach().cpu().numpy()[index]
                eps = abs(np.asarray(delta) - q_init[index])
                with np.errstate(all='ignore'):
                    lam = (np.sum(G * act_np, axis=1) - eps) / np.sum(G * G, axis=1)
                lam[np.where(lam < 0)] = 0.0
                tmp = torch.as_tensor(lam.reshape(-1, 1) * G, dtype=torch.float32).cuda()
                idx = torch.as_tensor(index[0], device='cuda')
                out[idx] = act[idx] + tmp
                return out.detach()

            def torch_loop():
                # lpg.py:486-564
                o = El._obs
                q_init = None
                for t in range(T):
                    with torch.no_grad():
                        mu = mu_n(o)
                        a = mu + std * torch.randn_like(mu)
                        logp = (-((a - mu) ** 2) / (2 * std * std) - std.log() - 0.9189385332046727).sum(-1)
                        v = v_n(o).squeeze(-1)
                        qc = c_n(torch.cat((o, a), 1)).squeeze(-1)
                    if t == 0:
                        q_init = np.asarray(qc.cpu().numpy(), dtype=np.double)
                    a_safe = safety_correction(o, a, q_init)
                    El.step(a_safe)
                    o = El.reset_done()
                return logp, v, qc

            lams = []

            def lpg():
                lams.append(Es.rollout_lpg(p, T, q_critic=qp, delta=delta, grad_scale=gs)['lam'])

            forms = (("lpg", lpg),
                     ("stepwise_policy", lambda: Ep.rollout_policy(p, T)),
                     ("torch_loop", torch_loop))
            for _ in range(args.warmup):
                for _, fn in forms:
                    fn()
            times = {k: [] for k, _ in forms}
            for _ in range(args.reps):
                for k, fn in forms:
                    times[k].append(timed(fn))
            case = dict(robot=robot, D=D, hidden=h,
                        corrected_share=round(float((torch.stack(lams[args.warmup:]) > 0).float().mean()), 3))
            for k, ts in times.items():
                case[k + "_Msteps_s"] = round(N * T / statistics.median(ts) / 1e6, 2)
                case[k + "_spread_pct"] = round(100 * (max(ts) - min(ts)) / statistics.median(ts), 1)
            cases.append(case)
            for e in (Es, Ep, El):
                e.close()
    print(json.dumps(dict(tool="bench_lpg", env_num=N, T=T, reps=args.reps, delta=args.delta, grad_scale=args.grad_scale,
                          device=torch.cuda.get_device_name(0), cases=cases)), flush=True)


if __name__ == "__main__":
    main()
