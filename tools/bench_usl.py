"""Rate of Engine.rollout_usl (the USL learner's collection loop on the device, guardx_amd/usl.py).

    python tools/bench_usl.py [--env-num 2000] [--T 200] [--reps 5] [--niter 20] [--delta 0]

For the Point and the Ant at hidden widths 64 and 256 (the three networks of the same width), alternated in one process:
  usl              rollout_usl(correct=True, delta, niter): two launches per control step
  stepwise_policy  rollout_policy under set_policy_impl(3): the existing two-launch form -- the floor that two networks
                   and no correction cost
  torch_loop       what a USL user has without this path: ac.step(o) with Q(o, a) in torch + a torch safety_correction
                   (up to niter autograd passes through c_net with its index bookkeeping, usl_core.py:165-196) +
                   env.step + env.reset_done, per control step
Device-synchronised wall time, warm-up, the median of --reps repetitions.  Prints one JSON line: env-steps/s per form and
the mean number of updates per env-step of the device path (the cost scales with it).
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
    ap.add_argument("--niter", type=int, default=20)
    ap.add_argument("--delta", type=float, default=0.0)
    ap.add_argument("--eta", type=float, default=0.05)
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
            mu_n, v_n = net(D, A, h, 0), net(D, 1, h, 1)
            c_n = nn.Sequential(*net(D + A, 1, h, 2), nn.Softplus())
            p = Engine.pack_actor_critic(mu_net=mu_n, v_net=v_n, log_std=log_std).cuda()
            qp = Engine.pack_q_critic(c_n, device='cuda')
            mu_n, v_n, c_n = mu_n.cuda(), v_n.cuda(), c_n.cuda()
            std = log_std.exp().cuda()
            niter, delta, eta = args.niter, args.delta, args.eta

            def safety_correction(o, act):
                # usl_core.py:165-196 restated: frozen rows are kept as an index set, every pass is a forward and an
                # autograd backward of pred.mean() through c_net into act.grad, which the reference never clears
                # (usl_core.py:180-194): the update uses the running sum, normalised by the row's largest |sum|
                act = act.clone()
                acc = None
                rows = torch.arange(N, device='cuda')
                frozen = torch.zeros(N, dtype=torch.bool, device='cuda')
                with torch.no_grad():
                    frozen |= c_n(torch.cat((o, act), 1)).squeeze(-1) <= delta
                for _ in range(niter):
                    frozen |= act.max(1).values > 1
                    if bool(frozen.all()):
                        break
                    act.requires_grad_()
                    pred = c_n(torch.cat((o, act), 1)).squeeze(-1)
                    grad, = torch.autograd.grad(pred.mean(), act)
                    grad = acc = grad if acc is None else acc + grad
                    frozen |= pred.detach() <= delta
                    if bool(frozen.all()):
                        break
                    act = act.detach()
                    Z = grad.abs().max(1).values
                    upd = rows[~frozen]
                    act[upd] = act[upd] - eta * grad[upd] / (Z[upd].unsqueeze(-1) + 1e-8)
                return act.detach()

            def torch_loop():
                # usl.py:478-553
                o = El._obs
                for _ in range(T):
                    with torch.no_grad():
                        mu = mu_n(o)
                        a = mu + std * torch.randn_like(mu)
                        logp = (-((a - mu) ** 2) / (2 * std * std) - std.log() - 0.9189385332046727).sum(-1)
                        v = v_n(o).squeeze(-1)
                        qc = c_n(torch.cat((o, a), 1)).squeeze(-1)
                    a_safe = safety_correction(o, a)
                    El.step(a_safe)
                    o = El.reset_done()
                return logp, v, qc

            iters = []

            def usl():
                iters.append(Es.rollout_usl(p, T, q_critic=qp, delta=delta, niter=niter, eta=eta)['iters'])

            forms = (("usl", usl),
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
                        mean_iters=round(float(torch.stack(iters[args.warmup:]).mean()), 2))
            for k, ts in times.items():
                case[k + "_Msteps_s"] = round(N * T / statistics.median(ts) / 1e6, 2)
                case[k + "_spread_pct"] = round(100 * (max(ts) - min(ts)) / statistics.median(ts), 1)
            cases.append(case)
            for e in (Es, Ep, El):
                e.close()
    print(json.dumps(dict(tool="bench_usl", env_num=N, T=T, reps=args.reps, niter=args.niter, delta=args.delta, device=torch.cuda.get_device_name(0),
                          cases=cases)), flush=True)


if __name__ == "__main__":
    main()
