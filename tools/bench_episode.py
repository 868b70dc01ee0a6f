"""Rate of Engine.rollout_episode + rollout_buffer.episode_rollout_batch (the `*_one_episode` learners' collection loop
and buffer on the device, guardx_amd/episode.py).

    python tools/bench_episode.py [--env-num 2000] [--T 200] [--reps 5]

For the Point and the Ant at hidden widths 64 and 256, without and with a cost critic (of the same width), alternated in
one process:
  episode          rollout_episode + episode_rollout_batch: two launches per control step, two for the batch, one .item()
  stepwise_policy  rollout_policy under set_policy_impl(3) (+ the batched cost critic pass): the existing two-launch
                   form with reset_done -- the floor
  torch_loop       what a one-episode learner has without this path (trpo_one_episode/trpo.py:450-545): the NaN / Inf
                   edit and ac.step(o) in torch, env.step, the .cpu() of done every step, then finish_path / get over
                   [0, first_done) in torch
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
    from guardx_amd.rollout_buffer import episode_rollout_batch
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
    gamma, lam = 0.99, 0.95
    cases = []
    for robot, extra in (("point", {}), ("ant", ANT)):
        for h in (64, 256):
            for with_vc in (False, True):
                cfg = task_config(N, seed=1, num_steps=1000, **extra)
                Ee, Ep, El = (Engine(cfg, n_candidates=200000) for _ in range(3))
                Ep.set_policy_impl(3)
                for e in (Ee, Ep, El):
                    e.reset()
                D, A = Ee.obs_flat_size, Ee.action_space.shape[0]
                log_std = torch.full((A,), -0.5)
                mu_n, v_n, vc_n = net(D, A, h, 0), net(D, 1, h, 1), net(D, 1, h, 2)
                p = Engine.pack_actor_critic(mu_net=mu_n, v_net=v_n, log_std=log_std).cuda()
                vcp = Engine.pack_critic(vc_n, device='cuda') if with_vc else None
                mu_n, v_n, vc_n = mu_n.cuda(), v_n.cuda(), vc_n.cuda()
                std = log_std.exp().cuda()

                def episode():
                    if Ee._episode is not None:
                        Ee._episode.reset_book()     # a new episode for the bookkeeping; the envs go on (num_steps = 1000)
                    return episode_rollout_batch(Ee.rollout_episode(p, T, cost_critic=vcp), gamma, lam)

                def stepwise():
                    return Ep.rollout_policy(p, T, cost_critic=vcp)

                def channel(rew, val, last, L):
                    # finish_path over [0, L) and the statistics over all T entries, vectorised over the envs
                    adv, ret = torch.zeros_like(rew), torch.zeros_like(rew)
                    a, r, vn = torch.zeros_like(last), last.clone(), last.clone()
                    for t in range(T - 1, -1, -1):
                        m = L > t
                        a = torch.where(m, rew[t] + gamma * vn - val[t] + gamma * lam * a, a)
                        r = torch.where(m, rew[t] + gamma * r, r)
                        adv[t], ret[t] = torch.where(m, a, adv[t]), torch.where(m, r, ret[t])
                        vn = torch.where(m, val[t], vn)
                    return adv, ret

                def torch_loop():
                    o = El._obs
                    rows = dict(obs=[], act=[], mu=[], logp=[], val=[], rew=[], vc=[], cost=[])
                    first = [0] * N
                    with torch.no_grad():
                        for t in range(T):
                            o = torch.where(torch.isfinite(o), o, torch.zeros_like(o))        # trpo.py:453-454
                            mu = mu_n(o)
                            a = mu + std * torch.randn_like(mu)
                            logp = (-((a - mu) ** 2) / (2 * std * std) - std.log() - 0.9189385332046727).sum(-1)
                            v = v_n(o).squeeze(-1)
                            if with_vc:
                                rows['vc'].append(vc_n(o).squeeze(-1))
                            o2, r, d, info = El.step(a)
                            for k, x in (('obs', o), ('act', a), ('mu', mu), ('logp', logp), ('val', v), ('rew', r),
                                         ('cost', info['cost'])):
                                rows[k].append(x)
                            for e in (d.cpu() > 0).nonzero().flatten().tolist():              # trpo.py:496
                                if not first[e]:
                                    first[e] = t + 1
                            o = o2
                        fd = torch.tensor(first, device='cuda')
                        L = torch.where(fd > 0, fd, torch.full_like(fd, T))
                        ok = torch.isfinite(o).all(1) & (fd == 0)
                        clean = torch.where(torch.isfinite(o), o, torch.zeros_like(o))
                        stack = {k: torch.stack(x) for k, x in rows.items() if x}
                        adv, ret = channel(stack['rew'], stack['val'], torch.where(ok, v_n(clean).squeeze(-1), 0.0), L)
                        adv = (adv - adv.mean(0)) / adv.std(0, unbiased=False)
                        valid = (torch.arange(T, device='cuda').view(1, T) < L.view(N, 1)).reshape(N * T)
                        flat = lambda x: x.transpose(0, 1).reshape(N * T, *x.shape[2:])[valid]   # noqa: E731
                        batch = {k: flat(stack[k]) for k in ('obs', 'act', 'mu', 'logp')}
                        batch.update(adv=flat(adv), ret=flat(ret))
                        if with_vc:
                            adc, cret = channel(stack['cost'], stack['vc'], torch.where(ok, vc_n(clean).squeeze(-1), 0.0), L)
                            batch.update(adc=flat(adc - adc.mean(0)), cost_ret=flat(cret))
                    return batch

                forms = (("episode", episode), ("stepwise_policy", stepwise), ("torch_loop", torch_loop))
                for _ in range(args.warmup):
                    for _, fn in forms:
                        fn()
                times = {k: [] for k, _ in forms}
                for _ in range(args.reps):
                    for k, fn in forms:
                        times[k].append(timed(fn))
                case = dict(robot=robot, D=D, hidden=h, cost_critic=with_vc)
                for k, ts in times.items():
                    case[k + "_Msteps_s"] = round(N * T / statistics.median(ts) / 1e6, 2)
                    case[k + "_spread_pct"] = round(100 * (max(ts) - min(ts)) / statistics.median(ts), 1)
                cases.append(case)
                for e in (Ee, Ep, El):
                    e.close()
    print(json.dumps(dict(tool="bench_episode", env_num=N, T=T, reps=args.reps, device=torch.cuda.get_device_name(0),
                          cases=cases)), flush=True)


if __name__ == "__main__":
    main()
