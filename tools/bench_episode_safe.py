"""Rate of the one-episode form of the three safe-action rollouts, Engine.rollout_safelayer / rollout_usl /
rollout_lpg(..., episode=True) + rollout_buffer.episode_rollout_batch (the collection loop and buffer of the
`safelayer_`, `usl_` and `lpg_one_episode` learners on the device).

    python tools/bench_episode_safe.py [--env-num 2000] [--T 200] [--reps 5] [--learners safelayer,usl,lpg] [--forms ...]

For each learner, the Point and the Ant at hidden widths 64 and 256 (the third network of the same width), correct=True,
alternated in one process:
  episode     episode=True + episode_rollout_batch: two launches per control step, two for the batch, one .item()
  reset_form  the same learner's episode=False rollout (reset_done speculated in the env launch, committed on the host)
  torch_loop  what the one-episode learner has without this path (safelayer_one_episode/safelayer.py:499-578,
              usl_one_episode/usl.py:463-543, lpg_one_episode/lpg.py:473-554): the NaN / Inf edit, ac.step(o) and the
              correction in torch (USL: up to 20 autograd passes through c_net, LPG: one), env.step, the .cpu() of done
              every step, then finish_path / get over [0, first_done) in torch
Between repetitions the path's bookkeeping is cleared directly (the envs go on: num_steps = 1000).  Device-synchronised
wall time, warm-up, the median of --reps repetitions with the spread (max - min) / median.  Prints one JSON line.
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
    ap.add_argument("--learners", default="safelayer,usl,lpg")
    ap.add_argument("--forms", default="episode,reset_form,torch_loop", help="a subset, e.g. one form alone under a profiler")
    args = ap.parse_args()
    import torch
    import torch.nn as nn
    from guardx_amd import Engine
    from guardx_amd.rollout_buffer import episode_rollout_batch
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
    gamma, lam = 0.99, 0.95
    delta = dict(safelayer=0.0, usl=0.5, lpg=0.5)
    cases = []
    for learner in args.learners.split(","):
        for robot, extra in (("point", {}), ("ant", ANT)):
            for h in (64, 256):
                cfg = task_config(N, seed=1, num_steps=1000, **extra)
                Ee, Er, El = (Engine(cfg, n_candidates=200000) for _ in range(3))
                for e in (Ee, Er, El):
                    e.reset()
                D, A = Ee.obs_flat_size, Ee.action_space.shape[0]
                log_std = torch.full((A,), -0.5)
                mu_n, v_n = net(D, A, h, 0), net(D, 1, h, 1)
                p = Engine.pack_actor_critic(mu_net=mu_n, v_net=v_n, log_std=log_std).cuda()
                if learner == "safelayer":
                    third = net(D, A, h, 2)
                    kw = dict(g_net=Engine.pack_g_net(third, device='cuda', act_dim=A), delta=delta[learner])
                else:
                    third = net(D + A, 1, h, 2, (nn.Softplus(),))
                    kw = dict(q_critic=Engine.pack_q_critic(third, device='cuda'), delta=delta[learner])
                mu_n, v_n, third = mu_n.cuda(), v_n.cuda(), third.cuda()
                std = log_std.exp().cuda()
                dl = delta[learner]

                def episode():
                    st = getattr(Ee, "_" + learner)
                    if st is not None:
                        st.reset_book()              # a new episode for the bookkeeping; the envs go on
                    return episode_rollout_batch(getattr(Ee, "rollout_" + learner)(p, T, episode=True, **kw), gamma, lam)

                def reset_form():
                    return getattr(Er, "rollout_" + learner)(p, T, **kw)

                def correct(o, a, prev_c, state):
                    """-> a_safe and the learner's own column (prev_cost or qc)"""
                    if learner == "safelayer":           # safelayer_core.py:169-190
                        g = third(o)
                        pred = (g * a).sum(-1) + prev_c
                        mult = torch.relu((pred - dl) / ((g * g).sum(-1) + 1e-8))
                        return torch.where((pred > dl).unsqueeze(-1), (a - mult.unsqueeze(-1) * g).clamp(-1, 1), a), prev_c
                    qc = third(torch.cat([o, a], -1)).squeeze(-1)
                    if learner == "usl":                 # usl_core.py:165-196
                        x = a.clone()
                        for _ in range(20):
                            x.requires_grad_(True)
                            with torch.enable_grad():
                                pred = third(torch.cat([o, x], -1)).squeeze(-1)
                                if bool(((x.max(-1).values > 1) | (pred <= dl)).all()):
                                    break
                                s, = torch.autograd.grad(pred.mean(), x)
                            live = ~((x.max(-1).values > 1) | (pred <= dl))
                            step = 0.05 * s / (s.abs().max(-1, keepdim=True).values + 1e-8)
                            x = torch.where(live.unsqueeze(-1), x.detach() - step, x.detach())
                        return x.detach(), qc
                    if state.get('q_init') is None:      # lpg_core.py:161-198
                        state['q_init'] = qc
                    z = torch.zeros_like(a).requires_grad_(True)
                    with torch.enable_grad():
                        G, = torch.autograd.grad(third(torch.cat([o, z], -1)).mean(), z)
                    eps = (dl - state['q_init']).abs()
                    lm = torch.relu(((G * a).sum(-1) - eps) / (G * G).sum(-1))
                    return torch.where((qc > dl).unsqueeze(-1), a + lm.unsqueeze(-1) * G, a), qc

                def torch_loop():
                    o = El._obs
                    rows = dict(obs=[], act=[], act_safe=[], mu=[], logp=[], val=[], rew=[], cost=[], own=[])
                    first = [0] * N
                    prev_c, state = torch.zeros(N, device='cuda'), {}
                    with torch.no_grad():
                        for t in range(T):
                            o = torch.where(torch.isfinite(o), o, torch.zeros_like(o))
                            mu = mu_n(o)
                            a = mu + std * torch.randn_like(mu)
                            logp = (-((a - mu) ** 2) / (2 * std * std) - std.log() - 0.9189385332046727).sum(-1)
                            v = v_n(o).squeeze(-1)
                            a_safe, own = correct(o, a, prev_c, state)
                            o2, r, d, info = El.step(a_safe)
                            for k, x in (('obs', o), ('act', a), ('act_safe', a_safe), ('mu', mu), ('logp', logp), ('val', v),
                                         ('rew', r), ('cost', info['cost']), ('own', own)):
                                rows[k].append(x)
                            for e in (d.cpu() > 0).nonzero().flatten().tolist():
                                if not first[e]:
                                    first[e] = t + 1
                            o, prev_c = o2, info['cost']
                        fd = torch.tensor(first, device='cuda')
                        L = torch.where(fd > 0, fd, torch.full_like(fd, T))
                        ok = torch.isfinite(o).all(1) & (fd == 0)
                        clean = torch.where(torch.isfinite(o), o, torch.zeros_like(o))
                        stack = {k: torch.stack(x) for k, x in rows.items()}
                        last = torch.where(ok, v_n(clean).squeeze(-1), 0.0)
                        rew, val = stack['rew'], stack['val']
                        adv, ret = torch.zeros_like(rew), torch.zeros_like(rew)
                        ac, rt, vn = torch.zeros_like(last), last.clone(), last.clone()
                        for t in range(T - 1, -1, -1):
                            m = L > t
                            ac = torch.where(m, rew[t] + gamma * vn - val[t] + gamma * lam * ac, ac)
                            rt = torch.where(m, rew[t] + gamma * rt, rt)
                            adv[t], ret[t] = torch.where(m, ac, adv[t]), torch.where(m, rt, ret[t])
                            vn = torch.where(m, val[t], vn)
                        adv = (adv - adv.mean(0)) / adv.std(0, unbiased=False)
                        valid = (torch.arange(T, device='cuda').view(1, T) < L.view(N, 1)).reshape(N * T)
                        flat = lambda x: x.transpose(0, 1).reshape(N * T, *x.shape[2:])[valid]   # noqa: E731
                        batch = {k: flat(stack[k]) for k in ('obs', 'act', 'act_safe', 'mu', 'logp', 'cost')}
                        batch.update(adv=flat(adv), ret=flat(ret))
                        if learner == "safelayer":
                            batch['prev_cost'] = flat(stack['own'])
                        else:
                            qn = torch.zeros_like(stack['own'])
                            qn[:-1] = stack['own'][1:]
                            qn = torch.where(torch.arange(1, T + 1, device='cuda').view(T, 1) < L.view(1, N), qn, torch.zeros_like(qn))
                            batch['targetc'] = flat(stack['cost'] + gamma * qn)
                    return batch

                forms = tuple((k, fn) for k, fn in (("episode", episode), ("reset_form", reset_form), ("torch_loop", torch_loop))
                              if k in args.forms.split(","))
                for _ in range(args.warmup):
                    for _, fn in forms:
                        fn()
                times = {k: [] for k, _ in forms}
                for _ in range(args.reps):
                    for k, fn in forms:
                        times[k].append(timed(fn))
                case = dict(learner=learner, robot=robot, D=D, hidden=h)
                for k, ts in times.items():
                    case[k + "_Msteps_s"] = round(N * T / statistics.median(ts) / 1e6, 3)
                    case[k + "_spread_pct"] = round(100 * (max(ts) - min(ts)) / statistics.median(ts), 1)
                cases.append(case)
                print(json.dumps(case), file=sys.stderr, flush=True)
                for e in (Ee, Er, El):
                    e.close()
    print(json.dumps(dict(tool="bench_episode_safe", env_num=N, T=T, reps=args.reps, device=torch.cuda.get_device_name(0),
                          cases=cases)), flush=True)


if __name__ == "__main__":
    main()
