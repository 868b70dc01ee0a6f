"""A/B of the first-order learners' actor update: guardx_amd.pifit (libguardx_pifit.so) against the learners' own loop.

    python tools/ab_pifit.py [--B 400000] [--D 43] [--A 2] [--iters 80] [--reps 7] [--warmup 2] [--out profiles/ab_pifit.json]

Point's actor (43 -> 64 -> 64 -> 2, tanh, a free log_std) over B = env_num x T = 2000 x 200 rows, seeded inputs as a rollout of
the actor leaves them (logp_old its own log-probability, adv standardised), lr = 3e-4, clip_ratio = 0.2.
  theirs   the loop of ppo_one_episode/ppo.py:307-316 in torch on the same device: zero_grad, compute_loss_pi with its three
           .item() calls (kl, ent, cf), `if kl > target_kl: break`, backward, Adam's step.
  ours     PolicyFit.fit(data, iters, target_kl, clip_ratio).
Both start from equal state (a fresh copy of the actor and a new optimizer, made before the clock starts).  A host clock around
each, ended by a device synchronise, the two alternating in one process, the median of --reps after --warmup with min .. max.
Twice: with a target_kl that never stops, and with one that stops early (halfway between the kl entries on either side of
iteration --stop-at of our own unstopped trace, so both sides stop there).  Also: the floor that the 2 iters launches set (the
same call over one row), both sides' stop_iter and last kl, and, on a subsample of 4099 rows, the relative L2 of both sides'
displacement after --iters unstopped iterations against tests/pifit64.py:fit64.
One JSON line on stdout and, with --out, in that file.  Needs a GPU: there is no CPU path to time.
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=400000)
    ap.add_argument("--D", type=int, default=43)
    ap.add_argument("--A", type=int, default=2)
    ap.add_argument("--iters", type=int, default=80)
    ap.add_argument("--stop-at", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sub", type=int, default=4099)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from torch.distributions.normal import Normal
    import fisher64 as f64
    import linesearch64 as l64
    import pifit64 as a64
    from guardx_amd import fisher, pifit
    if not torch.cuda.is_available():
        raise SystemExit("ab_pifit: no GPU; there is nothing to time without one")
    dev = torch.device("cuda:0")
    B, D, A, iters, clip = args.B, args.D, args.A, args.iters, a64.CLIP
    pi0 = f64.make_actor(D, A)
    batch = l64.batch_of(pi0, torch.randn(B, D, generator=torch.Generator().manual_seed(1)), seed=1, adc=False)
    keys = ("obs", "act", "adv", "logp")
    data = {k: torch.from_numpy(np.array(batch[k])).to(dev) for k in keys}
    theta0 = fisher.flat_params(pi0).numpy().astype(np.float64)

    def theirs_ready():
        pi = copy.deepcopy(pi0).to(dev)
        return pi, torch.optim.Adam(pi.parameters(), lr=a64.LR)

    def theirs(state, d, target_kl):
        pi, opt = state
        obs, act, adv, logp_old = d['obs'], d['act'], d['adv'], d['logp']
        for i in range(iters):
            opt.zero_grad()
            dist = Normal(pi.mu_net(obs), torch.exp(pi.log_std))
            logp = dist.log_prob(act).sum(axis=-1)
            ratio = torch.exp(logp - logp_old)
            loss_pi = -(torch.min(ratio * adv, torch.clamp(ratio, 1 - clip, 1 + clip) * adv)).mean()
            kl = (logp_old - logp).mean().item()
            dist.entropy().mean().item()
            torch.as_tensor(ratio.gt(1 + clip) | ratio.lt(1 - clip), dtype=torch.float32).mean().item()
            if kl > target_kl:
                break
            loss_pi.backward()
            opt.step()
        return i, kl

    def ours_ready():
        return pifit.PolicyFit(copy.deepcopy(pi0).to(dev), lr=a64.LR)

    def ours(PF, d, target_kl):
        info = PF.fit(d, iters=iters, target_kl=target_kl, clip_ratio=clip)
        return info['stop_iter'], info['kl_last']

    def wall_us(ready, fn, d, target_kl):
        state = ready()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(state, d, target_kl)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6, state, out

    def ab(d, target_kl):
        for _ in range(args.warmup):
            wall_us(ours_ready, ours, d, target_kl)
            wall_us(theirs_ready, theirs, d, target_kl)
        ta, tb = [], []
        for _ in range(args.reps):
            ta.append(wall_us(ours_ready, ours, d, target_kl))
            tb.append(wall_us(theirs_ready, theirs, d, target_kl))
        return ta, tb

    med = statistics.median
    r1 = lambda x: round(x, 1)      # noqa: E731

    def report(ta, tb):
        t_ours, t_theirs = [t[0] for t in ta], [t[0] for t in tb]
        return dict(fit_us=r1(med(t_ours)), fit_us_min_max=[r1(min(t_ours)), r1(max(t_ours))],
                    learners_loop_us=r1(med(t_theirs)), learners_loop_us_min_max=[r1(min(t_theirs)), r1(max(t_theirs))],
                    speedup=round(med(t_theirs) / med(t_ours), 2),
                    ranges_overlap=bool(max(t_ours) >= min(t_theirs) and max(t_theirs) >= min(t_ours)),
                    stop_iter=int(ta[-1][2][0]), learners_stop_iter=int(tb[-1][2][0]),
                    kl_last=float(ta[-1][2][1]), learners_kl_last=float(tb[-1][2][1]))

    never = 1e9
    PF = ours_ready()
    kl = PF.fit(data, iters=iters, target_kl=never, clip_ratio=clip)['kl'].cpu().numpy()
    j = max(1, int(np.argmax(kl[:min(args.stop_at, iters - 1) + 1])))      # kl need not rise all the way: the largest entry up to --stop-at
    early = 0.5 * (float(kl[:j].max()) + float(kl[j]))
    res_never = report(*ab(data, never))
    res_early = report(*ab(data, early))
    res_never.update(fit_us_per_iteration=r1(res_never["fit_us"] / iters), learners_us_per_iteration=r1(res_never["learners_loop_us"] / iters))
    # the launches' floor: the same call over one row
    one = {k: v[:1].contiguous() for k, v in data.items()}
    floor = [wall_us(ours_ready, ours, one, never)[0] for _ in range(args.warmup + args.reps)][args.warmup:]
    # both displacements against float64 on a subsample
    n = min(args.sub, B)
    sub = {k: v[:n].contiguous() for k, v in data.items()}
    sub_h = {k: np.array(batch[k][:n]) for k in keys}
    _, PFs, _ = wall_us(ours_ready, ours, sub, never)
    _, (ps, _), _ = wall_us(theirs_ready, theirs, sub, never)
    want = a64.fit64(theta0, sub_h, iters, None, clip)["theta"] - theta0
    d_ours = fisher.flat_params(PFs.pi).cpu().numpy().astype(np.float64) - theta0
    d_theirs = fisher.flat_params(ps).cpu().numpy().astype(np.float64) - theta0
    res = dict(tool="ab_pifit", device=torch.cuda.get_device_name(0), B=B, D=D, A=A, P=PF.P, iters=iters, reps=args.reps,
               warmup=args.warmup, lr=a64.LR, clip_ratio=clip, workgroups=int(PF._lib.gxa_default_workgroups(B)), launches=2 * iters,
               never_stops=res_never, stops_early=dict(res_early, target_kl=early, stop_at=j),
               one_row_fit_us=r1(med(floor)), launch_share=round(med(floor) / res_never["fit_us"], 3),
               sub_rows=n, sub_displacement_rel_l2=f64.rel_l2(d_ours, want), sub_learners_displacement_rel_l2=f64.rel_l2(d_theirs, want))
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
