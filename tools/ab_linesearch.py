"""A/B of the trust-region step's line search: guardx_amd.linesearch (libguardx_linesearch.so) against the learners' own loop.

    python tools/ab_linesearch.py [--B 400000] [--D 43] [--A 2] [--iters 100] [--reps 7] [--warmup 2]
                                   [--out profiles/ab_linesearch.json]

Point's actor (43 -> 64 -> 64 -> 2, tanh) over B = env_num x T = 2000 x 200 rows, seeded inputs, target_kl = 0.01.
  theirs   the loop of trpo.py:406-431 in torch on the same device: a deep copy of the actor, then per candidate the flat
           parameters fetched to the host, theta - 0.8**j x_direction in numpy, the assignment back into the copy, the KL
           forward, the loss forward, and the two .item()s; on acceptance the assignment into the actor and the loss once more.
  ours     LineSearch.search(x_direction, target_kl, iters) and assign_flat_params, ended by reading `accepted`.
Two directions along the loss gradient: KL(t = 1) = target / 2 (accepted at j = 0) and 5 target (accepted at j = 4).  A host
clock around each, ended by a device synchronise, the two alternating, the median of --reps after --warmup.  Also the cost of
the launches that follow an acceptance: the j = 0 case with iters = 100 against the same with iters = 1.
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
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--target-kl", type=float, default=0.01)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from torch.distributions.normal import Normal
    import fisher64 as f64
    from guardx_amd import fisher, linesearch
    if not torch.cuda.is_available():
        raise SystemExit("ab_linesearch: no GPU; there is nothing to time without one")
    dev = torch.device("cuda:0")
    B, D, A, target = args.B, args.D, args.A, args.target_kl
    pi = f64.make_actor(D, A, 64, seed=0).to(dev)
    gen = torch.Generator().manual_seed(1)
    obs = torch.randn(B, D, generator=gen).to(dev)
    noise, adv = torch.randn(B, A, generator=gen).to(dev), torch.randn(B, generator=gen).to(dev)
    with torch.no_grad():
        mu = pi.mu_net(obs)
        std = torch.exp(pi.log_std)
        act = mu + std * noise
        logp = Normal(mu, std).log_prob(act).sum(axis=-1)
        logstd = pi.log_std.detach().reshape(1, A).expand(B, A).contiguous()
    adv = (adv - adv.mean()) / adv.std()
    data = dict(obs=obs, act=act, adv=adv, logp=logp, mu=mu, logstd=logstd)

    # ---- the learners' functions (trpo.py:341-372), on the device
    def compute_kl_pi(cur_pi):
        return f64.mean_kl(mu, logstd, cur_pi.mu_net(obs), cur_pi.log_std)

    def compute_loss_pi(cur_pi):
        lp = Normal(cur_pi.mu_net(obs), torch.exp(cur_pi.log_std)).log_prob(act).sum(axis=-1)
        return -(torch.exp(lp - logp) * adv).mean()

    def get_flat(net):
        return torch.cat([p.data.view(-1) for p in net.parameters()]).cpu().numpy()

    def assign_flat(flat, net):
        at = 0
        for p in net.parameters():
            n = p.numel()
            p.data.copy_(torch.tensor(flat[at:at + n], dtype=torch.float32).view_as(p).to(dev))
            at += n

    g = torch.cat([x.reshape(-1) for x in torch.autograd.grad(compute_loss_pi(pi), list(pi.parameters()))]).detach()
    LS = linesearch.LineSearch(pi, data)

    def direction(kl_goal):
        d = g.clone()
        for _ in range(3):
            kl = float(LS.evaluate(d, [1.0])[0, 0])
            d = d * (kl_goal / kl) ** 0.5
        return d.contiguous()

    def theirs(d_np, iters):
        work = copy.deepcopy(pi)                                   # stands for ac.pi: the accepted parameters go here
        with torch.no_grad():
            pi_l_old = compute_loss_pi(work).item()
            actor_tmp = copy.deepcopy(work)
            for j in range(iters):
                assign_flat(get_flat(work) - 0.8 ** j * d_np, actor_tmp)
                kl, pi_l = compute_kl_pi(actor_tmp), compute_loss_pi(actor_tmp)
                if kl.item() <= target and pi_l.item() <= pi_l_old:
                    assign_flat(get_flat(work) - 0.8 ** j * d_np, work)
                    compute_loss_pi(work)
                    return j, work
        return -1, work

    def ours(d, iters):
        work = copy.deepcopy(pi)
        theta_new, info = LS.search(d, target, iters=iters)         # LS reads pi, whose parameters work starts from
        linesearch.assign_flat_params(work, theta_new)
        return int(info['accepted']), work

    def wall_us(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    def ab(fa, fb):
        for _ in range(args.warmup):
            fa()
            fb()
        ta, tb = [], []
        for _ in range(args.reps):
            ta.append(wall_us(fa))
            tb.append(wall_us(fb))
        return ta, tb

    med = statistics.median
    res = dict(tool="ab_linesearch", device=torch.cuda.get_device_name(0), B=B, D=D, A=A, P=LS.P, iters=args.iters, reps=args.reps,
               warmup=args.warmup, target_kl=target, workgroups=int(LS._lib.gxb_default_workgroups(B, D)))
    for name, goal in (("j0", 0.5 * target), ("j4", 5.0 * target)):
        d = direction(goal)
        d_np = d.cpu().numpy().astype(np.float64)                  # the learners' x_direction is a float64 numpy vector
        (jo, wo), (jt, wt) = ours(d, args.iters), theirs(d_np, args.iters)
        agree = float((fisher.flat_params(wo) - fisher.flat_params(wt)).abs().max())
        t_ours, t_theirs = ab(lambda: ours(d, args.iters), lambda: theirs(d_np, args.iters))
        res.update({f"{name}_accepted": jo, f"{name}_learners_accepted": jt, f"{name}_max_abs_param_difference": agree,
                    f"{name}_search_us": round(med(t_ours), 1), f"{name}_search_us_min_max": [round(min(t_ours), 1), round(max(t_ours), 1)],
                    f"{name}_learners_loop_us": round(med(t_theirs), 1),
                    f"{name}_learners_loop_us_min_max": [round(min(t_theirs), 1), round(max(t_theirs), 1)],
                    f"{name}_speedup": round(med(t_theirs) / med(t_ours), 2)})
        if name == "j0":
            t_full, t_one = ab(lambda: ours(d, args.iters), lambda: ours(d, 1))
            res.update(j0_search_iters_1_us=round(med(t_one), 1),
                       noop_launches=2 * (args.iters - 1), noop_launches_us=round(med(t_full) - med(t_one), 1))
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
