"""A/B of the safety critics' fit: guardx_amd.cfit (libguardx_cfit.so) against the learners' own loops in torch on the same
device.

    python tools/ab_cfit.py [--B 400000] [--iters 80] [--reps 10] [--warmup 3] [--out profiles/ab_cfit.json]

B = env_num x T = 2000 x 200 rows, seeded inputs, lr = 1e-3, nine targets in ten exactly 0.
  1  usl's fit, Din = 45 (Point's 43 observations and 2 actions), head 'softplus', no weights.
       theirs   usl.py:449-454 over usl.py:378-383: zero_grad, cat(obs, act_safe), the loss, backward, Adam's step, --iters times.
       ours     CostCriticFit.fit(cat(obs, act_safe), targetc, iters).
     Both by device events around the whole fit (neither synchronises).
  2  safelayer's fit, D = 43, A = 2, head 'dot', down-sampled.
       theirs   safelayer.py:483-488 over 384-418 as written: boolean indexing and a host choice per round.  It synchronises
                every round, so it is timed by the wall clock, ended by a device synchronise.
       ours     downsample_weights(cost, iters) and CostCriticFit.fit(obs, cost, iters, weight=, act=act_safe, offset=prev_cost),
                by the same wall clock (and by events).
  3  downsample_weights alone, by events.
Each pair alternates; the median of --reps after --warmup with min .. max.  Both sides start every repetition from equal state
(a fresh copy of the module and a new optimizer, made before the clock starts).  Also one gradient of each head by events, to
set beside profiles/ab_vfit.json's gradient_event_us at the same B.
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
    ap.add_argument("--iters", type=int, default=80)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    import cfit64 as c64
    from guardx_amd import cfit
    if not torch.cuda.is_available():
        raise SystemExit("ab_cfit: no GPU; there is nothing to time without one")
    dev = torch.device("cuda:0")
    B, iters, D, A = args.B, args.iters, 43, 2
    gen = torch.Generator().manual_seed(1)
    obs = torch.randn(B, D, generator=gen).to(dev)
    act_safe = torch.randn(B, A, generator=gen).clamp(-1, 1).to(dev)
    prev_cost = (torch.rand(B, generator=gen) < 0.1).float().to(dev)
    cost = torch.where(torch.rand(B, generator=gen) < 0.9, torch.zeros(()), torch.rand(B, generator=gen) + 0.5).contiguous().to(dev)
    q0, g0 = c64.make_module("softplus", D + A, seed=0), c64.make_module("dot", D, A, seed=0)
    med = statistics.median

    def event_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3, out

    def wall_us(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6, out

    def alternate(clock, ours_ready, ours, theirs_ready, theirs):
        ta, tb, la, lb = [], [], None, None
        for i in range(args.warmup + args.reps):
            sa = ours_ready()
            a, la = clock(lambda: ours(sa))
            sb = theirs_ready()
            b, lb = clock(lambda: theirs(sb))
            if i >= args.warmup:
                ta.append(a)
                tb.append(b)
        return ta, tb, float(la), float(lb)

    # ---- 1: usl
    def usl_theirs_ready():
        m = copy.deepcopy(q0).to(dev)
        return m, torch.optim.Adam(m.parameters(), lr=c64.LR)

    def usl_theirs(state):
        m, opt = state
        for _ in range(iters):
            opt.zero_grad()
            obs_act = torch.cat((obs, act_safe), dim=1)
            loss = ((m(obs_act) - cost) ** 2).mean()
            loss.backward()
            opt.step()
        return loss.detach()

    def usl_ours(QF):
        return QF.fit(torch.cat((obs, act_safe), dim=1), cost, iters=iters)['loss'][-1]

    u_ours, u_theirs, ul_a, ul_b = alternate(event_us, lambda: cfit.CostCriticFit(copy.deepcopy(q0).to(dev), lr=c64.LR), usl_ours,
                                             usl_theirs_ready, usl_theirs)

    # ---- 2: safelayer
    def sl_theirs_ready():
        m = copy.deepcopy(g0).to(dev)
        return m, torch.optim.Adam(m.parameters(), lr=c64.LR), np.random.RandomState(0)

    def sl_theirs(state):
        m, opt, downsample_rand = state
        for _ in range(iters):
            opt.zero_grad()
            target_c = cost
            current_c = m(obs, act_safe) + prev_cost
            target_c_zero, current_c_zero = target_c[target_c == 0], current_c[target_c == 0]
            target_c_positive, current_c_positive = target_c[target_c > 0], current_c[target_c > 0]
            frac = len(target_c_positive) / len(target_c_zero) if len(target_c_zero) != 0 else 1.0
            if frac < 1.0:
                indices = downsample_rand.choice(len(target_c_zero), size=int(len(target_c_zero) * frac), replace=False)
                current = torch.cat((current_c_positive, current_c_zero[indices]), dim=0)
                target = torch.cat((target_c_positive, target_c_zero[indices]), dim=0)
            else:
                current, target = current_c, target_c
            loss = F.mse_loss(current, target)
            loss.backward()
            opt.step()
        return loss.detach()

    def sl_ours(QF):
        w = cfit.downsample_weights(cost, iters)
        return QF.fit(obs, cost, iters=iters, weight=w, act=act_safe, offset=prev_cost)['loss'][-1]

    sl_ready = lambda: cfit.CostCriticFit(copy.deepcopy(g0).to(dev), lr=c64.LR)    # noqa: E731
    s_ours, s_theirs, sl_a, sl_b = alternate(wall_us, sl_ready, sl_ours, sl_theirs_ready, sl_theirs)
    s_ours_ev = [event_us(lambda: sl_ours(QF))[0] for QF in [sl_ready() for _ in range(args.reps)]]

    # ---- 3: downsample_weights alone; one gradient of each head
    ds = [event_us(lambda: cfit.downsample_weights(cost, iters))[0] for _ in range(args.warmup + args.reps)][args.warmup:]
    QFu, QFs = cfit.CostCriticFit(copy.deepcopy(q0).to(dev), lr=c64.LR), sl_ready()
    xu = torch.cat((obs, act_safe), dim=1)
    w1 = cfit.downsample_weights(cost, 1)[0].contiguous()
    grads = {}
    for name, fn in (("softplus", lambda: QFu.gradient(xu, cost)), ("softplus_masked", lambda: QFu.gradient(xu, cost, weight=w1)),
                     ("dot", lambda: QFs.gradient(obs, cost, act=act_safe, offset=prev_cost)),
                     ("dot_masked", lambda: QFs.gradient(obs, cost, weight=w1, act=act_safe, offset=prev_cost))):
        t = [event_us(fn)[0] for _ in range(args.warmup + args.reps)][args.warmup:]
        grads[name] = [round(med(t), 1), round(min(t), 1), round(max(t), 1)]

    r = lambda v: round(v, 1)    # noqa: E731
    mm = lambda t: [r(min(t)), r(max(t))]    # noqa: E731
    res = dict(tool="ab_cfit", device=torch.cuda.get_device_name(0), B=B, iters=iters, reps=args.reps, warmup=args.warmup, lr=c64.LR,
               zero_share=float((cost == 0).float().mean()),
               usl=dict(Din=D + A, clock="device events", fit_us=r(med(u_ours)), fit_us_min_max=mm(u_ours),
                        learners_loop_us=r(med(u_theirs)), learners_loop_us_min_max=mm(u_theirs),
                        speedup=round(med(u_theirs) / med(u_ours), 2), ranges_overlap=bool(max(u_ours) >= min(u_theirs)),
                        fit_us_per_iteration=r(med(u_ours) / iters), final_loss=ul_a, learners_final_loss=ul_b),
               safelayer=dict(D=D, A=A, clock="wall, ended by a synchronise", fit_us=r(med(s_ours)), fit_us_min_max=mm(s_ours),
                              fit_event_us=r(med(s_ours_ev)), fit_event_us_min_max=mm(s_ours_ev),
                              learners_loop_us=r(med(s_theirs)), learners_loop_us_min_max=mm(s_theirs),
                              speedup=round(med(s_theirs) / med(s_ours), 2), ranges_overlap=bool(max(s_ours) >= min(s_theirs)),
                              fit_us_per_iteration=r(med(s_ours) / iters), final_loss=sl_a, learners_final_loss=sl_b),
               downsample_weights_us=r(med(ds)), downsample_weights_us_min_max=mm(ds),
               gradient_event_us_med_min_max=grads)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
