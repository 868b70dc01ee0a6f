"""A/B of the update's closing block, the fit of the value critic: guardx_amd.vfit (libguardx_vfit.so) against the learners' own
loop.

    python tools/ab_vfit.py [--B 400000] [--D 43] [--iters 80] [--reps 7] [--warmup 2] [--out profiles/ab_vfit.json]

Point's critic (43 -> 64 -> 64 -> 1, tanh) over B = env_num x T = 2000 x 200 rows, seeded inputs, ret = 1 + 2 N(0, 1),
lr = 1e-3.
  theirs   the loop of trpo.py:434-439 in torch on the same device: zero_grad, the loss, backward, Adam's step, --iters times.
  ours     ValueFit.fit(obs, ret, iters).
Both start from equal state (a fresh copy of the critic and a new optimizer, made before the clock starts).  A host clock
around each, ended by a device synchronise, the two alternating, the median of --reps after --warmup with min .. max.  Also:
one gradient by HIP events (the two launches and the packing of the parameters), GFLOP and TFLOP/s by the closed form's shapes
(2 B (128 D + 3 x 4096 + 128) per gradient); the floor that the 2 iters launches set, as the same call over a batch of one
row, where the kernels have next to nothing to do (the fit has no early flag for its launches to skip on, so this stands in
for the line search's no-op launches); both sides' final loss; and, on a subsample of 4099 rows, the relative L2 of both
sides' displacement theta_iters - theta_0 against tests/vfit64.py:fit64.
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
    ap.add_argument("--iters", type=int, default=80)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sub", type=int, default=4099)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import vfit64 as v64
    from guardx_amd import vfit
    if not torch.cuda.is_available():
        raise SystemExit("ab_vfit: no GPU; there is nothing to time without one")
    dev = torch.device("cuda:0")
    B, D, iters = args.B, args.D, args.iters
    critic0 = v64.make_critic(D, 64, seed=0)
    gen = torch.Generator().manual_seed(1)
    obs_h = torch.randn(B, D, generator=gen)
    ret_h = (1.0 + 2.0 * torch.randn(B, generator=gen)).contiguous()
    obs, ret = obs_h.to(dev), ret_h.to(dev)
    theta0 = v64.flat(critic0).numpy().astype(np.float64)

    def theirs_ready():
        critic = copy.deepcopy(critic0).to(dev)
        return critic, torch.optim.Adam(critic.parameters(), lr=v64.LR)

    def theirs(state, o, r):
        critic, opt = state
        for _ in range(iters):
            opt.zero_grad()
            loss_v = ((critic(o) - r) ** 2).mean()
            loss_v.backward()
            opt.step()
        return loss_v.detach()

    def ours_ready():
        return vfit.ValueFit(copy.deepcopy(critic0).to(dev), lr=v64.LR)

    def ours(VF, o, r):
        return VF.fit(o, r, iters=iters)['loss'][-1]

    def wall_us(ready, fn, o, r):
        state = ready()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(state, o, r)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6, state, out

    def ab(o, r):
        for _ in range(args.warmup):
            wall_us(ours_ready, ours, o, r)
            wall_us(theirs_ready, theirs, o, r)
        ta, tb = [], []
        for _ in range(args.reps):
            ta.append(wall_us(ours_ready, ours, o, r))
            tb.append(wall_us(theirs_ready, theirs, o, r))
        return ta, tb

    med = statistics.median
    ta, tb = ab(obs, ret)
    t_ours, t_theirs = [t[0] for t in ta], [t[0] for t in tb]
    # one gradient by events
    VF = ours_ready()
    VF.gradient(obs, ret)
    ev_ms = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        VF.gradient(obs, ret)
        e1.record()
        e1.synchronize()
        ev_ms.append(e0.elapsed_time(e1))
    gflop = 2.0 * B * (128 * D + 3 * 4096 + 128) / 1e9
    # the launches' floor: the same call over one row
    floor = [wall_us(ours_ready, ours, obs[:1], ret[:1])[0] for _ in range(args.warmup + args.reps)][args.warmup:]
    # both displacements against float64 on a subsample
    n = min(args.sub, B)
    so, sr = obs[:n].contiguous(), ret[:n].contiguous()
    _, VFs, _ = wall_us(ours_ready, ours, so, sr)
    _, (cs, _), _ = wall_us(theirs_ready, theirs, so, sr)
    want = v64.fit64(theta0, obs_h[:n].numpy(), ret_h[:n].numpy(), iters)[0][-1] - theta0
    d_ours = v64.flat(VFs.critic).cpu().numpy().astype(np.float64) - theta0
    d_theirs = v64.flat(cs).cpu().numpy().astype(np.float64) - theta0
    res = dict(tool="ab_vfit", device=torch.cuda.get_device_name(0), B=B, D=D, P=VF.P, iters=iters, reps=args.reps, warmup=args.warmup,
               lr=v64.LR, workgroups=int(VF._lib.gxv_default_workgroups(B)),
               fit_us=round(med(t_ours), 1), fit_us_min_max=[round(min(t_ours), 1), round(max(t_ours), 1)],
               learners_loop_us=round(med(t_theirs), 1), learners_loop_us_min_max=[round(min(t_theirs), 1), round(max(t_theirs), 1)],
               speedup=round(med(t_theirs) / med(t_ours), 2), ranges_overlap=bool(max(t_ours) >= min(t_theirs)),
               fit_us_per_iteration=round(med(t_ours) / iters, 1), learners_us_per_iteration=round(med(t_theirs) / iters, 1),
               gradient_event_us=round(med(ev_ms) * 1e3, 1), gradient_event_us_min_max=[round(min(ev_ms) * 1e3, 1), round(max(ev_ms) * 1e3, 1)],
               gradient_gflop=round(gflop, 2), gradient_tflops=round(gflop / med(ev_ms), 2),
               launches=2 * iters, one_row_fit_us=round(med(floor), 1), launch_share=round(med(floor) / med(t_ours), 3),
               final_loss=float(ta[-1][2]), learners_final_loss=float(tb[-1][2]),
               sub_rows=n, sub_displacement_rel_l2=v64.rel_l2(d_ours, want), sub_learners_displacement_rel_l2=v64.rel_l2(d_theirs, want))
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
