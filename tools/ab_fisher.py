"""A/B of the trust-region step's linear algebra: guardx_amd.fisher (libguardx_fisher.so) against the learners' own method.

    python tools/ab_fisher.py [--B 400000] [--D 43] [--A 2] [--iters 100] [--reps 10] [--warmup 3] [--no-check64]
                               [--out profiles/ab_fisher.json]

Point's actor (43 -> 64 -> 64 -> 2, tanh) over B = env_num x T = 2000 x 200 rows, seeded inputs.
  product  F(x) against the double backward through autograd (auto_hession_x of the learners' KL), both with device
           tensors in and out; HIP events around each call, the two alternating, the median of --reps after --warmup.
  solve    F.solve(g, iters) against the loop the learners run: numpy cg over that double backward, with the
           .cpu().numpy() of every product and the FloatTensor(x).to(device) of every direction, and the closing product
           for s; a host clock around each, ended by a device synchronise (the device solve is synchronised by reading s).
Also what the product costs by the shapes: FLOPs (2 per multiply-add of the closed form) and the bytes of obs, over its time.
One JSON line on stdout and, with --out, in that file.  Needs a GPU: there is no CPU path to time.
"""
import argparse
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-check64", dest="check64", action="store_false")
    args = ap.parse_args()
    import numpy as np
    import torch
    import fisher64 as f64
    from guardx_amd import fisher
    if not torch.cuda.is_available():
        raise SystemExit("ab_fisher: no GPU; there is nothing to time without one")
    dev = torch.device("cuda:0")
    B, D, A = args.B, args.D, args.A
    pi = f64.make_actor(D, A, 64, seed=0).to(dev)
    gen = torch.Generator().manual_seed(1)
    obs = torch.randn(B, D, generator=gen).to(dev)
    P = fisher.param_count(D, A)
    x = torch.randn(P, generator=gen).to(dev)
    g = torch.randn(P, generator=gen).to(dev)
    F = fisher.FisherOperator(pi, obs)

    def event_us(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    def wall_us(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    def ab(clock, fa, fb, reps, warmup):
        for _ in range(warmup):
            fa()
            fb()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(reps):
            ta.append(clock(fa))
            tb.append(clock(fb))
        return ta, tb

    # ---- one product
    ours = lambda: F(x)                                         # noqa: E731
    theirs = lambda: f64.autograd_fvp(pi, obs, x)               # noqa: E731
    y, y_ref = ours(), theirs()
    agree = float((y - y_ref).norm() / y_ref.norm())
    # both against float64 at the timed size (numpy on the host; --no-check64 skips the few seconds it takes)
    err_ours = err_theirs = None
    if args.check64:
        want = f64.fvp64(f64.flat(pi).cpu().numpy(), x.cpu().numpy(), obs.cpu().numpy(), A, 64)
        err_ours, err_theirs = f64.rel_l2(y.cpu().numpy(), want), f64.rel_l2(y_ref.cpu().numpy(), want)
    t_ours, t_theirs = ab(event_us, ours, theirs, args.reps, args.warmup)

    # ---- the solve and s
    def solve_ours():
        x_hat, s, info = F.solve(g, iters=args.iters)
        return x_hat, float(s)                                  # the learner reads s: one synchronisation

    def solve_theirs():
        Hx = lambda v: f64.autograd_fvp(pi, obs, torch.FloatTensor(v).to(dev)).cpu().numpy()    # noqa: E731
        x_hat = f64.learners_cg32(Hx, g.cpu().numpy(), args.iters)
        return x_hat, float(x_hat.T @ Hx(x_hat))

    solve_reps = max(2, args.reps // 3)
    s_ours, s_theirs = ab(wall_us, solve_ours, solve_theirs, solve_reps, 1)
    (xo, so), (xt, st) = solve_ours(), solve_theirs()
    gn = g.cpu().numpy().astype(np.float64)

    def residual(v):
        hv = F(torch.from_numpy(np.asarray(v, dtype=np.float32)).to(dev)).cpu().numpy().astype(np.float64)
        return float(np.linalg.norm(hv - gn) / np.linalg.norm(gn))

    med = statistics.median
    flop = 2.0 * B * (2 * 64 * D + 3 * 64 * 64 + 2 * 64 * A + 64 * A + 64 * A + 2 * 64 * 64 + 64 * D)
    res = dict(tool="ab_fisher", device=torch.cuda.get_device_name(0), B=B, D=D, A=A, P=P, iters=args.iters, reps=args.reps,
               warmup=args.warmup, workgroups=int(F._lib.gxf_default_workgroups(B)),
               product_us=round(med(t_ours), 1), product_us_min_max=[round(min(t_ours), 1), round(max(t_ours), 1)],
               autograd_product_us=round(med(t_theirs), 1),
               autograd_product_us_min_max=[round(min(t_theirs), 1), round(max(t_theirs), 1)],
               product_speedup=round(med(t_theirs) / med(t_ours), 2), product_vs_autograd_rel_l2=agree,
               product_rel_l2_vs_float64=err_ours, autograd_product_rel_l2_vs_float64=err_theirs,
               product_gflop=round(flop / 1e9, 2), product_tflops=round(flop / med(t_ours) / 1e6, 2),
               obs_gb_per_s=round(4.0 * B * D / med(t_ours) / 1e3, 1),
               solve_us=round(med(s_ours), 1), solve_us_min_max=[round(min(s_ours), 1), round(max(s_ours), 1)],
               learners_loop_us=round(med(s_theirs), 1),
               learners_loop_us_min_max=[round(min(s_theirs), 1), round(max(s_theirs), 1)], solve_reps=solve_reps,
               solve_speedup=round(med(s_theirs) / med(s_ours), 2), s=so, learners_s=st,
               solve_residual=residual(xo.cpu().numpy()), learners_residual=residual(xt))
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
