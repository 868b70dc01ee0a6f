"""A/B of what opens the update, the surrogate gradients: guardx_amd.pgrad (libguardx_pgrad.so) against the learners' own
auto_grad.

    python tools/ab_pgrad.py [--B 400000] [--D 43] [--A 2] [--reps 10] [--warmup 3] [--out profiles/ab_pgrad.json]

Point's actor (43 -> 64 -> 64 -> 2, tanh, a free log_std) over B = env_num x T = 2000 x 200 rows, seeded inputs, adv
standardised, adc centred.
  theirs   auto_grad as the learners call it, in torch on the same device: the forward over all rows (Normal.log_prob, ratio,
           the loss) and torch.autograd.grad(..., create_graph=True), flattened: once for g (trpo), and twice with two forward
           passes for g and b (cpo.py:437-446).
  ours     SurrogateGradient.gradient(), without and with adc.
Device events around each call, the four alternating, the median of --reps after --warmup with min .. max.  Also: GFLOP and
TFLOP/s by the closed form's shapes (2 B (128 D + 3 x 4096 + 3 x 64 A + 128) for one gradient; the second adds the backward,
2 B (64 D + 2 x 4096 + 2 x 64 A + 128)); cpo_direction's ladder kernel by itself on supplied vectors; the relative L2 of
both sides' g and b against tests/pgrad64.py:grad64 on a subsample; and, read from profiles/ab_vfit.json, gxv_gradient's time
at the same B for comparison.
One JSON line on stdout and, with --out, in that file.  Needs a GPU: there is no CPU path to time.
"""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=400000)
    ap.add_argument("--D", type=int, default=43)
    ap.add_argument("--A", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sub", type=int, default=4099)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from torch.distributions.normal import Normal
    import fisher64 as f64
    import linesearch64 as l64
    import pgrad64 as p64
    from guardx_amd import pgrad
    if not torch.cuda.is_available():
        raise SystemExit("ab_pgrad: no GPU; there is nothing to time without one")
    dev = torch.device("cuda:0")
    B, D, A = args.B, args.D, args.A
    pi0 = f64.make_actor(D, A, 64, seed=0)
    obs_h = torch.randn(B, D, generator=torch.Generator().manual_seed(1))
    batch = l64.batch_of(pi0, obs_h, seed=0)
    data = {k: torch.from_numpy(np.array(v)).to(dev) for k, v in batch.items() if k in ("obs", "act", "adv", "logp", "adc")}
    pi = copy.deepcopy(pi0).to(dev)
    theta = f64.flat(pi0).numpy()

    def auto_grad(loss, actor):
        """the learners' flat gradient, in their way: autograd over the actor's parameters with the graph of the gradient
        kept (create_graph, which their Hessian product needs and the gradient itself does not), joined into one vector"""
        parts = torch.autograd.grad(loss, list(actor.parameters()), create_graph=True)
        return torch.cat([p.reshape(-1) for p in parts])

    def ratio():
        logp = Normal(pi.mu_net(data["obs"]), torch.exp(pi.log_std)).log_prob(data["act"]).sum(axis=-1)
        return torch.exp(logp - data["logp"])

    def theirs_g():
        return auto_grad(-(ratio() * data["adv"]).mean(), pi).detach(), None

    def theirs_gb():
        loss_pi = -(ratio() * data["adv"]).mean()
        surr_cost = (ratio() * data["adc"]).mean()
        return auto_grad(loss_pi, pi).detach(), auto_grad(surr_cost, pi).detach()

    S1 = pgrad.SurrogateGradient(pi, {k: v for k, v in data.items() if k != "adc"})
    S2 = pgrad.SurrogateGradient(pi, data)
    calls = dict(ours_g=lambda: S1.gradient()[:2], ours_gb=lambda: S2.gradient()[:2], theirs_g=theirs_g, theirs_gb=theirs_gb)

    def event_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3, out

    times = {k: [] for k in calls}
    for i in range(args.warmup + args.reps):
        for k, fn in calls.items():                            # alternating
            t, _ = event_us(fn)
            if i >= args.warmup:
                times[k].append(t)
    med = statistics.median
    stat = lambda k: (round(med(times[k]), 1), [round(min(times[k]), 1), round(max(times[k]), 1)])     # noqa: E731

    # the ladder kernel by itself, on supplied vectors (case 2 of tests/pgrad64.py at this actor's P)
    P = S2.P
    rng = np.random.default_rng(0)
    vec = lambda: torch.from_numpy(rng.standard_normal(P).astype(np.float32)).to(dev)      # noqa: E731
    b_, hg, hb, ag = vec(), vec(), vec(), vec()
    s_ = torch.tensor([float(P)], dtype=torch.float32, device=dev)
    c_, tkl = torch.tensor(-0.01, dtype=torch.float64, device=dev), torch.tensor(0.01, dtype=torch.float64, device=dev)
    ladder = []
    for i in range(args.warmup + args.reps):
        t, _ = event_us(lambda: pgrad._direction_from(b_, hg, hb, ag, s_, c_, tkl))
        if i >= args.warmup:
            ladder.append(t)

    # both sides against float64 on a subsample
    n = min(args.sub, B)
    sub = {k: (np.array(v[:n]) if v is not None else None) for k, v in batch.items()}
    if n > 1:
        sub["adv"] = ((sub["adv"] - sub["adv"].mean()) / sub["adv"].std()).astype(np.float32)
        sub["adc"] = (sub["adc"] - sub["adc"].mean()).astype(np.float32)
    sdev = {k: torch.from_numpy(sub[k]).to(dev) for k in ("obs", "act", "adv", "logp", "adc")}
    g_o, b_o, _ = pgrad.SurrogateGradient(pi, sdev).gradient()
    data_full, data = data, sdev
    g_t, b_t = theirs_gb()
    data = data_full
    want_g, want_b = p64.grad64(theta, sub)[0], p64.grad64(theta, sub, cost=True)[0]
    rel = lambda got, want: f64.rel_l2(got.cpu().numpy().astype(np.float64), want)         # noqa: E731

    fwd = 2.0 * B * (64 * D + 4096 + 64 * A)
    bwd = 2.0 * B * (64 * D + 2 * 4096 + 2 * 64 * A + 128)
    vfit_us = None
    try:
        with open(os.path.join(ROOT, "profiles", "ab_vfit.json")) as f:
            rec = json.loads(f.readline())
        if rec.get("B") == B and rec.get("D") == D:
            vfit_us = rec.get("gradient_event_us")
    except (OSError, ValueError):
        pass
    res = dict(tool="ab_pgrad", device=torch.cuda.get_device_name(0), B=B, D=D, A=A, P=P, reps=args.reps, warmup=args.warmup,
               workgroups=int(S2._lib.gxg_default_workgroups(B)))
    for k in calls:
        res[k + "_us"], res[k + "_us_min_max"] = stat(k)
    res.update(speedup_g=round(med(times["theirs_g"]) / med(times["ours_g"]), 2),
               speedup_gb=round(med(times["theirs_gb"]) / med(times["ours_gb"]), 2),
               gb_over_g=round(med(times["ours_gb"]) / med(times["ours_g"]), 3),
               g_gflop=round((fwd + bwd) / 1e9, 2), g_tflops=round((fwd + bwd) / 1e6 / med(times["ours_g"]), 2),
               gb_gflop=round((fwd + 2 * bwd) / 1e9, 2), gb_tflops=round((fwd + 2 * bwd) / 1e6 / med(times["ours_gb"]), 2),
               vfit_gradient_event_us=vfit_us, g_over_vfit_gradient=round(med(times["ours_g"]) / vfit_us, 3) if vfit_us else None,
               ladder_us=round(med(ladder), 1), ladder_us_min_max=[round(min(ladder), 1), round(max(ladder), 1)],
               sub_rows=n, sub_g_rel_l2=rel(g_o, want_g), sub_b_rel_l2=rel(b_o, want_b),
               sub_learners_g_rel_l2=rel(g_t, want_g), sub_learners_b_rel_l2=rel(b_t, want_b))
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
