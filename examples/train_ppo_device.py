#!/usr/bin/env python3
"""examples/train_ppo_fused.py with the learners' own update, on the device: after the one-launch collection phase and GAE,
the actor is fitted over the FULL batch of env_num x 200 rows by PolicyFit.fit (ppo.py's loop of train_pi_iters = 80 rounds of
Adam on the clipped surrogate with its early stop on kl, decided on the device) and the critic by ValueFit.fit
(train_v_iters = 80) -- no subsampling, no autograd graph, and no host synchronisation until the epoch's line is printed.

    python examples/train_ppo_device.py [--epochs 30] [--env-num 2000]

The hidden width is 64, the one the two fits serve.  The return must go up.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from guardx_amd import Engine, PolicyFit, ValueFit, configuration  # noqa: E402
from guardx_amd.rollout_buffer import gae_rollout  # noqa: E402


def mlp(sizes):          # trpo_core.py:30-35
    layers = []
    for j in range(len(sizes) - 1):
        layers += [nn.Linear(sizes[j], sizes[j + 1]), nn.Tanh() if j < len(sizes) - 2 else nn.Identity()]
    return nn.Sequential(*layers)


class Actor(nn.Module):  # trpo_core.MLPGaussianActor's parameters, in its order: log_std, then mu_net
    def __init__(self, D, A):
        super().__init__()
        self.log_std = nn.Parameter(torch.full((A,), -0.5))
        self.mu_net = mlp([D, 64, 64, A])


class Critic(nn.Module):  # trpo_core.MLPCritic
    def __init__(self, D):
        super().__init__()
        self.v_net = mlp([D, 64, 64, 1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--env-num", type=int, default=2000)
    ap.add_argument("--task", default="Goal_Point_8Hazards")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--train-pi-iters", type=int, default=80)
    ap.add_argument("--train-v-iters", type=int, default=80)
    ap.add_argument("--target-kl", type=float, default=0.01)
    ap.add_argument("--clip-ratio", type=float, default=0.2)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)
    T = 200
    cfg = dict(configuration(args.task), env_num=args.env_num, _seed=args.seed, num_steps=T)
    env = Engine(cfg)
    D, A = env.obs_flat_size, env.action_space.shape[0]
    pi, v = Actor(D, A).to(dev), Critic(D).to(dev)
    PF, VF = PolicyFit(pi, lr=3e-4), ValueFit(v, lr=1e-3)     # in place of pi_optimizer and vf_optimizer
    print(f"{'epoch':>5} {'EpRet':>9} {'EpCost':>9} {'EpLen':>7} {'goals/env':>9} {'StopIter':>8} {'KL':>9} {'ClipFrac':>8} "
          f"{'LossV':>9} {'collect ms':>10} {'update ms':>10}")
    for epoch in range(args.epochs):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        env.reset(check=False)
        params = Engine.pack_actor_critic(mu_net=pi.mu_net, v_net=v.v_net, log_std=pi.log_std)
        out = env.rollout_policy(params, T, noise_seed=(args.seed, epoch))
        adv, ret = gae_rollout(out['rew'], out['val'], out['done'])
        torch.cuda.synchronize(); t1 = time.perf_counter()
        # episode statistics (an episode ends at done or at the end of the tape)
        done = out['done']
        n_ep = done.sum() + (done[-1] == 0).sum()
        ep_ret = out['rew'].sum() / n_ep
        ep_cost = out['cost'].sum() / n_ep
        ep_len = done.numel() / n_ep
        # the learners' update over the whole batch
        adv_f = adv.reshape(-1)
        adv_f = ((adv_f - adv_f.mean()) / (adv_f.std() + 1e-8)).contiguous()
        data = dict(obs=out['obs'].reshape(-1, D).contiguous(), act=out['act'].reshape(-1, A).contiguous(), adv=adv_f,
                    logp=out['logp'].reshape(-1).contiguous())
        pinfo = PF.fit(data, iters=args.train_pi_iters, target_kl=args.target_kl, clip_ratio=args.clip_ratio)
        vinfo = VF.fit(data['obs'], ret.reshape(-1).contiguous(), iters=args.train_v_iters)
        torch.cuda.synchronize(); t2 = time.perf_counter()
        print(f"{epoch:5d} {ep_ret.item():9.4f} {ep_cost.item():9.4f} {ep_len.item():7.1f} "
              f"{(done.sum() / args.env_num).item():9.3f} {int(pinfo['stop_iter']):8d} {float(pinfo['kl_last']):9.5f} "
              f"{float(pinfo['cf_last']):8.4f} {float(vinfo['loss'][0]):9.4f} {(t1 - t0) * 1e3:10.2f} {(t2 - t1) * 1e3:10.2f}")
    env.check_layouts()


if __name__ == "__main__":
    main()
