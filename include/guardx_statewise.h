/*
 * guardx_statewise.h -- C ABI of libguardx_statewise.so: the per-control-step policy launch of the
 * state-wise (SCPO) rollout, for gfx950.  SCPO (safe_rl_libX/scpo/scpo.py:640-720, scpo_core.py:158-200)
 * feeds its three networks the observation augmented by M, the env's running maximum of the cost since
 * its episode began, and stores the cost INCREMENT of every step.  M depends on the cost of the step
 * just made, so it lives inside the closed loop: one gxs_policy_step launch per control step does
 *
 *   prologue (the M update of the step just made, skipped at t == 0), per env, fp32, in this order:
 *       inc    = first ? cost : max(cost - M, 0)
 *       M_next = first ? cost : M + inc
 *       cost_inc[t-1] = inc;  M_after[t-1] = M_next;  rew / cost / done [t-1] = the step's (copied)
 *       done ? (M = 0, first = 1) : (M = M_next, first = 0)
 *   body: o_aug = [obs_rd | M] -> obs[t]; mu_net, v_net and the Softplus-headed cost critic on o_aug;
 *       act = mu + exp(log_std) z with z from the Threefry block at (env_offset + env, 16 (step0 + t) + pair)
 *       -> act, mu, logp, val, vc [t]  (and logstd)
 *   tail (t == T): the prologue for step T - 1, then obs_last, val_last, vc_last; no action, no noise.
 *
 * The arithmetic is the fused rollout's (guardx_amd/csrc/gx_policy.h, oracle/gx_oracle.c:mlp_forward):
 *   hidden unit j:  acc = b[j]; acc = fmaf(x[k], W[j][k], acc) for k = 0, 1, ...; then gx tanh
 *   output:         16 partials, partial l = fmaf chain from 0 over the units 64 c + 4 l + j, folded by a
 *                   butterfly (xor 8, 4, 2, 1); b3 + sum
 *   Softplus (torch: beta 1, threshold 20):  x > 20 ? x : max(x, 0) + log1p(exp(-|x|))
 *
 * Parameters: d_params = pack_actor_critic layout on D_aug inputs,
 *   pi{W1[h][D_aug] b1 W2[h][h] b2 W3[A][h] b3} v{.. W3[1][h] b3} log_std[A]   (gxs_params_floats)
 * d_vc_params = one critic W1[hc][D_aug] b1 W2[hc][hc] b2 W3[1][hc] b3; h, hc in {64, 128, 192, 256}.
 *
 * All `d_*` pointers are DEVICE addresses, fp32, dense.  `stream` is a hipStream_t passed as void*
 * (NULL = default stream).  Nothing here throws or synchronises; every call that can fail returns a
 * gxs_status and gxs_last_error() describes the last failure on the calling thread.  This library is
 * separate from libguardx_hip.so and libguardx_critic.so and carries its own build id.
 */
#ifndef GUARDX_STATEWISE_H
#define GUARDX_STATEWISE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gxs_status {
    GXS_OK = 0,
    GXS_ERR_ARG = 1,         /* null pointer, negative count, bad struct_size, t outside [0, T] */
    GXS_ERR_UNSUPPORTED = 2, /* hidden width not in {64, 128, 192, 256}, odd or too wide A, D_aug too wide for the LDS */
    GXS_ERR_HIP = 4          /* a HIP runtime call failed */
} gxs_status;

/* One control step `t` of a T-step call.  Time-major outputs are addressed by the kernel itself (row
 * block t, or t - 1 for the prologue's), so a driver sets `t` and nothing else between launches. */
typedef struct gxs_step_args {
    uint32_t struct_size;     /* sizeof(gxs_step_args) */
    int32_t N, D_aug, A;      /* envs, observation width + 1, action width (even, <= 16) */
    int32_t hidden, vc_hidden;
    int32_t env_offset;       /* global index of env 0 (noise counter) */
    int32_t T, t;             /* t in [0, T]; t == T is the tail */
    uint32_t seed[2];         /* key of the action-noise stream */
    uint32_t step0;           /* policy steps taken before this call (noise counter offset) */
    const float* d_params;    /* gxs_params_floats(D_aug, A, hidden) */
    const float* d_vc_params; /* the cost critic, Softplus output */
    const float* d_work;      /* gxs_work_floats(...), filled by gxs_prepare */
    const float* d_obs0;      /* [N][D_aug - 1] observation at entry (read at t == 0) */
    const float* d_obs_rd;    /* [N][D_aug - 1] post-reset_done observation of the step just made (t > 0) */
    const float* d_rew_in;    /* [N] reward, cost, done of the step just made (t > 0) */
    const float* d_cost_in;
    const float* d_done_in;
    float* d_M;               /* [N] state: running maximum, updated in place */
    float* d_first;           /* [N] state: 1.f on an episode's first step, else 0.f */
    float* d_obs;             /* [T][N][D_aug] */
    float* d_act;             /* [T][N][A] */
    float* d_mu;              /* [T][N][A] */
    float* d_logp;            /* [T][N] */
    float* d_val;             /* [T][N] */
    float* d_vc;              /* [T][N] */
    float* d_rew;             /* [T][N] copies of the step's reward / cost / done */
    float* d_cost;
    float* d_done;
    float* d_cost_inc;        /* [T][N] */
    float* d_M_after;         /* [T][N] M_next after step t, before any reset */
    float* d_obs_last;        /* [N][D_aug] */
    float* d_val_last;        /* [N] */
    float* d_vc_last;         /* [N] */
    float* d_logstd;          /* [A] */
} gxs_step_args;

const char* gxs_last_error(void);
/* sha256 (24 hex digits) over the library's sources, headers, flags and compiler (guardx_amd/build.py) */
const char* gxs_build_id(void);

/* floats of the packed actor-critic on D_aug inputs; -1 if unsupported */
int64_t gxs_params_floats(int32_t D_aug, int32_t A, int32_t hidden);
/* floats of the device workspace (the transposed hidden layers of the three networks); -1 if unsupported */
int64_t gxs_work_floats(int32_t D_aug, int32_t A, int32_t hidden, int32_t vc_hidden);

/* Once per call, before its first gxs_policy_step: transposes the hidden layers into d_work (stream-ordered). */
gxs_status gxs_prepare(int32_t D_aug, int32_t A, int32_t hidden, int32_t vc_hidden, const float* d_params,
                       const float* d_vc_params, float* d_work, void* stream);

/* One launch over all N envs (see the top of this file).  Arguments are checked before anything is launched;
 * N == 0 launches nothing. */
gxs_status gxs_policy_step(const gxs_step_args* args, void* stream);

/* d_y[i] = Softplus(d_x[i]) for i < n with the kernel's own evaluation: measures its accuracy on its own. */
gxs_status gxs_softplus_probe(int32_t n, const float* d_x, float* d_y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GUARDX_STATEWISE_H */
