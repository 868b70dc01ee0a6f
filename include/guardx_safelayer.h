/*
 * guardx_safelayer.h -- C ABI of libguardx_safelayer.so: the per-control-step policy launch of the
 * safety-layer rollout (Dalal et al. 2018), for gfx950.  The `safelayer` learner
 * (safe_rl_libX/safelayer/safelayer.py:514-581, safelayer_core.py:147-190) edits the action between
 * ac.step and env.step, and the edit reads the cost of the step just made (prev_c), so prev_c lives
 * inside the closed loop: one gxl_policy_step launch per control step does
 *
 *   prologue (skipped at t == 0), per env: rew / cost / done [t-1] = the step's (copied);
 *       prev_c = done ? 0 : cost
 *   body: obs_rd -> obs[t]; mu_net, v_net and g_net on the same row;
 *       act = mu + exp(log_std) z with z from the Threefry block at (env_offset + env, 16 (step0 + t) + pair);
 *       prev_cost[t] = prev_c; act_safe = correct ? correction(g, act, prev_c, delta) : act
 *       -> obs, act, act_safe, mu, g, logp, val, prev_cost [t]  (and logstd); logp is that of act
 *   tail (t == T): the prologue for step T - 1, then obs_last, val_last; no action, no noise.
 *
 * The networks' arithmetic is the fused rollout's (guardx_amd/csrc/gx_policy.h, oracle/gx_oracle.c:mlp_forward):
 *   hidden unit j:  acc = b[j]; acc = fmaf(x[k], W[j][k], acc) for k = 0, 1, ...; then gx tanh
 *   output:         16 partials, partial l = fmaf chain from 0 over the units 64 c + 4 l + j, folded by a
 *                   butterfly (xor 8, 4, 2, 1); b3 + sum
 *
 * The correction (safelayer_core.py:169-190 for act_dim = 2, mult[:, None] * g for any A), fp32, every
 * operator one IEEE operation, no fused multiply-add, in this order:
 *   ga = g[0] * a[0];  ga = ga + g[k] * a[k]   for k = 1 .. A - 1
 *   gg = g[0] * g[0];  gg = gg + g[k] * g[k]   for k = 1 .. A - 1
 *   pred = ga + prev_c
 *   pred <= delta:  a_safe[k] = a[k]                          (unclamped)
 *   otherwise:      numer = pred - delta;  denom = gg + 1e-8f;  mult = numer / denom  (IEEE division)
 *                   mult = mult > 0 ? mult : 0
 *                   a_safe[k] = min(max(a[k] - mult * g[k], -1), 1)
 * A numpy float32 transcription gives the same bits from the same g, a, prev_c.
 *
 * Parameters: d_params = pack_actor_critic layout on D inputs,
 *   pi{W1[h][D] b1 W2[h][h] b2 W3[A][h] b3} v{.. W3[1][h] b3} log_std[A]   (gxl_params_floats)
 * d_g_params = g_net W1[hg][D] b1 W2[hg][hg] b2 W3[A][hg] b3 (gxl_g_floats); h, hg in {64, 128, 192, 256}:
 * the actor and the critic share one width, g_net may have its own.
 *
 * All `d_*` pointers are DEVICE addresses, fp32, dense.  `stream` is a hipStream_t passed as void*
 * (NULL = default stream).  Nothing here throws or synchronises; every call that can fail returns a
 * gxl_status and gxl_last_error() describes the last failure on the calling thread.  This library is
 * separate from libguardx_hip.so, libguardx_critic.so and libguardx_statewise.so and carries its own build id.
 */
#ifndef GUARDX_SAFELAYER_H
#define GUARDX_SAFELAYER_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gxl_status {
    GXL_OK = 0,
    GXL_ERR_ARG = 1,         /* null pointer, negative count, bad struct_size, t outside [0, T] */
    GXL_ERR_UNSUPPORTED = 2, /* hidden width not in {64, 128, 192, 256}, odd or too wide A, D too wide for the LDS */
    GXL_ERR_HIP = 4          /* a HIP runtime call failed */
} gxl_status;

/* One control step `t` of a T-step call.  Time-major outputs are addressed by the kernel itself (row
 * block t, or t - 1 for the prologue's), so a driver sets `t` and nothing else between launches. */
typedef struct gxl_step_args {
    uint32_t struct_size;     /* sizeof(gxl_step_args) */
    int32_t N, D, A;          /* envs, observation width, action width (even, <= 16) */
    int32_t hidden, g_hidden;
    int32_t env_offset;       /* global index of env 0 (noise counter) */
    int32_t T, t;             /* t in [0, T]; t == T is the tail */
    int32_t correct;          /* 0: the warm-up branch, act_safe = act */
    uint32_t seed[2];         /* key of the action-noise stream */
    uint32_t step0;           /* policy steps taken before this call (noise counter offset) */
    float delta;              /* the correction's threshold */
    const float* d_params;    /* gxl_params_floats(D, A, hidden) */
    const float* d_g_params;  /* gxl_g_floats(D, A, g_hidden) */
    const float* d_work;      /* gxl_work_floats(...), filled by gxl_prepare */
    const float* d_obs0;      /* [N][D] observation at entry (read at t == 0) */
    const float* d_obs_rd;    /* [N][D] post-reset_done observation of the step just made (t > 0) */
    const float* d_rew_in;    /* [N] reward, cost, done of the step just made (t > 0) */
    const float* d_cost_in;
    const float* d_done_in;
    float* d_prev_c;          /* [N] state: the cost of the env's previous step, 0 after a done; updated in place */
    float* d_obs;             /* [T][N][D] */
    float* d_act;             /* [T][N][A] */
    float* d_act_safe;        /* [T][N][A] what env.step receives */
    float* d_mu;              /* [T][N][A] */
    float* d_g;               /* [T][N][A] */
    float* d_logp;            /* [T][N] */
    float* d_val;             /* [T][N] */
    float* d_rew;             /* [T][N] copies of the step's reward / cost / done */
    float* d_cost;
    float* d_done;
    float* d_prev_cost;       /* [T][N] the prev_c the correction at step t used */
    float* d_obs_last;        /* [N][D] */
    float* d_val_last;        /* [N] */
    float* d_logstd;          /* [A] */
} gxl_step_args;

const char* gxl_last_error(void);
/* sha256 (24 hex digits) over the library's sources, headers, flags and compiler (guardx_amd/build.py) */
const char* gxl_build_id(void);

/* floats of the packed actor-critic on D inputs; -1 if unsupported */
int64_t gxl_params_floats(int32_t D, int32_t A, int32_t hidden);
/* floats of the packed g_net; -1 if unsupported */
int64_t gxl_g_floats(int32_t D, int32_t A, int32_t g_hidden);
/* floats of the device workspace (the transposed hidden layers of the three networks); -1 if unsupported */
int64_t gxl_work_floats(int32_t D, int32_t A, int32_t hidden, int32_t g_hidden);

/* Once per call, before its first gxl_policy_step: transposes the hidden layers into d_work (stream-ordered). */
gxl_status gxl_prepare(int32_t D, int32_t A, int32_t hidden, int32_t g_hidden, const float* d_params,
                       const float* d_g_params, float* d_work, void* stream);

/* One launch over all N envs (see the top of this file).  Arguments are checked before anything is launched;
 * N == 0 launches nothing. */
gxl_status gxl_policy_step(const gxl_step_args* args, void* stream);

/* The per-env bookkeeping of a one-episode rollout, the second argument of guardx_safelayer_policy_step_episode.  The
 * same declaration stands in guardx_safelayer.h, guardx_usl.h and guardx_lpg.h under one guard (each library's build
 * id covers its own header alone).  The prologue of step t > 0 of such a launch does, per env, after its copies
 * of rew / cost / done [t-1] and in this order, with k = t_base + t:
 *       first_done == 0 ?  ep_ret += rew, ep_cost += cost (fp32, one add each), ep_len = k
 *       done > 0 and first_done == 0 ?  first_done = k
 * which is include/guardx_episode.h's bookkeeping, operation for operation.  Device addresses, dense, [N]. */
#ifndef GX_FIRST_DONE_STATE_DEFINED
#define GX_FIRST_DONE_STATE_DEFINED
typedef struct gx_first_done_state {
    uint32_t struct_size;     /* sizeof(gx_first_done_state) */
    int32_t t_base;           /* steps of the episode made before this call (>= 0) */
    int32_t* d_first_done;    /* 1-based index of the first step with done, 0 = not finished */
    int32_t* d_ep_len;        /* steps counted into ep_ret / ep_cost */
    float* d_ep_ret;          /* reward summed up to and including the first done step */
    float* d_ep_cost;         /* cost likewise */
} gx_first_done_state;
#endif

/* The two entries below carry the library's full name instead of its gxl_ prefix: the set of gxl_ symbols is the
 * library's first ABI, which stays as it was. */
/* The one-episode form of gxl_policy_step (the `safelayer_one_episode` learner: no reset_done between the steps; the
 * driver's env launch is a plain step and d_obs_rd is the env's plain observation).  Same arguments, same checks,
 * plus the bookkeeping of gx_first_done_state below (null, t_base < 0, a wrong struct_size or a null pointer
 * in it: GXL_ERR_ARG, nothing launched).  Against gxl_policy_step:
 *   the row read has every NaN / +Inf / -Inf entry replaced by +0.0f; that row feeds every network and is what
 *   obs[t] keeps;
 *   the prologue of t > 0 runs the first-done bookkeeping after its copies (gx_first_done_state);
 *   the tail writes obs_last raw and val_last = v on the sanitised row, 0 for a row with any non-finite entry.
 *   prev_c = cost, whatever `done` says: nothing is re-initialised at a done (safelayer_one_episode/
 *   safelayer.py:553); prev_cost[t] is still the value the correction at step t used.  The tail makes the
 *   last prev_c update.
 */
gxl_status guardx_safelayer_policy_step_episode(const gxl_step_args* args, const gx_first_done_state* book, void* stream);

/* The tail launch of the one-episode form alone on n caller-supplied rows d_rows [n][D] (after gxl_prepare on the
 * same networks): d_obs_last = the rows as they are, d_val_last by the tail's rule.  No state is touched. */
gxl_status guardx_safelayer_tail_probe(int32_t n, int32_t D, int32_t A, int32_t hidden, int32_t g_hidden, const float* d_params,
                          const float* d_g_params, const float* d_work, const float* d_rows, float* d_obs_last,
                          float* d_val_last, void* stream);

/* d_a_safe[i][:] = correction(d_g[i][:], d_a[i][:], d_prev_c[i], delta) for i < n, rows of A (1 .. 16) floats:
 * the correction alone, with the kernel's own evaluation. */
gxl_status gxl_correction_probe(int32_t n, int32_t A, const float* d_g, const float* d_a, const float* d_prev_c,
                                float delta, float* d_a_safe, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GUARDX_SAFELAYER_H */
