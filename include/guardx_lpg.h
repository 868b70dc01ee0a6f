/*
 * guardx_lpg.h -- C ABI of libguardx_lpg.so: the per-control-step policy launch of the LPG rollout, for gfx950.
 * The `lpg` learner (safe_rl_libX/lpg/lpg.py:486-564, lpg_core.py:148-198, 224-233) evaluates a cost critic
 * Q(obs, act) = Softplus(c_net(cat(obs, act))) next to the actor and the critic (USL's module) and, after its warm-up,
 * projects the action along the gradient of Q at the ZERO action before env.step sees it.  One gxp_policy_step launch
 * per control step does
 *
 *   prologue (skipped at t == 0), per env: rew / cost / done [t-1] = the step's (copied)
 *   body: obs_rd -> obs[t]; mu_net and v_net on the row (the bits of rollout_policy);
 *       act = mu + exp(log_std) z with z from the Threefry block at (env_offset + env, 16 (step0 + t) + pair);
 *       qc[t] = Q(obs, act) on the UNCORRECTED act (what ac.step returns and buf.store keeps);
 *       if t == 0 and store_init: q_init[env] = qc[0]          (C_Critic.store_init, held for the whole epoch)
 *       act_safe = correct ? projection(obs, act, q_init) : act;  lam[t] = the multiplier applied (0 if none)
 *       -> obs, act, act_safe, mu, logp, val, qc, lam [t]  (and logstd); logp is that of act
 *   tail (t == T): the prologue for step T - 1, then obs_last, val_last; no action, no noise, no Q.
 *
 * The projection, per row (lpg_core.py:171-198); it is closed-form, not an iteration:
 *   q = Q(obs, act);  if q <= delta: a_safe = act                                   (branch 0)
 *   G[k] = grad_scale * d Q(obs, 0) / d a[k]           the gradient at the zero action, not at act
 *   eps = |delta - q_init|                             lpg_core.py:187-188: (1 - gamma) |delta - Q_init| with gamma = 0.0
 *   lam = max((G . act - eps) / (G . G), 0);  a_safe = act + step_sign * lam G      (branch 1: lam > 0; 2: clipped or NaN)
 * There is no clamp and no epsilon in the denominator; Niter, eta and prev_cost of the reference's signature are unused.
 * Quirks of the reference, kept in the open rather than copied silently:
 *   1. lpg_core.py:178 backpropagates pred_0.mean(), so its G is the true gradient Gt divided by the batch size N.
 *      Unlike USL's update the factor does NOT cancel: lam G = (Gt . a - N eps) / (Gt . Gt) Gt.  grad_scale carries it:
 *      1 / env_num is the reference's arithmetic for an unsharded engine, 1 the unscaled form.
 *   2. lpg_core.py:195 ADDS lam G: the step goes up Q's gradient (Dalal's layer subtracts).  step_sign = +1 is the
 *      reference as written, -1 the other sign; the factor is exact either way.
 *   3. lpg_core.py:193 concatenates (lam, lam), which hard-codes act_dim == 2.  Here lam multiplies every component of
 *      G: the reference's expression at A = 2, an extension elsewhere.
 *   4. The reference computes lam in float64 numpy (Q_init is stored as double) and casts lam G back to float32; this
 *      library works in float32 throughout.
 *   5. There is no guard on G . G == 0, and none here: the same IEEE division.  A zero gradient with eps > 0 gives
 *      -inf, lam = 0 and a_safe = act exactly; 0 / 0 gives a NaN action (lam < 0 is false for a NaN, as numpy's
 *      lam[lam < 0] = 0 leaves it), which the env's NaN guard handles like any other NaN action.
 *   6. lpg_core.py:182 `len(torch.where(...)) != 0` is always true and changes no value.
 *
 * Arithmetic.  c_net is evaluated by the device code libguardx_usl.so uses (guardx_amd/csrc/gx_qcritic.h), in the order
 * include/guardx_usl.h fixes for one pass: hidden units are fmaf chains from the bias over k ascending (c_net's first
 * layer over the D observation columns, P, then the A action columns), gx tanh, z3 = b3 + dot16(w3, h2), gx Softplus.
 *   act pass:   the A action terms of act on top of P, tanh, second layer, head: qc = softplus(z3)
 *   zero pass:  h1 = tanh(P) with NO action terms (not A terms with a zero action), second layer, head z3_0, then
 *               d2[j] = (1 - h2[j] * h2[j]) * w3[j];  d1 = fmaf chain from 0 over j ascending of d2[j] * W2[j][k];
 *               g1[k] = (1 - h1[k] * h1[k]) * d1[k];  g~[i] = dot16(W1[:, D + i], g1)
 *               e = exp(z3_0);  sp = z3_0 > 20 ? 1 : e / (e + 1);  c0 = grad_scale * sp;  G[i] = c0 * g~[i]
 * The projection, every operator one IEEE fp32 operation, no fused multiply-add:
 *   eps = |delta - q_init|
 *   top = (G[0] * a[0] + G[1] * a[1] + ... ) - eps          (the sum from the first product, k ascending)
 *   bot =  G[0] * G[0] + G[1] * G[1] + ...                  (the same order)
 *   lam = top / bot;  lam = lam < 0 ? 0 : lam               (a NaN stays a NaN)
 *   a_safe[k] = a[k] + step_sign * (lam * G[k])
 * A numpy float32 transcription of these lines gives the same bits from the same G, q and q_init.
 *
 * Parameters: d_params = pack_actor_critic layout on D inputs (gxp_params_floats);
 * d_c_params = c_net W1[hc][D + A] b1 W2[hc][hc] b2 W3[1][hc] b3 (gxp_q_floats); h, hc in {64, 128, 192, 256},
 * independent of each other.  d_q_init: one float per env, owned by the caller across calls.
 *
 * All `d_*` pointers are DEVICE addresses, dense; fp32 unless said otherwise.  `stream` is a hipStream_t passed as
 * void* (NULL = default stream).  Nothing here throws or synchronises; every call that can fail returns a gxp_status
 * and gxp_last_error() describes the last failure on the calling thread.  This library is separate from the five
 * older ones and carries its own build id.
 */
#ifndef GUARDX_LPG_H
#define GUARDX_LPG_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gxp_status {
    GXP_OK = 0,
    GXP_ERR_ARG = 1,         /* null pointer, negative count, bad struct_size, t outside [0, T] */
    GXP_ERR_UNSUPPORTED = 2, /* hidden width not in {64, 128, 192, 256}, odd or too wide A, D too wide for the LDS */
    GXP_ERR_HIP = 4          /* a HIP runtime call failed */
} gxp_status;

/* One control step `t` of a T-step call.  Time-major outputs are addressed by the kernel itself (row block t, or
 * t - 1 for the prologue's), so a driver sets `t` and nothing else between launches. */
typedef struct gxp_step_args {
    uint32_t struct_size;     /* sizeof(gxp_step_args) */
    int32_t N, D, A;          /* envs, observation width, action width (even, <= 16) */
    int32_t hidden, c_hidden;
    int32_t env_offset;       /* global index of env 0 (noise counter) */
    int32_t T, t;             /* t in [0, T]; t == T is the tail */
    int32_t correct;          /* 0: the warm-up branch, act_safe = act */
    int32_t store_init;       /* != 0: the launch at t == 0 writes q_init = qc[0] before it projects */
    uint32_t seed[2];         /* key of the action-noise stream */
    uint32_t step0;           /* policy steps taken before this call (noise counter offset) */
    float delta, grad_scale, step_sign;
    const float* d_params;    /* gxp_params_floats(D, A, hidden) */
    const float* d_c_params;  /* gxp_q_floats(D, A, c_hidden) */
    const float* d_work;      /* gxp_work_floats(...), filled by gxp_prepare */
    const float* d_obs0;      /* [N][D] observation at entry (read at t == 0) */
    const float* d_obs_rd;    /* [N][D] post-reset_done observation of the step just made (t > 0) */
    const float* d_rew_in;    /* [N] reward, cost, done of the step just made (t > 0) */
    const float* d_cost_in;
    const float* d_done_in;
    float* d_q_init;          /* [N] Q of the epoch's first step: written at t == 0 if store_init, read otherwise */
    float* d_obs;             /* [T][N][D] */
    float* d_act;             /* [T][N][A] */
    float* d_act_safe;        /* [T][N][A] what env.step receives */
    float* d_mu;              /* [T][N][A] */
    float* d_logp;            /* [T][N] */
    float* d_val;             /* [T][N] */
    float* d_qc;              /* [T][N] Q(obs, act) */
    float* d_lam;             /* [T][N] the multiplier applied, 0 for an uncorrected row */
    float* d_rew;             /* [T][N] copies of the step's reward / cost / done */
    float* d_cost;
    float* d_done;
    float* d_obs_last;        /* [N][D] */
    float* d_val_last;        /* [N] */
    float* d_logstd;          /* [A] */
} gxp_step_args;

const char* gxp_last_error(void);
/* sha256 (24 hex digits) over the library's sources, headers, flags and compiler (guardx_amd/build.py) */
const char* gxp_build_id(void);

/* floats of the packed actor-critic on D inputs; -1 if unsupported */
int64_t gxp_params_floats(int32_t D, int32_t A, int32_t hidden);
/* floats of the packed c_net on D + A inputs; -1 if unsupported */
int64_t gxp_q_floats(int32_t D, int32_t A, int32_t c_hidden);
/* floats of gxp_policy_step's device workspace (the transposed hidden layers of the three networks); -1 if unsupported */
int64_t gxp_work_floats(int32_t D, int32_t A, int32_t hidden, int32_t c_hidden);
/* floats of gxp_projection_probe's device workspace (c_net's transposed hidden layers); -1 if unsupported */
int64_t gxp_probe_work_floats(int32_t D, int32_t A, int32_t c_hidden);

/* Once per call, before its first gxp_policy_step: transposes the hidden layers into d_work (stream-ordered). */
gxp_status gxp_prepare(int32_t D, int32_t A, int32_t hidden, int32_t c_hidden, const float* d_params,
                       const float* d_c_params, float* d_work, void* stream);

/* One launch over all N envs (see the top of this file).  Arguments are checked before anything is launched;
 * N == 0 launches nothing. */
gxp_status gxp_policy_step(const gxp_step_args* args, void* stream);

/* The per-env bookkeeping of a one-episode rollout, the second argument of guardx_lpg_policy_step_episode.  The
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

/* The two entries below carry the library's full name instead of its gxp_ prefix: the set of gxp_ symbols is the
 * library's first ABI, which stays as it was. */
/* The one-episode form of gxp_policy_step (the `lpg_one_episode` learner: no reset_done between the steps; the
 * driver's env launch is a plain step and d_obs_rd is the env's plain observation).  Same arguments, same checks,
 * plus the bookkeeping of gx_first_done_state below (null, t_base < 0, a wrong struct_size or a null pointer
 * in it: GXP_ERR_ARG, nothing launched).  Against gxp_policy_step:
 *   the row read has every NaN / +Inf / -Inf entry replaced by +0.0f; that row feeds every network and is what
 *   obs[t] keeps;
 *   the prologue of t > 0 runs the first-done bookkeeping after its copies (gx_first_done_state);
 *   the tail writes obs_last raw and val_last = v on the sanitised row, 0 for a row with any non-finite entry.
 *   The sanitised row is what c_net reads in both passes; qc, q_init, the projection and lam are those of
 *   gxp_policy_step.
 */
gxp_status guardx_lpg_policy_step_episode(const gxp_step_args* args, const gx_first_done_state* book, void* stream);

/* The tail launch of the one-episode form alone on n caller-supplied rows d_rows [n][D] (after gxp_prepare on the
 * same networks): d_obs_last = the rows as they are, d_val_last by the tail's rule.  No state is touched. */
gxp_status guardx_lpg_tail_probe(int32_t n, int32_t D, int32_t A, int32_t hidden, int32_t c_hidden, const float* d_params,
                          const float* d_c_params, const float* d_work, const float* d_rows, float* d_obs_last,
                          float* d_val_last, void* stream);

/* The projection alone, with the step kernel's own device functions, on n caller-supplied rows d_obs [n][D], d_act
 * [n][A], d_q_init [n]:  d_a_safe [n][A];  d_q [n] Q at the input action;  d_G [n][A] the scaled gradient at the zero
 * action (every row);  d_lam [n] the multiplier applied, 0 for branch 0;  d_branch [n] (int32): 0 q <= delta, 1 corrected
 * with lam > 0, 2 corrected with lam clipped to 0 or NaN.  d_work: gxp_probe_work_floats floats of scratch, filled by
 * this call itself (stream-ordered). */
gxp_status gxp_projection_probe(int32_t n, int32_t D, int32_t A, int32_t c_hidden, const float* d_c_params,
                                float* d_work, const float* d_obs, const float* d_act, const float* d_q_init,
                                float delta, float grad_scale, float step_sign, float* d_a_safe, float* d_q, float* d_G,
                                float* d_lam, int32_t* d_branch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GUARDX_LPG_H */
