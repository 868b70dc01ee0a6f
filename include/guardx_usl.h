/*
 * guardx_usl.h -- C ABI of libguardx_usl.so: the per-control-step policy launch of the USL rollout, for gfx950.
 * The `usl` learner (safe_rl_libX/usl/usl.py:478-553, usl_core.py:146-196, 239-248) evaluates a cost critic
 * Q(obs, act) = Softplus(c_net(cat(obs, act))) next to the actor and the critic and, after its warm-up, walks the
 * action down Q's gradient before env.step sees it.  One gxu_policy_step launch per control step does
 *
 *   prologue (skipped at t == 0), per env: rew / cost / done [t-1] = the step's (copied)
 *   body: obs_rd -> obs[t]; mu_net and v_net on the row (the bits of rollout_policy);
 *       act = mu + exp(log_std) z with z from the Threefry block at (env_offset + env, 16 (step0 + t) + pair);
 *       qc[t] = Q(obs, act) on the UNCORRECTED act (what ac.step returns and buf.store keeps);
 *       act_safe = correct ? iteration(obs, act) : act;  iters[t] = the updates applied (float32)
 *       -> obs, act, act_safe, mu, logp, val, qc, iters [t]  (and logstd); logp is that of act
 *   tail (t == T): the prologue for step T - 1, then obs_last, val_last; no action, no noise, no Q.
 *
 * The iteration, per row (usl_core.py:165-196):
 *   a = act;  acc = 0
 *   repeat at most niter times:
 *       if max_k a[k] > 1:  stop (reason 1)        the SIGNED maximum, not |a|: usl_core.py:174-175 as written
 *       q = Q(obs, a);  if q <= delta: stop (reason 2)
 *       g~[k] = d z3 / d a[k]                       z3 = c_net's output before its Softplus
 *       c = grad_scale * softplus'(z3)              softplus'(z) = z > 20 ? 1 : e^z / (e^z + 1)  (torch's backward)
 *       s[k] = c g~[k];  acc[k] = acc[k] + s[k];  Z = max_k |acc[k]|;  a[k] = a[k] - eta * (acc[k] / (Z + 1e-8))
 *   reason 0: niter updates applied.  There is no clamp, and a stopped row never moves again.
 * Three quirks of the reference, kept in the open rather than copied silently:
 *   * usl_core.py:184 backpropagates pred.mean(), so its act.grad is the true gradient divided by the batch size; the
 *     division by Z takes the factor out again except against the 1e-8.  grad_scale carries it: 1 / env_num is the
 *     reference's arithmetic for an unsharded engine, 1 the unscaled form.
 *   * the box test is max_k a[k] > 1 on the signed components: a row at a = (-3, 0.5) keeps iterating.
 *   * usl_core.py:180-194 never clears act.grad: c_net.zero_grad() (line 182) zeroes the network's gradients only and
 *     act is the same leaf tensor in every pass, so each backward() (line 184) ADDS to act.grad (an fp32 add inside
 *     torch's accumulation) and the update of pass p (lines 190-194) uses the sum of s over the passes 1 .. p, a
 *     momentum-like step, not the gradient at the current action.  Against the memoryless form (which this library
 *     computed before): equal on rows that move once, 8.9e-4 apart on rows that move twice, up to 0.05 at ten passes
 *     and 0.54 at twenty (C_Critic(43, 2, (64, 64)), 64 rows, eta 0.05); no stop reason changed.
 *
 * Arithmetic.  Hidden units are the project's chains (guardx_amd/csrc/gx_policy.h, oracle/gx_oracle.c:mlp_forward):
 *   hidden unit j:  acc = b[j]; acc = fmaf(x[k], W[j][k], acc) for k = 0, 1, ...; then gx tanh
 *   c_net's first layer runs k over the D observation columns and THEN the A action columns: the observation part
 *   is evaluated once per control step, every pass continues it with the A action terms.
 *   z3 = b3 + dot16(w3, h2);  dot16(w, h): 16 partials, partial l = fmaf chain from 0 over the units 64 c + 4 l + j
 *   (c, then j ascending), folded by a butterfly (xor 8, 4, 2, 1).  q = gx Softplus (the statewise path's form).
 * The backward pass, every operator one IEEE operation (fp32, no contraction) unless written fmaf:
 *   d2[j] = (1 - h2[j] * h2[j]) * w3[j]
 *   d1[k] = fmaf chain from 0 over j = 0, 1, ..., h_c - 1 of d2[j] * W2[j][k]      (one MFMA chain, j ascending)
 *   g1[k] = (1 - h1[k] * h1[k]) * d1[k]
 *   g~[i] = dot16(W1[:, D + i], g1)                                                 (the order of dot16 over k)
 *   e = exp(z3);  sp = z3 > 20 ? 1 : e / (e + 1);  c = grad_scale * sp
 *   s[i] = c * g~[i];  acc[i] = s[i] in the row's first pass, acc[i] + s[i] after it (per row, in registers)
 *   Z = |acc[0]|, then Z = |acc[i]| > Z ? |acc[i]| : Z for i = 1 .. A - 1;  den = Z + 1e-8f
 *   a[i] = a[i] - eta * (acc[i] / den)                     (IEEE division, then the product, then the difference)
 * A numpy float32 transcription of the last three lines gives the same bits from the same acc.  (torch evaluates
 * eta * acc / den from the left, (eta acc) / den: a last-place difference, not a different update.)
 *
 * Parameters: d_params = pack_actor_critic layout on D inputs (gxu_params_floats);
 * d_c_params = c_net W1[hc][D + A] b1 W2[hc][hc] b2 W3[1][hc] b3 (gxu_q_floats); h, hc in {64, 128, 192, 256},
 * independent of each other.  W2 is read in this layout by the backward pass; d_work holds the forward passes'
 * transposed copies.
 *
 * All `d_*` pointers are DEVICE addresses, dense; fp32 unless said otherwise.  `stream` is a hipStream_t passed as
 * void* (NULL = default stream).  Nothing here throws or synchronises; every call that can fail returns a gxu_status
 * and gxu_last_error() describes the last failure on the calling thread.  This library is separate from the four
 * older ones and carries its own build id.
 */
#ifndef GUARDX_USL_H
#define GUARDX_USL_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gxu_status {
    GXU_OK = 0,
    GXU_ERR_ARG = 1,         /* null pointer, negative count, bad struct_size, t outside [0, T], niter < 0 */
    GXU_ERR_UNSUPPORTED = 2, /* hidden width not in {64, 128, 192, 256}, odd or too wide A, D too wide for the LDS */
    GXU_ERR_HIP = 4          /* a HIP runtime call failed */
} gxu_status;

/* One control step `t` of a T-step call.  Time-major outputs are addressed by the kernel itself (row block t, or
 * t - 1 for the prologue's), so a driver sets `t` and nothing else between launches. */
typedef struct gxu_step_args {
    uint32_t struct_size;     /* sizeof(gxu_step_args) */
    int32_t N, D, A;          /* envs, observation width, action width (even, <= 16) */
    int32_t hidden, c_hidden;
    int32_t env_offset;       /* global index of env 0 (noise counter) */
    int32_t T, t;             /* t in [0, T]; t == T is the tail */
    int32_t correct;          /* 0: the warm-up branch, act_safe = act */
    int32_t niter;            /* passes of the iteration at most (>= 0) */
    uint32_t seed[2];         /* key of the action-noise stream */
    uint32_t step0;           /* policy steps taken before this call (noise counter offset) */
    float delta, eta, grad_scale;
    const float* d_params;    /* gxu_params_floats(D, A, hidden) */
    const float* d_c_params;  /* gxu_q_floats(D, A, c_hidden) */
    const float* d_work;      /* gxu_work_floats(...), filled by gxu_prepare */
    const float* d_obs0;      /* [N][D] observation at entry (read at t == 0) */
    const float* d_obs_rd;    /* [N][D] post-reset_done observation of the step just made (t > 0) */
    const float* d_rew_in;    /* [N] reward, cost, done of the step just made (t > 0) */
    const float* d_cost_in;
    const float* d_done_in;
    float* d_obs;             /* [T][N][D] */
    float* d_act;             /* [T][N][A] */
    float* d_act_safe;        /* [T][N][A] what env.step receives */
    float* d_mu;              /* [T][N][A] */
    float* d_logp;            /* [T][N] */
    float* d_val;             /* [T][N] */
    float* d_qc;              /* [T][N] Q(obs, act) */
    float* d_iters;           /* [T][N] updates applied, as float32 */
    float* d_rew;             /* [T][N] copies of the step's reward / cost / done */
    float* d_cost;
    float* d_done;
    float* d_obs_last;        /* [N][D] */
    float* d_val_last;        /* [N] */
    float* d_logstd;          /* [A] */
} gxu_step_args;

const char* gxu_last_error(void);
/* sha256 (24 hex digits) over the library's sources, headers, flags and compiler (guardx_amd/build.py) */
const char* gxu_build_id(void);

/* floats of the packed actor-critic on D inputs; -1 if unsupported */
int64_t gxu_params_floats(int32_t D, int32_t A, int32_t hidden);
/* floats of the packed c_net on D + A inputs; -1 if unsupported */
int64_t gxu_q_floats(int32_t D, int32_t A, int32_t c_hidden);
/* floats of gxu_policy_step's device workspace (the transposed hidden layers of the three networks); -1 if unsupported */
int64_t gxu_work_floats(int32_t D, int32_t A, int32_t hidden, int32_t c_hidden);
/* floats of gxu_correction_probe's device workspace (c_net's transposed hidden layers); -1 if unsupported */
int64_t gxu_probe_work_floats(int32_t D, int32_t A, int32_t c_hidden);

/* Once per call, before its first gxu_policy_step: transposes the hidden layers into d_work (stream-ordered). */
gxu_status gxu_prepare(int32_t D, int32_t A, int32_t hidden, int32_t c_hidden, const float* d_params,
                       const float* d_c_params, float* d_work, void* stream);

/* One launch over all N envs (see the top of this file).  Arguments are checked before anything is launched;
 * N == 0 launches nothing. */
gxu_status gxu_policy_step(const gxu_step_args* args, void* stream);

/* The per-env bookkeeping of a one-episode rollout, the second argument of guardx_usl_policy_step_episode.  The
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

/* The two entries below carry the library's full name instead of its gxu_ prefix: the set of gxu_ symbols is the
 * library's first ABI, which stays as it was. */
/* The one-episode form of gxu_policy_step (the `usl_one_episode` learner: no reset_done between the steps; the
 * driver's env launch is a plain step and d_obs_rd is the env's plain observation).  Same arguments, same checks,
 * plus the bookkeeping of gx_first_done_state below (null, t_base < 0, a wrong struct_size or a null pointer
 * in it: GXU_ERR_ARG, nothing launched).  Against gxu_policy_step:
 *   the row read has every NaN / +Inf / -Inf entry replaced by +0.0f; that row feeds every network and is what
 *   obs[t] keeps;
 *   the prologue of t > 0 runs the first-done bookkeeping after its copies (gx_first_done_state);
 *   the tail writes obs_last raw and val_last = v on the sanitised row, 0 for a row with any non-finite entry.
 *   The sanitised row is what c_net reads in every pass of the iteration; qc, the correction and iters are
 *   those of gxu_policy_step.
 */
gxu_status guardx_usl_policy_step_episode(const gxu_step_args* args, const gx_first_done_state* book, void* stream);

/* The tail launch of the one-episode form alone on n caller-supplied rows d_rows [n][D] (after gxu_prepare on the
 * same networks): d_obs_last = the rows as they are, d_val_last by the tail's rule.  No state is touched. */
gxu_status guardx_usl_tail_probe(int32_t n, int32_t D, int32_t A, int32_t hidden, int32_t c_hidden, const float* d_params,
                          const float* d_c_params, const float* d_work, const float* d_rows, float* d_obs_last,
                          float* d_val_last, void* stream);

/* The iteration alone, with the step kernel's own device functions, on n caller-supplied rows d_obs [n][D], d_act
 * [n][A]:  d_a_safe [n][A] the final a;  d_q0 [n] Q at the input action;  d_grad0 [n][A] the scaled gradient s of the
 * first pass (s, not the running sum: with niter = 1 the two are the same), 0 for a row that stops before it;
 * d_iters [n] (int32) the updates applied;  d_stop [n] (int32) why the row stopped: 0 niter exhausted, 1 max a > 1,
 * 2 q <= delta.  d_work: gxu_probe_work_floats floats of scratch, filled by this call itself (stream-ordered). */
gxu_status gxu_correction_probe(int32_t n, int32_t D, int32_t A, int32_t c_hidden, const float* d_c_params,
                                float* d_work, const float* d_obs, const float* d_act, float delta, int32_t niter,
                                float eta, float grad_scale, float* d_a_safe, float* d_q0, float* d_grad0,
                                int32_t* d_iters, int32_t* d_stop, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GUARDX_USL_H */
