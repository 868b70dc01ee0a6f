/*
 * guardx_episode.h -- C ABI of libguardx_episode.so: the per-control-step policy launch of the one-episode
 * rollout and the one-episode buffer's finish_path + get, for gfx950.  The `*_one_episode` learners
 * (safe_rl_libX/trpo_one_episode/trpo.py:450-545, cpo_one_episode/cpo.py:619-708) never call reset_done():
 * an env that finishes keeps being stepped, the learner remembers per env the first step at which `done`
 * was 1 and uses the rows before it only.  One gxe_policy_step launch per control step does
 *
 *   prologue (the bookkeeping of the step just made, skipped at t == 0), per env, in this order:
 *       rew / cost / done [t-1] = the step's (copied);  k = t_base + t  (the step's 1-based index in the episode)
 *       first_done == 0 ?  ep_ret += rew, ep_cost += cost (fp32, one add each), ep_len = k
 *       done > 0 and first_done == 0 ?  first_done = k
 *     so the reward and the cost of the step that finishes an env are counted (trpo.py:473-501).
 *   body: row = d_obs_rd (d_obs0 at t == 0) with every NaN / +Inf / -Inf entry replaced by +0.0f
 *       (trpo.py:453-454) -> obs[t]; mu_net, v_net and, with has_vc, the cost critic vc (identity output) on
 *       that row; act = mu + exp(log_std) z with z from the Threefry block at
 *       (env_offset + env, 16 (step0 + t) + pair) -> act, mu, logp, val, vc [t]  (and logstd)
 *   tail (t == T): the prologue for step T - 1, then obs_last = the row as it is (NOT sanitised), val_last
 *       and vc_last = the critics on the sanitised row, 0 for a row with any non-finite entry; no action, no
 *       noise.  (The reference's intent at trpo.py:513-521; as written its second filter makes the scatter
 *       fail on a shape mismatch once an Inf row occurs.)
 *
 * The arithmetic is the fused rollout's (guardx_amd/csrc/gx_policy.h, oracle/gx_oracle.c:mlp_forward):
 *   hidden unit j:  acc = b[j]; acc = fmaf(x[k], W[j][k], acc) for k = 0, 1, ...; then gx tanh
 *   output:         16 partials, partial l = fmaf chain from 0 over the units 64 c + 4 l + j, folded by a
 *                   butterfly (xor 8, 4, 2, 1); b3 + sum
 *
 * Parameters: d_params = pack_actor_critic layout on D inputs,
 *   pi{W1[h][D] b1 W2[h][h] b2 W3[A][h] b3} v{.. W3[1][h] b3} log_std[A]   (gxe_params_floats)
 * d_vc_params = one critic W1[hc][D] b1 W2[hc][hc] b2 W3[1][hc] b3 (gxe_vc_floats); h, hc in
 * {64, 128, 192, 256}.  Without a cost critic (has_vc == 0) the caller passes the value network's block
 * (d_params + the actor's floats) and vc_hidden = hidden: the third network's slot is prepared as usual and
 * the kernel leaves it idle.
 *
 * gxe_finish is the one-episode buffer's finish_path + get (trpo.py:67-132, cpo.py:72-156) on the
 * time-major tensors of a whole episode (t_base == 0), in two launches.  Per env, with
 * L = first_done ? min(first_done, T) : T and b = first_done ? 0 : val_last:
 *   for t = L - 1 .. 0:  delta = (rew[t] + gamma32 v[t + 1]) - val[t] in fp32 (v[L] = b);
 *                        a = delta + gamma lam a;  r = rew[t] + gamma r in fp64 from a = 0, r = b;
 *                        (gamma and lam are the fp32 arguments, widened; their product is taken in fp64)
 *                        adv[t] = (float)a, ret[t] = (float)r, s += adv[t] (fp32);  adv = ret = 0 on [L, T)
 *   mean = s / T;  q = sum over t = 0 .. T - 1 ascending of (adv[t] - mean)^2, the zeros included;
 *   sd = sqrt(q / T);  adv[t] = (adv[t] - mean) / sd   (no guard on sd == 0, mpi_tools.py:81-86)
 * and the same on cost, vc, vc_last when a cost channel is given, centred only (cpo.py:133-137).  The
 * valid rows of env e are [0, L_e): row t of env e goes to output row (sum of L over the envs before e) + t,
 * the order x.view(N T, .)[valid] gives on env-major buffers.  Rows past the total are not written.
 *
 * All `d_*` pointers are DEVICE addresses, fp32 (int32 where the type says so), dense.  `stream` is a
 * hipStream_t passed as void* (NULL = default stream).  Nothing here throws or synchronises; every call
 * that can fail returns a gxe_status and gxe_last_error() describes the last failure on the calling
 * thread.  This library is separate from libguardx_hip.so and the other side libraries and carries its
 * own build id.
 */
#ifndef GUARDX_EPISODE_H
#define GUARDX_EPISODE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gxe_status {
    GXE_OK = 0,
    GXE_ERR_ARG = 1,         /* null pointer, negative count, bad struct_size, t outside [0, T], t_base < 0 */
    GXE_ERR_UNSUPPORTED = 2, /* hidden width not in {64, 128, 192, 256}, odd or too wide A, D too wide for the LDS */
    GXE_ERR_HIP = 4          /* a HIP runtime call failed */
} gxe_status;

/* One control step `t` of a T-step call.  Time-major outputs are addressed by the kernel itself (row
 * block t, or t - 1 for the prologue's), so a driver sets `t` and nothing else between launches. */
typedef struct gxe_step_args {
    uint32_t struct_size;     /* sizeof(gxe_step_args) */
    int32_t N, D, A;          /* envs, observation width, action width (even, <= 16) */
    int32_t hidden, vc_hidden;
    int32_t has_vc;           /* 0: no cost critic; d_vc_params is a stand-in, d_vc / d_vc_last are not touched */
    int32_t env_offset;       /* global index of env 0 (noise counter) */
    int32_t T, t;             /* t in [0, T]; t == T is the tail */
    int32_t t_base;           /* steps of the episode made before this call (>= 0) */
    uint32_t seed[2];         /* key of the action-noise stream */
    uint32_t step0;           /* policy steps taken before this call (noise counter offset) */
    const float* d_params;    /* gxe_params_floats(D, A, hidden) */
    const float* d_vc_params; /* the cost critic, identity output (has_vc == 0: the value network's block) */
    const float* d_work;      /* gxe_work_floats(...), filled by gxe_prepare */
    const float* d_obs0;      /* [N][D] observation at entry (read at t == 0) */
    const float* d_obs_rd;    /* [N][D] the env's plain observation of the step just made (t > 0): no reset_done
                                 is involved; the field keeps the name the step libraries share */
    const float* d_rew_in;    /* [N] reward, cost, done of the step just made (t > 0) */
    const float* d_cost_in;
    const float* d_done_in;
    int32_t* d_first_done;    /* [N] state: 1-based index of the first step with done, 0 = not finished */
    float* d_ep_ret;          /* [N] state: reward summed up to and including the first done step */
    float* d_ep_cost;         /* [N] state: cost likewise */
    int32_t* d_ep_len;        /* [N] state: steps counted into ep_ret / ep_cost */
    float* d_obs;             /* [T][N][D] the sanitised rows */
    float* d_act;             /* [T][N][A] */
    float* d_mu;              /* [T][N][A] */
    float* d_logp;            /* [T][N] */
    float* d_val;             /* [T][N] */
    float* d_vc;              /* [T][N] (has_vc) */
    float* d_rew;             /* [T][N] copies of the step's reward / cost / done */
    float* d_cost;
    float* d_done;
    float* d_obs_last;        /* [N][D] raw */
    float* d_val_last;        /* [N] */
    float* d_vc_last;         /* [N] (has_vc) */
    float* d_logstd;          /* [A] */
} gxe_step_args;

const char* gxe_last_error(void);
/* sha256 (24 hex digits) over the library's sources, headers, flags and compiler (guardx_amd/build.py) */
const char* gxe_build_id(void);

/* floats of the packed actor-critic on D inputs; -1 if unsupported */
int64_t gxe_params_floats(int32_t D, int32_t A, int32_t hidden);
/* floats of a packed cost critic on D inputs; -1 if unsupported */
int64_t gxe_vc_floats(int32_t D, int32_t vc_hidden);
/* floats of the device workspace (the transposed hidden layers of the three networks); -1 if unsupported */
int64_t gxe_work_floats(int32_t D, int32_t A, int32_t hidden, int32_t vc_hidden);

/* Once per call, before its first gxe_policy_step: transposes the hidden layers into d_work (stream-ordered). */
gxe_status gxe_prepare(int32_t D, int32_t A, int32_t hidden, int32_t vc_hidden, const float* d_params,
                       const float* d_vc_params, float* d_work, void* stream);

/* One launch over all N envs (see the top of this file).  Arguments are checked before anything is launched;
 * N == 0 launches nothing. */
gxe_status gxe_policy_step(const gxe_step_args* args, void* stream);

/* The tail launch alone on n caller-supplied rows d_rows [n][D] (after gxe_prepare on the same networks):
 * d_obs_last = the rows as they are, d_val_last / d_vc_last (has_vc) by the tail's rule.  No state is touched. */
gxe_status gxe_tail_probe(int32_t n, int32_t D, int32_t A, int32_t hidden, int32_t vc_hidden, int32_t has_vc,
                          const float* d_params, const float* d_vc_params, const float* d_work, const float* d_rows,
                          float* d_obs_last, float* d_val_last, float* d_vc_last, void* stream);

/* floats of gxe_finish's workspace; -1 for N < 0 or T < 1 */
int64_t gxe_finish_work_floats(int32_t N, int32_t T);

/* finish_path + get of the one-episode buffer (see the top of this file).  Inputs: the time-major tensors of
 * a call with t_base == 0 and d_first_done [N] after it (read only).  d_cost, d_vc, d_vc_last, d_cost_ret and
 * d_adc are all given or all null (no cost channel).  Outputs hold N T rows each, of which the first
 * *d_n_valid are written, env-major: d_obs_c [.][D], d_act_c, d_mu_c [.][A], d_logp_c, d_ret, d_adv (and
 * d_cost_ret, d_adc) [.].  N == 0 writes *d_n_valid = 0. */
gxe_status gxe_finish(int32_t N, int32_t T, int32_t D, int32_t A, float gamma, float lam, int32_t* d_first_done,
                      const float* d_obs, const float* d_act, const float* d_mu, const float* d_logp,
                      const float* d_rew, const float* d_val, const float* d_val_last, const float* d_cost,
                      const float* d_vc, const float* d_vc_last, float* d_work, float* d_obs_c, float* d_act_c,
                      float* d_mu_c, float* d_logp_c, float* d_ret, float* d_adv, float* d_cost_ret, float* d_adc,
                      int32_t* d_n_valid, void* stream);

/* (guardx_episode_finish_cols below carries the library's full name instead of its gxe_ prefix: the set of gxe_ symbols
 * is the library's first ABI, which stays as it was.)
 * One extra column of guardx_episode_finish_cols: d_src [T][N][width] time-major -> d_dst [.][width], the valid rows compacted
 * env-major like every other output. */
#define GXE_FINISH_MAX_COLS 4
typedef struct gxe_finish_col {
    const float* d_src;
    float* d_dst;
    int32_t width;            /* >= 1 */
} gxe_finish_col;

/* gxe_finish (same arguments, same arithmetic, same two launches) plus, in the gather launch:
 *   n_cols (0 .. GXE_FINISH_MAX_COLS) extra columns `cols` (a HOST array, read before the call returns);
 *   with d_qc, d_qcost [T][N] and d_targetc [.] (all given or all null), per valid row t of env e
 *       targetc = qcost[t] + gamma * qc[t + 1]   one fp32 multiply, then one fp32 add, no fused multiply-add;
 *       the product is taken as +0.0f at t + 1 == L (usl_one_episode/usl.py:105-107: qc counts as 0 there).
 * The one-episode buffers of the safelayer, USL and LPG learners (safelayer_one_episode/safelayer.py:30-140,
 * usl_one_episode/usl.py:22-144): act_safe, cost, prev_cost columns, or act_safe, cost and targetc. */
gxe_status guardx_episode_finish_cols(int32_t N, int32_t T, int32_t D, int32_t A, float gamma, float lam, int32_t* d_first_done,
                           const float* d_obs, const float* d_act, const float* d_mu, const float* d_logp,
                           const float* d_rew, const float* d_val, const float* d_val_last, const float* d_cost,
                           const float* d_vc, const float* d_vc_last, float* d_work, float* d_obs_c, float* d_act_c,
                           float* d_mu_c, float* d_logp_c, float* d_ret, float* d_adv, float* d_cost_ret, float* d_adc,
                           int32_t n_cols, const gxe_finish_col* cols, const float* d_qc, const float* d_qcost,
                           float* d_targetc, int32_t* d_n_valid, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GUARDX_EPISODE_H */
