/*
 * guardx_linesearch.h -- C ABI of libguardx_linesearch.so: the backtracking line search of the
 * TRPO-family learners (safe_rl_libX/trpo/trpo.py:406-431 and the same lines of trpolag, trpoipo,
 * trpofac, safelayer, usl, lpg and their _one_episode forms; cpo/cpo.py:527-560, scpo and pdo with
 * the cost condition) for the diagonal-Gaussian MLP actor (trpo_core.py:110-133, hidden_sizes
 * (64, 64), tanh), on the device, for gfx950.
 *
 * theta and d have P = A + h D + h + h h + h + A h + A entries in the order of ac.pi.parameters(),
 * the order of the learners' flat vectors: log_std[A], W1[h][D], b1[h], W2[h][h], b2[h], W3[A][h],
 * b3[A]; weights row-major [out][in], float32.  The batch: obs (B, D), act (B, A), adv (B,),
 * logp_old (B,), mu_old (B, A), logstd_old (B, A) (the per-row copies the learners' buffers hold)
 * and, optionally, adc (B,); float32, dense.
 *
 * The candidate for a step size t (a float64):
 *   theta_t[i] = float32(double(theta[i]) - t * double(d[i])),
 * one product and one difference in float64, rounded once: what numpy's float32 - float64 * float64
 * gives once it is assigned to float32 parameters; at t = 0 the candidate is theta itself, whatever d
 * holds.  The learners' t_j = coeff ** j are computed by
 * the caller, in float64, and passed as an array on the HOST that is read before the call returns.
 *
 * Per row, with mu = mu_net_t(obs), ls the candidate's log_std, v1 = exp(2 ls), v0 = exp(2 logstd_old),
 * EPS = 1e-8:
 *   kl_row = sum_a 0.5 (((mu - mu_old)^2 + v0) / (v1 + EPS) - 1) + ls - logstd_old
 *            (diagonal_gaussian_kl(mu_old, logstd_old, mu, ls), trpo_core.py:12-22, the order of _d_kl)
 *   logp   = sum_a -(act - mu)^2 / (2 v1) - ls - 0.5 log(2 pi)
 *   ratio  = exp(logp - logp_old)
 * and the four means over the B rows, in this order wherever four values stand together:
 *   kl = mean(kl_row)   pi_l = -mean(ratio adv)   surr_cost = mean(ratio adc)   approx_kl = mean(logp_old - logp)
 * (surr_cost is 0 without adc).
 *
 * mu is float32: chains of v_mfma_f32_16x16x4_f32 over 64-row tiles, the sums over a layer's inputs
 * as four chains, k-step s on chain s mod 4 and the bias on chain 0, added as (c0 + c1) + (c2 + c3);
 * the activation is the Fisher product's tanh (2.3 ulp).  The terms of a row are then evaluated in
 * float64 from the float32 inputs (1 / (v1 + EPS) and 1 / (2 v1) once per candidate, the exponentials
 * in float64) and each of the four row values kl_row, ratio adv, ratio adc and logp_old - logp is
 * rounded once to float32; logp is rounded to float32 before logp_old is subtracted, the difference
 * is taken in float32, and ratio is the float64 exponential of it rounded to float32 (relative
 * error 2^-24 plus the exponential's own, below 2^-50).  Every sum over rows is float64 in a fixed order:
 * the 16 rows of a wave's quarter of a tile (a fixed tree), a wave's tiles in tile order, the four
 * waves of a workgroup in wave order, the workgroups' partials in workgroup order.  Rows past B
 * contribute exact zeros by selection and are never read.  No atomics: the same arguments give the
 * same bits.
 *
 * All `d_*` pointers are DEVICE addresses, dense; `h_*` pointers are HOST addresses.  Pointers to
 * float64 data travel as void*.  `stream` is a hipStream_t passed as void* (NULL = default stream).
 * Nothing here throws or synchronises; every call that can fail returns a gxb_status and
 * gxb_last_error() describes the last failure on the calling thread.  This library is separate
 * from the others and carries its own build id.
 */
#ifndef GUARDX_LINESEARCH_H
#define GUARDX_LINESEARCH_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gxb_status {
    GXB_OK = 0,
    GXB_ERR_ARG = 1,         /* null pointer, B < 1, D < 1, A < 1, iters < 0, n_steps < 1, workgroups outside 0 .. 4096 */
    GXB_ERR_UNSUPPORTED = 2, /* hidden != 64, D > 128, A odd or > 16 */
    GXB_ERR_HIP = 4          /* a HIP runtime call failed */
} gxb_status;

const char* gxb_last_error(void);
/* sha256 (24 hex digits) over the library's sources, headers, flags and compiler (guardx_amd/build.py) */
const char* gxb_build_id(void);

/* P for an actor of observation width D, action width A and hidden width `hidden`; -1 for sizes below 1 */
int64_t gxb_param_count(int32_t D, int32_t A, int32_t hidden);

/* the workgroups a call with `workgroups` == 0 launches: the 64-row tiles of B rows, at most 512 for D <= 64 (two
 * workgroups share a CU) and at most 256 above; 0 for sizes below 1 */
int32_t gxb_default_workgroups(int32_t B, int32_t D);

/* bytes of the device workspace of gxb_evaluate and gxb_search (one size serves both) for hidden width 64:
 * 32 per workgroup and 32 of state; -1 for arguments that gxb_evaluate refuses */
int64_t gxb_work_bytes(int32_t B, int32_t D, int32_t A, int32_t workgroups);

/* d_out (n_steps, 4) float64: the four means at each of the step sizes h_steps[0 .. n_steps - 1] (float64,
 * host), unconditionally.  d_adc may be null.  `workgroups`: 0, or the size of the grid (workgroup g takes
 * the tiles g, g + workgroups, ...; one that gets none contributes zeros).  d_work: gxb_work_bytes(B, D, A,
 * workgroups) bytes, 8-byte aligned, overwritten.  Two launches per step. */
gxb_status gxb_evaluate(int32_t B, int32_t D, int32_t A, int32_t hidden, const float* d_theta, const float* d_dir,
                        const float* d_obs, const float* d_act, const float* d_adv, const float* d_logp_old,
                        const float* d_mu_old, const float* d_logstd_old, const float* d_adc, int32_t n_steps,
                        void* h_steps, int32_t workgroups, void* d_work, void* d_out, void* stream);

/* The learners' loop.  The batch is evaluated at t = 0, which gives pi_l_old and surr_cost_old (their
 * compute_loss_pi(data, ac.pi) and compute_cost_pi(data, ac.pi)), then at h_steps[j], j = 0 .. iters - 1, in
 * turn.  The means are rounded to float32, as the .item() of a float32 tensor is, and the first j with
 *   kl <= target_kl  and  (need_loss == 0 or pi_l <= pi_l_old)  and  (no adc or surr_cost - surr_cost_old <= cost_margin)
 * is accepted: IEEE comparisons in float64, so a NaN anywhere rejects.  d_criteria: 3 float64 on the device,
 * target_kl, cost_margin, need_loss.  Acceptance sets a flag on the device, and every later launch of the
 * call sees it and does nothing.
 *   d_theta_new[P]  theta_j of the accepted candidate, bit for bit what the evaluation used; theta itself if
 *                   none was accepted or iters == 0.  May not alias d_theta or d_dir.
 *   d_accepted      j, or -1
 *   d_means         6 float64, not rounded: kl, pi_l, surr_cost, approx_kl at the accepted candidate (at t = 0
 *                   if none was), then pi_l_old and surr_cost_old
 *   d_trace         (iters + 1, 4) float64: row 0 the means at t = 0, row j + 1 those of candidate j.  Only the
 *                   rows of evaluated candidates are written; the caller fills the rest beforehand.
 * 2 + 2 iters launches. */
gxb_status gxb_search(int32_t B, int32_t D, int32_t A, int32_t hidden, const float* d_theta, const float* d_dir,
                      const float* d_obs, const float* d_act, const float* d_adv, const float* d_logp_old,
                      const float* d_mu_old, const float* d_logstd_old, const float* d_adc, int32_t iters,
                      void* h_steps, void* d_criteria, int32_t workgroups, void* d_work, float* d_theta_new,
                      int32_t* d_accepted, void* d_means, void* d_trace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GUARDX_LINESEARCH_H */
