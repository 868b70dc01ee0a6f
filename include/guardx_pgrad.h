/*
 * guardx_pgrad.h -- C ABI of libguardx_pgrad.so: what opens the TRPO family's update(), the flat
 * gradients of the two surrogate losses over the Gaussian MLP actor
 * (safe_rl_libX/trpo/trpo.py: g = auto_grad(loss_pi, ac.pi); cpo/cpo.py:445-446, which adds
 * b = auto_grad(surr_cost, ac.pi); the same lines of trpolag, trpoipo, trpofac, safelayer, usl, lpg,
 * scpo and pdo) and CPO's step direction (cpo/cpo.py:459-525), on the device, for gfx950.
 *
 * theta, g, b and every direction have P = A + h D + h + h h + h + A h + A entries in the order of
 * ac.pi.parameters(): log_std[A], W1[h][D], b1[h], W2[h][h], b2[h], W3[A][h], b3[A]; weights
 * row-major [out][in], float32.  The batch: obs (B, D), act (B, A), adv (B,), logp_old (B,) and,
 * optionally, adc (B,), float32, dense.
 *
 * Per row x of obs, with a its action, w its weight (adv or adc) and l its entry of logp_old:
 *   h1 = tanh(W1 x + b1)    h2 = tanh(W2 h1 + b2)    mu = W3 h2 + b3    v1 = exp(2 log_std)
 *   logp  = sum_a -(a - mu)^2 / (2 v1) - log_std - 0.5 log(2 pi)
 *   ratio = exp(logp - l)
 * and loss_pi = -mean(ratio adv), surr_cost = mean(ratio adc), approx_kl = mean(l - logp),
 * ent = sum_a (log_std + 0.5 + 0.5 log(2 pi)).  The gradient of either loss, in closed form, with
 *   c = -adv ratio / B  (g)        c = adc ratio / B  (b)
 *   dlog_std_a = sum c ((a_a - mu_a)^2 / v1_a - 1)
 *   dmu_a = c (a_a - mu_a) / v1_a
 *   dW3 = dmu' h2                 db3 = sum dmu
 *   dz2 = (dmu W3) (1 - h2^2)     dW2 = dz2' h1     db2 = sum dz2
 *   dz1 = (dz2 W2) (1 - h1^2)     dW1 = dz1' x      db1 = sum dz1
 * (sums over the rows).  ratio is computed, not taken as 1: the learners differentiate through it at
 * a logp they recompute.
 *
 * The arithmetic is float32: chains of v_mfma_f32_16x16x4_f32 over 64-row tiles.  The sums over a
 * layer's inputs (z1, z2, mu) are four chains, k-step s on chain s mod 4 and the bias on chain 0,
 * added as (c0 + c1) + (c2 + c3); the activation is the Fisher product's tanh (2.3 ulp); 1 - h^2 is
 * fmaf(-h, h, 1).  A row's terms are float64 from the float32 mu, in the line search's words: with
 * i2 = 1 / (2 v1) and da = a - mu, logp = float32(sum_a -(da da) i2 - log_std - 0.5 log(2 pi)), the
 * four lanes of a row adding their actions as (p0 + p1) + (p2 + p3); ratio = float32(exp(float64(
 * float32(logp - l)))).  c = float32(-(adv ratio) / B) and float32((adc ratio) / B), the product and
 * the quotient in float64; dmu = float32((c da) / v1) in float64; c ((da da) / v1 - 1) is float64
 * and every sum of it is float64 in a fixed order.  dmu W3, dz2 W2 and the six sums over a tile's 64
 * rows are single MFMA chains that start from zero.  A tile's sums are added, in float32, to its
 * workgroup's running sums (workgroup g walks the tiles g, g + grid, ... in that order); the
 * workgroups' partial vectors are added in workgroup order in float64 and each gradient is rounded
 * once to float32, as .grad is.  ratio adv, ratio adc (float32 products) and l - logp are summed in
 * float64 in a fixed order; the three means and ent are float64.  Rows past B contribute exact zeros
 * by selection and are never read.  Both gradients come from one forward pass while D <= 72; wider
 * observations take a second pass with adc as the row weight (the same arithmetic).  No atomics: the
 * same arguments give the same bits, and g is the same whether b is asked for or not.
 *
 * CPO's direction, with EPS = 1e-8, every operation float64 in the order written, from the float32
 * vectors b, Hinv_g = cg(Hx, g), approx_g = Hx(Hinv_g), Hinv_b = cg(Hx, b), the float32
 * s = Hinv_b' Hx(Hinv_b) of the second solve, and the float64 c and target_kl:
 *   q = Hinv_g . approx_g      bb = b . b      (sums in a fixed order)
 *   if bb <= 1e-8 and c < 0:   optim_case = 4;  r = s = A = B = 0 and Hinv_b counts as 0
 *   else: r = Hinv_b . approx_g;  A = q - r r / s;  B = 2 target_kl - c c / s;
 *         optim_case = 3 if c < 0 and B < 0, else 2 if c < 0 and B >= 0, else 1 if c >= 0 and
 *         B >= 0, else 0
 *   case 3, 4:  lam = sqrt(q / (2 target_kl)), nu = 0
 *   case 1, 2:  LA = [0, r / c], LB = [r / c, inf], exchanged unless c < 0;
 *               proj(x, L) = max(L0, min(L1, x)), min(u, x) = x if x < u else u, max(l, y) = y if y > l else l;
 *               lam_a = proj(sqrt(A / B), LA), lam_b = proj(sqrt(q / (2 target_kl)), LB),
 *               f_a = -0.5 (A / (lam_a + EPS) + B lam_a) - r c / (s + EPS),
 *               f_b = -0.5 (q / (lam_b + EPS) + 2 target_kl lam_b),
 *               lam = lam_a if f_a >= f_b else lam_b;  nu = max(0, lam c - r) / (s + EPS)
 *   case 0:     lam = 0, nu = sqrt(2 target_kl / (s + EPS))
 *   x_direction = float32((1 / (lam + EPS)) (Hinv_g + nu Hinv_b)) if optim_case > 0, else float32(nu Hinv_b)
 * In case 4 Hinv_b is not read: whatever a solve of a zero b left there cannot reach the output.
 * TRPO's direction is x_direction = float32(sqrt(2 target_kl / (s + EPS)) x_hat).
 *
 * All `d_*` pointers are DEVICE addresses, dense.  Pointers to float64 data travel as void*.
 * `stream` is a hipStream_t passed as void* (NULL = default stream).  Nothing here throws or
 * synchronises; every call that can fail returns a gxg_status and gxg_last_error() describes the last
 * failure on the calling thread.  This library is separate from the others and carries its own build id.
 */
#ifndef GUARDX_PGRAD_H
#define GUARDX_PGRAD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gxg_status {
    GXG_OK = 0,
    GXG_ERR_ARG = 1,         /* null pointer, B < 1, D < 1, A < 1, P < 1, workgroups outside 0 .. 4096 */
    GXG_ERR_UNSUPPORTED = 2, /* hidden != 64, D > 128, A odd or > 16 */
    GXG_ERR_HIP = 4          /* a HIP runtime call failed */
} gxg_status;

const char* gxg_last_error(void);
/* sha256 (24 hex digits) over the library's sources, headers, flags and compiler (guardx_amd/build.py) */
const char* gxg_build_id(void);

/* P for an actor of observation width D, action width A and hidden width `hidden`; -1 for sizes below 1 */
int64_t gxg_param_count(int32_t D, int32_t A, int32_t hidden);

/* the workgroups a call with `workgroups` == 0 launches: the 64-row tiles of B rows, at most 256 (one to a CU);
 * 0 for B < 1 */
int32_t gxg_default_workgroups(int32_t B);

/* bytes of the device workspace of gxg_gradient for hidden width 64 (one size serves the call with and without adc):
 * two partial vectors of P float32 (the whole rounded up to a multiple of 8) and 36 float64 per workgroup; -1 for
 * arguments that gxg_gradient refuses */
int64_t gxg_work_bytes(int32_t B, int32_t D, int32_t A, int32_t workgroups);

/* d_g[P] the gradient of loss_pi and, where d_adc is not null, d_b[P] that of surr_cost, at d_theta; d_info: 4 float64,
 * pi_l, surr_cost (0 without d_adc), approx_kl, ent.  d_adc and d_b are null together.  `workgroups`: 0, or the size of
 * the grid (workgroup g takes the tiles g, g + workgroups, ...; one that gets none contributes zeros).  d_work:
 * gxg_work_bytes(B, D, A, workgroups) bytes, 8-byte aligned, overwritten.  Two launches; three for both
 * gradients at D > 72. */
gxg_status gxg_gradient(int32_t B, int32_t D, int32_t A, int32_t hidden, const float* d_theta, const float* d_obs,
                        const float* d_act, const float* d_adv, const float* d_logp, const float* d_adc, int32_t workgroups,
                        void* d_work, float* d_g, float* d_b, void* d_info, void* stream);

/* CPO's direction from the two solves' results.  d_s: the float32 s of the second solve; d_crit: 2 float64, c and
 * target_kl.  -> d_x[P], d_case[0] (int32 optim_case), d_out: 7 float64, lam nu q r s A B.  One launch of one workgroup. */
gxg_status gxg_cpo_direction(int32_t P, const float* d_b, const float* d_hinv_g, const float* d_hinv_b, const float* d_approx_g,
                             const float* d_s, void* d_crit, float* d_x, int32_t* d_case, void* d_out, void* stream);

/* TRPO's direction: d_x[P] = sqrt(2 target_kl / (s + EPS)) d_x_hat.  d_s: float32; d_target_kl: 1 float64.  One launch. */
gxg_status gxg_trpo_direction(int32_t P, const float* d_x_hat, const float* d_s, void* d_target_kl, float* d_x, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GUARDX_PGRAD_H */
