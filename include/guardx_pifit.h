/*
 * guardx_pifit.h -- C ABI of libguardx_pifit.so: the actor half of the first-order learners' update(),
 * the fit of the Gaussian MLP actor by Adam on the clipped surrogate
 * (safe_rl_libX/ppo_one_episode/ppo.py:307-316 and the same lines of ppo/ppo_train.py, ppo_runner.py,
 * ppo_isaac.py; espo_one_episode/espo.py:292-301, whose loss is not clipped; a2c/a2c.py:303-307, one
 * step on -(logp adv).mean()):
 *   for i in range(train_pi_iters): pi_optimizer.zero_grad(); loss_pi, pi_info = compute_loss_pi(data)
 *                                   if pi_info['kl'] > target_kl: break
 *                                   loss_pi.backward(); pi_optimizer.step()
 * with pi_optimizer = Adam(ac.pi.parameters(), lr=pi_lr), on the device, for gfx950.
 *
 * theta, g, m and v have P = A + h D + h + h h + h + A h + A entries in the order of
 * ac.pi.parameters(): log_std[A], W1[h][D], b1[h], W2[h][h], b2[h], W3[A][h], b3[A]; weights
 * row-major [out][in], float32.  The batch: obs (B, D), act (B, A), adv (B,), logp_old (B,), float32,
 * dense.
 *
 * Per row x of obs, with a its action, adv its advantage and l its entry of logp_old:
 *   h1 = tanh(W1 x + b1)    h2 = tanh(W2 h1 + b2)    mu = W3 h2 + b3    v1 = exp(2 log_std)
 *   logp  = sum_a -(a - mu)^2 / (2 v1) - log_std - 0.5 log(2 pi)
 *   ratio = exp(logp - l)
 * The three losses, with lo = 1 - clip_ratio and hi = 1 + clip_ratio:
 *   ratio, clipped:    loss = -mean(min(ratio adv, clamp(ratio, lo, hi) adv))
 *   ratio, unclipped:  loss = -mean(ratio adv)
 *   logp:              loss = -mean(logp adv)
 * and kl = mean(l - logp), cf = mean(ratio > hi or ratio < lo) (0 where nothing is clipped),
 * ent = sum_a (log_std + 0.5 + 0.5 log(2 pi)).  The gradient, in closed form, with the row weight
 *   c = -adv ratio active / B      (ratio)          c = -adv / B      (logp)
 * where active = 0 exactly where clamp(ratio, lo, hi) adv < ratio adv, that is where adv > 0 and
 * ratio > hi or adv < 0 and ratio < lo, and 1 elsewhere (without clipping: everywhere).  This is what
 * autograd gives for torch.min of the two branches: inside the range they tie and their halves add to
 * the whole, outside it only the selected branch passes.  From c on:
 *   dlog_std_a = sum c ((a_a - mu_a)^2 / v1_a - 1)
 *   dmu_a = c (a_a - mu_a) / v1_a
 *   dW3 = dmu' h2                 db3 = sum dmu
 *   dz2 = (dmu W3) (1 - h2^2)     dW2 = dz2' h1     db2 = sum dz2
 *   dz1 = (dz2 W2) (1 - h1^2)     dW1 = dz1' x      db1 = sum dz1
 * (sums over the rows).
 *
 * The arithmetic of the forward pass, of logp and of ratio is guardx_pgrad.h's, in the line search's
 * constants and order: float32 chains of v_mfma_f32_16x16x4_f32 over 64-row tiles, the sums over a
 * layer's inputs four chains added as (c0 + c1) + (c2 + c3), the Fisher product's tanh (2.3 ulp),
 * 1 - h^2 = fmaf(-h, h, 1); a row's terms float64 from the float32 mu, logp rounded to float32,
 * ratio = float32(exp(float64(float32(logp - l)))).  lo and hi are float32(1 - clip_ratio) and
 * float32(1 + clip_ratio), the sums taken in float64, and ratio is compared with them in float32, as
 * torch compares a float32 tensor with a Python number.  c = float32(-(adv ratio) / B), or
 * float32(-adv / B), the product and the quotient in float64, and 0 by selection where active = 0;
 * dmu = float32((c da) / v1) in float64; c ((da da) / v1 - 1) is float64 and every sum of it is
 * float64 in a fixed order.  The backward pass from dmu on is guardx_pgrad.h's for one gradient.
 * A row's term of the loss is the float32 min(ratio adv, clamp(ratio) adv) (ratio adv; logp adv), its
 * term of kl the float32 l - logp, of cf 1 or 0; each is summed in float64 in a fixed order (the rows
 * of a lane, the lanes of a wave as a tree, the four waves in wave order, the workgroups in workgroup
 * order) and divided by B in float64.  Rows past B contribute exact zeros by selection and are never
 * read.  No atomics: the same arguments and the same state give the same bits.
 *
 * Adam is guardx_vfit.h's: torch's single-tensor form (no weight decay, no amsgrad), per entry in
 * float64 from the float32 g, m, v, theta, every operation one IEEE operation in the order written:
 *   M = b1 * m + (1 - b1) * g
 *   V = b2 * v + (1 - b2) * (g * g)
 *   T = theta - (lr / (1 - b1^t)) * (M / (sqrt(V) / sqrt(1 - b2^t) + eps))
 * and m = float32(M), v = float32(V), theta = float32(T).  The step count t lives on the device (the
 * host does not know how many steps a call took), counted from 1 over the optimizer's life.  b1^t and
 * b2^t are the bits of Python's b ** t: the caller uploads a table of b1 ** t, b2 ** t for
 * t = 1 .. t_sat, t_sat the first t at which 1 - b1 ** t == 1 and 1 - b2 ** t == 1 in float64, and the
 * kernel reads entry min(t, t_sat): past t_sat both corrections are exactly 1.
 *
 * The loop, for i = 0 .. iters - 1, exactly the learners':
 *   1  loss, kl and cf at the current parameters -> entry i of the three traces
 *   2  if kl > target_kl (in float64; a NaN kl or a NaN target_kl does not stop): stop_iter = i, and
 *      nothing further happens in this call: no step, no count, no trace entry
 *   3  otherwise one Adam step, t = t + 1
 * Two launches per iteration, 2 iters in all whatever the data are: after a stop the remaining
 * launches return at once (the gradient's on a device flag, the step's on the decision it takes again
 * from the same partial sums, which every workgroup of that launch adds for itself in the same order).
 *
 * All `d_*` pointers are DEVICE addresses, dense; `h_*` pointers are HOST addresses, read before the
 * call returns.  Pointers to float64 and int64 data travel as void*.  `stream` is a hipStream_t passed
 * as void* (NULL = default stream).  Nothing here throws or synchronises; every call that can fail
 * returns a gxa_status and gxa_last_error() describes the last failure on the calling thread.  This
 * library is separate from the others and carries its own build id.
 */
#ifndef GUARDX_PIFIT_H
#define GUARDX_PIFIT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gxa_status {
    GXA_OK = 0,
    GXA_ERR_ARG = 1,         /* null pointer, B < 1, D < 1, A < 1, n < 0, iters < 0, t_sat < 1, a loss outside 0 .. 1, a clip_ratio with
                                the logp loss or below 0, workgroups outside 0 .. 4096 */
    GXA_ERR_UNSUPPORTED = 2, /* hidden != 64, D > 128, A odd or > 16 */
    GXA_ERR_HIP = 4          /* a HIP runtime call failed */
} gxa_status;

const char* gxa_last_error(void);
/* sha256 (24 hex digits) over the library's sources, headers, flags and compiler (guardx_amd/build.py) */
const char* gxa_build_id(void);

/* P for an actor of observation width D, action width A and hidden width `hidden`; -1 for sizes below 1 */
int64_t gxa_param_count(int32_t D, int32_t A, int32_t hidden);

/* the workgroups a call with `workgroups` == 0 launches: the 64-row tiles of B rows, at most 256 (one to a CU);
 * 0 for B < 1 */
int32_t gxa_default_workgroups(int32_t B);

/* bytes of the device workspace of gxa_fit and gxa_gradient (one size serves both) for hidden width 64: a partial
 * vector of P float32 (the whole rounded up to a multiple of 8) and 20 float64 per workgroup; -1 for arguments that
 * gxa_gradient refuses */
int64_t gxa_work_bytes(int32_t B, int32_t D, int32_t A, int32_t workgroups);

/* test infrastructure: d_out[i] = the activation's tanh of d_x[i], i < n; n == 0 is legal */
gxa_status gxa_tanh_act(int32_t n, const float* d_x, float* d_out, void* stream);

/* d_g[P] the gradient of the loss at d_theta; d_info: 4 float64, loss, kl, cf, ent.  `loss`: 0 the ratio's, 1 logp's.
 * h_hyper: 1 float64 on the host, clip_ratio, NaN for none (it must be NaN with loss 1).  `workgroups`: 0, or the size
 * of the grid (workgroup g takes the tiles g, g + workgroups, ...; one that gets none contributes zeros).  d_work:
 * gxa_work_bytes(B, D, A, workgroups) bytes, 8-byte aligned, overwritten.  Two launches. */
gxa_status gxa_gradient(int32_t B, int32_t D, int32_t A, int32_t hidden, const float* d_theta, const float* d_obs,
                        const float* d_act, const float* d_adv, const float* d_logp, int32_t loss, void* h_hyper,
                        int32_t workgroups, void* d_work, float* d_g, void* d_info, void* stream);

/* The learners' loop over `iters` iterations: d_theta, d_m, d_v (P entries each) and d_count updated in place.
 * d_count: 2 int64, the optimizer's step count (read at the start of the call, written at every step) and a slot the
 * call keeps its starting value in.  h_hyper: 6 float64 on the host: lr, b1, b2, eps, target_kl (NaN: never stop),
 * clip_ratio (NaN: none).  d_table: 2 t_sat float64, b1 ** t, b2 ** t for t = 1 .. t_sat in turn.  d_trace: 3 iters
 * float64, the traces of loss, kl and cf one after the other; an entry the call does not reach keeps what the caller
 * put there.  d_ctl: 3 int32: the stop flag (the call clears it), stop_iter and steps (the caller puts iters - 1 and
 * 0 there; written at a stop and at every step).  d_last: 4 float64: the last evaluated loss, kl and cf, and ent at
 * the call's first parameters.  iters == 0 launches nothing and changes nothing.  2 iters launches. */
gxa_status gxa_fit(int32_t B, int32_t D, int32_t A, int32_t hidden, float* d_theta, float* d_m, float* d_v, void* d_count,
                   const float* d_obs, const float* d_act, const float* d_adv, const float* d_logp, int32_t iters,
                   int32_t loss, void* h_hyper, void* d_table, int32_t t_sat, int32_t workgroups, void* d_work,
                   void* d_trace, int32_t* d_ctl, void* d_last, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GUARDX_PIFIT_H */
