/*
 * guardx_vfit.h -- C ABI of libguardx_vfit.so: the closing block of the learners' update(), the fit
 * of the value critic (and, for the CPO family, of the cost-value critic) by Adam on the MSE loss
 * (safe_rl_libX/trpo/trpo.py:434-439, cpo/cpo.py:563-576 and the same lines of every other learner:
 *   for i in range(train_v_iters): vf_optimizer.zero_grad(); loss_v = ((ac.v(obs) - ret)**2).mean();
 *                                  loss_v.backward(); vf_optimizer.step()
 * with vf_optimizer = Adam(ac.v.parameters(), lr=vf_lr)) for the MLP critic (trpo_core.py:136-143,
 * hidden_sizes (64, 64), tanh, one linear output), on the device, for gfx950.
 *
 * theta, g, m and v have P = h D + h + h h + h + h + 1 entries in the order of ac.v.parameters():
 * W1[h][D], b1[h], W2[h][h], b2[h], W3[1][h], b3[1]; weights row-major [out][in], float32.  The
 * batch: obs (B, D) and ret (B,), float32, dense.
 *
 * Per row x of obs, with r its entry of ret:
 *   h1 = tanh(W1 x + b1)    h2 = tanh(W2 h1 + b2)    val = W3 h2 + b3    e = val - r
 * and loss = mean(e^2) over the B rows.  The gradient of the loss, in closed form:
 *   dval = 2 e / B
 *   dW3 = sum dval h2             db3 = sum dval
 *   dz2 = dval W3 (1 - h2^2)      dW2 = dz2' h1     db2 = sum dz2
 *   dz1 = (dz2 W2) (1 - h1^2)     dW1 = dz1' x      db1 = sum dz1
 * (sums over the rows).
 *
 * The arithmetic is float32: chains of v_mfma_f32_16x16x4_f32 over 64-row tiles.  The sums over a
 * layer's inputs (z1, z2, val) are four chains, k-step s on chain s mod 4 and the bias on chain 0,
 * added as (c0 + c1) + (c2 + c3); the activation is the Fisher product's tanh (2.3 ulp); 1 - h^2 is
 * fmaf(-h, h, 1).  e is one float32 difference; dval is the float64 product e * (2 / B) rounded once
 * to float32; dz2 = (dval * W3) * (1 - h2^2) in float32; dz2 W2 and the six sums over a tile's 64
 * rows are single MFMA chains that start from zero.  A tile's sums are added, in float32, to its
 * workgroup's running sums (workgroup g walks the tiles g, g + grid, ... in that order); the
 * workgroups' partial vectors are added in workgroup order in float64 and the gradient is rounded
 * once to float32, as .grad is.  e^2 is taken in float64 from the float32 e and every sum of it is
 * float64 in a fixed order (the rows of a lane, the lanes of a wave as a tree, a wave's tiles in tile
 * order, the four waves in wave order, the workgroups in workgroup order); loss is that sum over B,
 * rounded once to float32.  Rows past B contribute exact zeros by selection and are never read.
 * No atomics: the same arguments give the same bits.
 *
 * Adam is torch's single-tensor form (no weight decay, no amsgrad), t counted from 1 over the
 * optimizer's life.  Per entry, in float64 from the float32 g, m, v, theta, every operation one IEEE
 * operation in the order written:
 *   M = b1 * m + (1 - b1) * g
 *   V = b2 * v + (1 - b2) * (g * g)
 *   T = theta - (lr / (1 - b1^t)) * (M / (sqrt(V) / sqrt(1 - b2^t) + eps))
 * and m = float32(M), v = float32(V), theta = float32(T): each is rounded once, for storage (T is
 * formed from M and V before they are rounded).  1 - b1, 1 - b2, lr / (1 - b1^t) and sqrt(1 - b2^t)
 * are float64 too, computed once per step.  b1^t and b2^t are the caller's, float64, in h_hyper.
 *
 * All `d_*` pointers are DEVICE addresses, dense; `h_*` pointers are HOST addresses, read before the
 * call returns.  Pointers to float64 data travel as void*.  `stream` is a hipStream_t passed as void*
 * (NULL = default stream).  Nothing here throws or synchronises; every call that can fail returns a
 * gxv_status and gxv_last_error() describes the last failure on the calling thread.  This library
 * is separate from the others and carries its own build id.
 */
#ifndef GUARDX_VFIT_H
#define GUARDX_VFIT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gxv_status {
    GXV_OK = 0,
    GXV_ERR_ARG = 1,         /* null pointer, B < 1, D < 1, P < 1, n < 0, iters < 0, step0 < 0, workgroups outside 0 .. 4096 */
    GXV_ERR_UNSUPPORTED = 2, /* hidden != 64, D > 128 */
    GXV_ERR_HIP = 4          /* a HIP runtime call failed */
} gxv_status;

const char* gxv_last_error(void);
/* sha256 (24 hex digits) over the library's sources, headers, flags and compiler (guardx_amd/build.py) */
const char* gxv_build_id(void);

/* P for a critic of observation width D and hidden width `hidden`; -1 for sizes below 1 */
int64_t gxv_param_count(int32_t D, int32_t hidden);

/* the workgroups a call with `workgroups` == 0 launches: the 64-row tiles of B rows, at most 256 (one to a CU);
 * 0 for B < 1 */
int32_t gxv_default_workgroups(int32_t B);

/* bytes of the device workspace of gxv_fit and gxv_gradient (one size serves both) for hidden width 64: a partial
 * vector of P float32 (the whole rounded up to a multiple of 8) and one float64 per workgroup; -1 for arguments that
 * gxv_gradient refuses */
int64_t gxv_work_bytes(int32_t B, int32_t D, int32_t workgroups);

/* test infrastructure: d_out[i] = the activation's tanh of d_x[i], i < n; n == 0 is legal */
gxv_status gxv_tanh_act(int32_t n, const float* d_x, float* d_out, void* stream);

/* d_g[P] the gradient and d_loss[0] the loss at d_theta.  `workgroups`: 0, or the size of the grid (workgroup g takes
 * the tiles g, g + workgroups, ...; one that gets none contributes zeros).  d_work: gxv_work_bytes(B, D, workgroups)
 * bytes, 8-byte aligned, overwritten.  Two launches. */
gxv_status gxv_gradient(int32_t B, int32_t D, int32_t hidden, const float* d_theta, const float* d_obs, const float* d_ret,
                        int32_t workgroups, void* d_work, float* d_g, float* d_loss, void* stream);

/* test infrastructure: one Adam step of d_theta, d_m, d_v (P entries each, updated in place) from the float32 gradient
 * d_g.  h_hyper: 6 float64 on the host: lr, b1, b2, eps, b1^t, b2^t.  One launch. */
gxv_status gxv_adam_step(int32_t P, float* d_theta, float* d_m, float* d_v, const float* d_g, void* h_hyper, void* stream);

/* The learners' loop: `iters` times the gradient at d_theta and one Adam step of d_theta, d_m, d_v in place.
 * d_loss[i], i < iters, is the loss at the parameters before step i.  `step0`: the steps the optimizer has taken
 * before this call, so that step i has t = step0 + 1 + i.  h_hyper: 4 + 2 iters float64 on the host: lr, b1, b2, eps,
 * then b1^t, b2^t for each step in turn.  iters == 0 launches nothing and changes nothing.  2 iters launches. */
gxv_status gxv_fit(int32_t B, int32_t D, int32_t hidden, float* d_theta, float* d_m, float* d_v, int64_t step0,
                   const float* d_obs, const float* d_ret, int32_t iters, void* h_hyper, int32_t workgroups, void* d_work,
                   float* d_loss, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GUARDX_VFIT_H */
