/*
 * guardx_cfit.h -- C ABI of libguardx_cfit.so: the fit of the safety critics of the safelayer, USL,
 * LPG and SCPO learners by Adam on a row-weighted squared loss, on the device, for gfx950:
 *   usl / lpg  (usl/usl.py:378-383, 449-454; lpg/lpg.py:386-391, 457-462):
 *              ((Softplus(c_net(cat(obs, act_safe))) - targetc)**2).mean()
 *   safelayer  (safelayer/safelayer.py:384-418, 483-488): mse(g_net(obs).act_safe + prev_cost, cost)
 *              over a down-sampled batch
 *   scpo       (scpo/scpo.py:419-450): ((Softplus(v_net(cat(obs, M))) - cost_ret)**2).mean(), down-sampled
 * each `train_ccritic_iters` rounds of zero_grad / backward / Adam.step, for the MLP of hidden_sizes
 * (64, 64) with tanh.
 *
 * theta, g, m and v have P = h Din + h + h h + h + A h + A entries in the order of the module's
 * parameters(): W1[h][Din], b1[h], W2[h][h], b2[h], W3[A][h], b3[A]; weights row-major [out][in],
 * float32.  A = 1 for the heads with one output.  The batch: x (B, Din), y (B,), and for the head
 * GXQ_HEAD_DOT act (B, A) and offset (B,), float32, dense; the row weights w are (B,) (w_stride 0)
 * or one (B,) row per iteration (w_stride B), or null: every w_i = 1.
 *
 * Per row x, with h1 = tanh(W1 x + b1), h2 = tanh(W2 h1 + b2), z = W3 h2 + b3:
 *   GXQ_HEAD_IDENTITY  f = z                          f' = 1
 *   GXQ_HEAD_SOFTPLUS  f = Softplus(z)                f' = Softplus'(z)   (the rollout kernels' own two
 *                      functions: beta 1, threshold 20, gxq_softplus_probe shows them)
 *   GXQ_HEAD_DOT       f = sum_a z_a act_a + offset   df/dz_a = act_a
 * and with e = f - y, W = sum_i w_i:
 *   loss = sum_i w_i e_i^2 / W          dz_i = 2 w_i e_i f'(z_i) / W
 *   dW3 = sum dz' h2              db3 = sum dz
 *   dz2 = (dz W3)(1 - h2^2)       dW2 = dz2' h1     db2 = sum dz2
 *   dz1 = (dz2 W2)(1 - h1^2)      dW1 = dz1' x      db1 = sum dz1
 *
 * A row with w_i == 0 is selected out, never multiplied out: its x is replaced by zeros before the
 * first product, its dz and its terms of the loss and of W are exact zeros, whatever its x, y, act
 * and offset hold (NaN and Inf included).  Rows past B are the same, and are never read.
 * W == 0 (no live row) is the mean of an empty selection: the loss and every entry of the gradient
 * are 0 / 0 = NaN, and Adam carries the NaN into theta, m and v.  The reference does the same.
 *
 * The arithmetic is float32: chains of v_mfma_f32_16x16x4_f32 over 64-row tiles, as in
 * guardx_vfit.h (the one-output heads) and guardx_pgrad.h (GXQ_HEAD_DOT, the 16-column head): four
 * chains per forward sum added as (c0 + c1) + (c2 + c3), the Fisher product's tanh, 1 - h^2 =
 * fmaf(-h, h, 1).  GXQ_HEAD_DOT forms sum_a z_a act_a + offset in float64 and rounds it once.  e is
 * one float32 difference; the row's dz before the division by W is the float64 product
 * ((2 w) e) f' (or ((2 w) e) act_a) rounded once to float32.  A tile's sums start from zero and are
 * added in float32 to the workgroup's running sums; the workgroups' partial vectors are added in
 * workgroup order in float64, divided by W in float64 and rounded once to float32.  w e^2 and w are
 * float64 from the float32 values and every sum of them is float64 in a fixed order (a lane's rows,
 * the lanes of a wave as a tree, the four waves in wave order, the workgroups in workgroup order).
 * No atomics: the same arguments give the same bits.
 *
 * Adam is that of guardx_vfit.h, operation for operation (torch's single-tensor form, float64 per
 * entry from the float32 g, m, v, theta, each rounded once for storage; b1^t and b2^t are the
 * caller's, in h_hyper).
 *
 * All `d_*` pointers are DEVICE addresses, dense; `h_*` pointers are HOST addresses, read before the
 * call returns.  Pointers to float64 data travel as void*.  `stream` is a hipStream_t passed as void*
 * (NULL = default stream).  Nothing here throws or synchronises; every call that can fail returns a
 * gxq_status and gxq_last_error() describes the last failure on the calling thread.  This library
 * is separate from the others and carries its own build id.
 */
#ifndef GUARDX_CFIT_H
#define GUARDX_CFIT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gxq_status {
    GXQ_OK = 0,
    GXQ_ERR_ARG = 1,         /* null pointer, B < 1, Din < 1, A < 1, n < 0, iters < 0, step0 < 0, workgroups outside 0 .. 4096,
                                an unknown head, w_stride other than 0 and B */
    GXQ_ERR_UNSUPPORTED = 2, /* hidden != 64, Din > 128, A != 1 for a one-output head, A odd or above 16 for GXQ_HEAD_DOT */
    GXQ_ERR_HIP = 4          /* a HIP runtime call failed */
} gxq_status;

typedef enum gxq_head {
    GXQ_HEAD_IDENTITY = 0,
    GXQ_HEAD_SOFTPLUS = 1,
    GXQ_HEAD_DOT = 2
} gxq_head;

const char* gxq_last_error(void);
/* sha256 (24 hex digits) over the library's sources, headers, flags and compiler (guardx_amd/build.py) */
const char* gxq_build_id(void);

/* P for input width Din, A outputs and hidden width `hidden`; -1 for sizes below 1 */
int64_t gxq_param_count(int32_t Din, int32_t A, int32_t hidden);

/* the workgroups a call with `workgroups` == 0 launches: the 64-row tiles of B rows, at most 256 (one to a CU);
 * 0 for B < 1 */
int32_t gxq_default_workgroups(int32_t B);

/* bytes of the device workspace of gxq_fit and gxq_gradient (one size serves both) for hidden width 64: a partial
 * vector of P float32 per workgroup (the whole rounded up to a multiple of 8) and two float64 per workgroup; -1 for
 * arguments that gxq_gradient refuses */
int64_t gxq_work_bytes(int32_t B, int32_t Din, int32_t A, int32_t head, int32_t workgroups);

/* test infrastructure: d_f[i] = Softplus(d_x[i]) and d_df[i] = Softplus'(d_x[i]) as the kernel evaluates them, i < n;
 * n == 0 is legal */
gxq_status gxq_softplus_probe(int32_t n, const float* d_x, float* d_f, float* d_df, void* stream);

/* d_g[P] the gradient, d_loss[0] the loss (float32) and d_wsum[0] = W (float64) at d_theta.  d_w may be null (every
 * weight 1); d_act is read for GXQ_HEAD_DOT alone, where d_offset may be null (zeros).  `workgroups`: 0, or the size
 * of the grid (workgroup g takes the tiles g, g + workgroups, ...; one that gets none contributes zeros).  d_work:
 * gxq_work_bytes(...) bytes, 8-byte aligned, overwritten.  Two launches. */
gxq_status gxq_gradient(int32_t B, int32_t Din, int32_t A, int32_t hidden, int32_t head, const float* d_theta, const float* d_x,
                        const float* d_y, const float* d_w, const float* d_act, const float* d_offset, int32_t workgroups,
                        void* d_work, float* d_g, float* d_loss, void* d_wsum, void* stream);

/* The learners' loop: `iters` times the gradient at d_theta and one Adam step of d_theta, d_m, d_v in place.
 * Iteration i reads the weights d_w + i * w_stride (w_stride 0: one (B,) weight for every round; w_stride B: an
 * (iters, B) table).  d_loss[i] and d_wsum[i] (float64), i < iters, are the loss and W at the parameters before step i.
 * `step0`: the steps the optimizer has taken before this call.  h_hyper: 4 + 2 iters float64 on the host: lr, b1, b2,
 * eps, then b1^t, b2^t for each step in turn.  iters == 0 launches nothing and changes nothing.  2 iters launches. */
gxq_status gxq_fit(int32_t B, int32_t Din, int32_t A, int32_t hidden, int32_t head, float* d_theta, float* d_m, float* d_v,
                   int64_t step0, const float* d_x, const float* d_y, const float* d_w, int64_t w_stride, const float* d_act,
                   const float* d_offset, int32_t iters, void* h_hyper, int32_t workgroups, void* d_work, float* d_loss,
                   void* d_wsum, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GUARDX_CFIT_H */
