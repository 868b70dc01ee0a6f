/*
 * guardx_fisher.h -- C ABI of libguardx_fisher.so: the Fisher-vector product of the TRPO-family
 * learners (safe_rl_libX/trpo/trpo.py:386-404: auto_hession_x(kl_div, ac.pi, x) and the cg around
 * it; the same lines of cpo, pcpo, scpo, trpolag, trpoipo, trpofac, apo, pdo, safelayer, usl, lpg)
 * for the diagonal-Gaussian MLP actor (trpo_core.py:110-116, hidden_sizes (64, 64), tanh), on the
 * device, for gfx950.
 *
 * theta and every vector of its length P = A + h D + h + h h + h + A h + A are in the order of
 * ac.pi.parameters(), the order of the learners' flat vectors: log_std[A], W1[h][D], b1[h],
 * W2[h][h], b2[h], W3[A][h], b3[A]; weights row-major [out][in], float32.
 *
 * The Hessian of diagonal_gaussian_kl (trpo_core.py:12-22) at the old policy is J' diag(1/(v + eps)) J / B
 * over the net's parameters plus a diagonal block for log_std; v = exp(2 log_std).  With h1, h2 the
 * tanh activations of row o at theta and (dls, dW1, db1, dW2, db2, dW3, db3) = x, per row:
 *   dh1 = (1 - h1^2) (dW1 o + db1)
 *   dh2 = (1 - h2^2) (dW2 h1 + W2 dh1 + db2)
 *   dmu = dW3 h2 + W3 dh2 + db3
 *   u   = dmu / (v + eps) / B
 *   gW3 += u h2'      gb3 += u
 *   gz2  = (W3' u)(1 - h2^2)     gW2 += gz2 h1'    gb2 += gz2
 *   gz1  = (W2' gz2)(1 - h1^2)   gW1 += gz1 o'     gb1 += gz1
 *   y_ls = c dls,  c = v (-4 v / (v + eps)^2 + 8 v^2 / (v + eps)^3) / 2
 * and y += damping x.  Every product of a 64-row tile of obs is a chain of v_mfma_f32_16x16x4_f32
 * (float32, one fused multiply-add per term; the sums over a layer's inputs -- z, their tangents
 * and dmu -- as four chains, k-step s on chain s mod 4 and the bias on chain 0, added as
 * (c0 + c1) + (c2 + c3)); a workgroup adds its tiles' sums in tile order and
 * writes one partial vector, the partial vectors are added in workgroup order.  No atomics: two
 * calls with the same arguments give the same bits.  1 / ((v + eps) B) and c are evaluated in
 * float64 and rounded once.
 *
 * All `d_*` pointers are DEVICE addresses, dense.  `stream` is a hipStream_t passed as void*
 * (NULL = default stream).  Nothing here throws or synchronises; every call that can fail returns
 * a gxf_status and gxf_last_error() describes the last failure on the calling thread.  This
 * library is separate from libguardx_hip.so and carries its own build id.
 */
#ifndef GUARDX_FISHER_H
#define GUARDX_FISHER_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gxf_status {
    GXF_OK = 0,
    GXF_ERR_ARG = 1,         /* null pointer, B < 1, D < 1, A < 1, iters < 0, n < 0, workgroups outside 0 .. 4096 */
    GXF_ERR_UNSUPPORTED = 2, /* hidden != 64, D > 128, A odd or > 16 */
    GXF_ERR_HIP = 4          /* a HIP runtime call failed */
} gxf_status;

const char* gxf_last_error(void);
/* sha256 (24 hex digits) over the library's sources, headers, flags and compiler (guardx_amd/build.py) */
const char* gxf_build_id(void);

/* P for an actor of observation width D, action width A and hidden width `hidden`; -1 for sizes below 1 */
int64_t gxf_param_count(int32_t D, int32_t A, int32_t hidden);

/* the workgroups a call with `workgroups` == 0 launches: min(256, the 64-row tiles of B rows) */
int32_t gxf_default_workgroups(int32_t B);

/* bytes of the device workspace of gxf_fvp and gxf_cg (one size serves both) for hidden width 64; -1 for
 * arguments that gxf_fvp refuses */
int64_t gxf_work_bytes(int32_t B, int32_t D, int32_t A, int32_t workgroups);

/* d_y[P] = H d_x + damping d_x at d_theta[P] over d_obs (B, D).  `workgroups`: 0, or the size of the
 * grid (workgroup g takes the tiles g, g + workgroups, ...; one that gets none contributes zeros).
 * d_work: gxf_work_bytes(B, D, A, workgroups) bytes, 8-byte aligned, overwritten.  d_y may not
 * alias d_x.  Two launches. */
gxf_status gxf_fvp(int32_t B, int32_t D, int32_t A, int32_t hidden, const float* d_obs, const float* d_theta,
                   const float* d_x, float eps, float damping, int32_t workgroups, void* d_work, float* d_y,
                   void* stream);

/* The learners' cg(Hx, g) (trpo.py:162-178) for `iters` iterations, stream-ordered, then s = x' H x:
 *   x = 0, r = p = g, rr = r.r;   per iteration:  z = H p;  alpha = rr / (p.z + eps);  x += alpha p;
 *   r -= alpha z;  rr' = r.r;  p = r + (rr' / rr) p;  rr = rr';  stop when |p| < eps.
 * The dots are float64 sums of the float32 vectors' products in a fixed order, alpha and rr' / rr are
 * float64, each vector update is rounded once to float32.  The stop is a device flag: from that
 * iteration on every launch leaves x, r and p as they are; rr == 0 stops in the same way, so g = 0
 * gives x = 0 after 0 iterations.  H includes `damping`.
 * d_xhat[P]; d_s: x' (H x); d_rdot: the final rr; d_iters: iterations done.  d_work as for gxf_fvp. */
gxf_status gxf_cg(int32_t B, int32_t D, int32_t A, int32_t hidden, const float* d_obs, const float* d_theta,
                  const float* d_g, float eps, float damping, int32_t iters, int32_t workgroups, void* d_work,
                  float* d_xhat, float* d_s, float* d_rdot, int32_t* d_iters, void* stream);

/* Test infrastructure, like `workgroups`: d_out[i] = the activation the product applies to d_x[i], i < n
 * (the kernel's own tanh: an odd polynomial below |x| = 0.625, the rollouts' tanh above), so that
 * the tests can measure it by itself.  n < 0 and a null pointer are refused, n == 0 launches nothing.
 * One launch. */
gxf_status gxf_tanh_act(int32_t n, const float* d_x, float* d_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GUARDX_FISHER_H */
