/*
 * guardx_critic.h -- C ABI of libguardx_critic.so: a batched two-hidden-layer tanh critic
 * (the cost critic `ac.vc` of the CPO-family learners, safe_rl_libX/cpo/cpo_core.py) over rows
 * of observations on the device, for gfx950.
 *
 * The arithmetic is the one the fused rollout's value head uses (guardx_amd/csrc/gx_policy.h,
 * oracle/gx_oracle.c:mlp_forward), so Vc(row) has the bits the in-kernel critic would give for
 * the same weights:
 *   hidden unit j:  acc = b[j]; acc = fmaf(x[k], W[j][k], acc) for k = 0, 1, ...; then gx tanh
 *   output:         16 partials, partial l = fmaf chain from 0 over the units 64 c + 4 l + j
 *                   (c = 0 .. h/64 - 1, j = 0 .. 3), folded by a butterfly (xor 8, 4, 2, 1); b3 + sum
 *
 * Parameters: one critic in torch layout W1[h][D] b1[h] W2[h][h] b2[h] W3[1][h] b3[1]
 * (gxc_critic_floats(D, h) floats), h in {64, 128, 192, 256}.
 *
 * All `d_*` pointers are DEVICE addresses, fp32, dense.  `stream` is a hipStream_t passed as
 * void* (NULL = default stream).  Nothing here throws or synchronises; every call that can
 * fail returns a gxc_status and gxc_last_error() describes the last failure on the calling
 * thread.  This library is separate from libguardx_hip.so and carries its own build id.
 */
#ifndef GUARDX_CRITIC_H
#define GUARDX_CRITIC_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gxc_status {
    GXC_OK = 0,
    GXC_ERR_ARG = 1,         /* null pointer, negative count, D < 1 */
    GXC_ERR_UNSUPPORTED = 2, /* hidden width not in {64, 128, 192, 256}, or D too wide for the LDS */
    GXC_ERR_HIP = 4          /* a HIP runtime call failed */
} gxc_status;

const char* gxc_last_error(void);
/* sha256 (24 hex digits) over the library's sources, headers, flags and compiler (guardx_amd/build.py) */
const char* gxc_build_id(void);

/* floats of one packed critic of input width D and hidden width `hidden`; -1 if unsupported */
int64_t gxc_critic_floats(int32_t D, int32_t hidden);
/* floats of the device workspace gxc_critic_values needs (the transposed hidden layers); -1 if unsupported */
int64_t gxc_critic_work_floats(int32_t D, int32_t hidden);

/* d_out[i] = Vc(d_x[i * D .. i * D + D - 1]) for i < M.  d_work: gxc_critic_work_floats(D, hidden) floats,
 * overwritten (stream-ordered).  M == 0 launches nothing. */
gxc_status gxc_critic_values(int32_t M, int32_t D, int32_t hidden, const float* d_params, const float* d_x,
                             float* d_out, float* d_work, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GUARDX_CRITIC_H */
