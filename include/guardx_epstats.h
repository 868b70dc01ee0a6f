/*
 * guardx_epstats.h -- C ABI of libguardx_epstats.so: the episode bookkeeping of the reset_done
 * learners (safe_rl_libX/trpo/trpo.py:455-541, cpo/cpo.py:596-670: ep_ret, ep_cost, ep_cost_ret,
 * ep_len, max_ep_len_ret and what the logger makes of them, utils/mpi_tools.py:70-92) over the
 * time-major (T, N) rew / cost / done tensors a fused rollout returns, on the device, for gfx950.
 *
 * Per env n, for t = 0 .. T - 1 (epoch step t0 + t), in float64, one add per step:
 *   ep_ret += rew; ep_cost += cost; epoch_ret += rew; cost_env += cost; ep_len += 1;
 *   with a discount table: ep_cost_ret += (double)cost * g[t0 + t]   (one multiply, one add)
 *   t0 + t + 1 == max_ep_len:  the env emits (ep_ret, ep_cost, ep_cost_ret, ep_len) iff ep_len == max_ep_len;
 *                              max_ret[n] = epoch_ret; every accumulator is cleared
 *   else done == 1.0f:         the env emits and clears ep_ret, ep_cost, ep_cost_ret, ep_len (not epoch_ret)
 * Emitted episodes are compacted in logger order: by step, within a step by env.
 *
 * Moments of a list x_0 .. x_{n-1} (each entry rounded to float32 first, then float64 throughout):
 *   slot s = 0 .. 255 adds x_s, x_{s+256}, ... in that order from 0.0; the slots fold pairwise,
 *   slot s += slot s + stride for stride = 128, 64, .., 1; S = slot 0; mean = S / n;
 *   Q the same reduction of (x_i - mean)^2; min, max (-0 < +0); a NaN entry makes min and max NaN.
 *   n == 0: S = Q = 0, mean = NaN, min = +inf, max = -inf.
 *   A row of moments is seven doubles: n, S, mean, Q, min, max and std = sqrt(Q / n), correctly rounded.
 *
 * All `d_*` pointers are DEVICE addresses, dense.  The float64 arrays travel as void*.  `stream` is a
 * hipStream_t passed as void* (NULL = default stream).  Nothing here throws or synchronises; every call
 * that can fail returns a gxt_status and gxt_last_error() describes the last failure on the calling
 * thread.  This library is separate from libguardx_hip.so and carries its own build id.
 */
#ifndef GUARDX_EPSTATS_H
#define GUARDX_EPSTATS_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gxt_status {
    GXT_OK = 0,
    GXT_ERR_ARG = 1,         /* null pointer, negative size, t0 < 0, t0 + T > max_ep_len */
    GXT_ERR_UNSUPPORTED = 2, /* T * (N rounded up to 64) does not fit 31 bits */
    GXT_ERR_HIP = 4          /* a HIP runtime call failed */
} gxt_status;

/* rows of d_moments that gxt_episode_stats writes; row GXT_KEY_COST_SUM holds the call's cost sum in S
 * (the per-env float64 sums reduced over the envs in the slot order above, not rounded to float32) */
typedef enum gxt_key {
    GXT_KEY_EP_RET = 0,
    GXT_KEY_EP_COST = 1,
    GXT_KEY_EP_LEN = 2,
    GXT_KEY_EP_COST_RET = 3, /* written only with d_gpow */
    GXT_KEY_MAX_RET = 4,     /* written only when t0 + T == max_ep_len */
    GXT_KEY_VVALS = 5,       /* written only with d_val: its T * N elements in memory order */
    GXT_KEY_COST_SUM = 6,
    GXT_KEYS = 7
} gxt_key;

const char* gxt_last_error(void);
/* sha256 (24 hex digits) over the library's sources, headers, flags and compiler (guardx_amd/build.py) */
const char* gxt_build_id(void);

/* bytes of the device workspace gxt_episode_stats needs for N envs and T steps; -1 for negative sizes or
 * sizes past GXT_ERR_UNSUPPORTED's bound */
int64_t gxt_work_bytes(int32_t N, int32_t T);

/* The scan, the ordered compaction and the moments, stream-ordered.
 * d_rew, d_cost, d_done: (T, N) float32.  d_val: (T, N) float32 or NULL.  d_gpow: double[max_ep_len], the
 * discount table g, or NULL.  d_carry_in: double[4][N] (ep_ret, ep_cost, ep_cost_ret, epoch_ret) and
 * d_carry_len_in: int32[N], the accumulators at step t0, or both NULL for zeros; d_carry and d_carry_len receive
 * those at step t0 + T (they may be the same arrays).
 * d_work: gxt_work_bytes(N, T) bytes, 8-byte aligned, overwritten.
 * The compact episode arrays, each of capacity T * N, of which the first *d_count entries are written:
 * d_env, d_t_end (the epoch step t0 + t), d_ep_len: int32; d_ep_ret, d_ep_cost, d_ep_cost_ret: double.
 * d_max_ret: double[N], written when t0 + T == max_ep_len.  d_moments: double[GXT_KEYS][7].
 * N == 0 or T == 0 launches nothing. */
gxt_status gxt_episode_stats(int32_t N, int32_t T, int32_t t0, int32_t max_ep_len, const float* d_rew,
                             const float* d_cost, const float* d_done, const float* d_val, void* d_gpow,
                             void* d_carry_in, int32_t* d_carry_len_in, void* d_carry, int32_t* d_carry_len,
                             void* d_work, int32_t* d_env, int32_t* d_t_end, void* d_ep_ret, void* d_ep_cost,
                             void* d_ep_cost_ret, int32_t* d_ep_len, int32_t* d_count, void* d_max_ret,
                             void* d_moments, void* stream);

/* Moments of `rows` lists of n entries each: d_x (rows, n), d_moments double[rows][7].  f64 == 0: the entries are
 * float32.  f64 != 0: they are float64 and enter as they are, not rounded to float32 (the S of such a row is the plain
 * float64 sum in the slot order).  rows == 0 launches nothing; n == 0 writes the empty moments. */
gxt_status gxt_moments(int32_t rows, int32_t n, int32_t f64, void* d_x, void* d_moments, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GUARDX_EPSTATS_H */
