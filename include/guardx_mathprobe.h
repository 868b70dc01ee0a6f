/*
 * guardx_mathprobe.h -- C ABI of libguardx_mathprobe.so: the fp32 device primitives of
 * guardx_amd/csrc/gx_device.h and gx_policy.h evaluated by themselves on the device, for gfx950.
 * TEST INFRASTRUCTURE: nothing in the product calls it (tests/test_gpu_math64.py does).
 *
 * The translation unit includes the two headers unchanged and is compiled with the flags of every
 * other library (guardx_amd/build.py:FLAGS), so a primitive here has the code the kernels get.
 *
 * All `d_*` pointers are DEVICE addresses, dense.  `stream` is a hipStream_t passed as void*
 * (NULL = default stream).  Nothing here throws or synchronises; every call that can fail returns
 * a gxm_status and gxm_last_error() describes the last failure on the calling thread.  This
 * library is separate from libguardx_hip.so and carries its own build id.
 */
#ifndef GUARDX_MATHPROBE_H
#define GUARDX_MATHPROBE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gxm_status {
    GXM_OK = 0,
    GXM_ERR_ARG = 1,         /* null pointer, negative count, unknown id, a range past 2^32 */
    GXM_ERR_UNSUPPORTED = 2, /* (not returned by this library) */
    GXM_ERR_HIP = 4          /* a HIP runtime call failed */
} gxm_status;

/* gxm_eval's `fn`.  d_y is read by ATAN2 and DIV alone, d_out1 written by the two SINCOS forms alone
 * (both may be NULL otherwise). */
typedef enum gxm_fn {
    GXM_FN_SINCOS = 0,        /* sincos_f<false>(x): out0 = sin, out1 = cos */
    GXM_FN_SINCOS_FINITE = 1, /* sincos_f<true>(x):  out0 = sin, out1 = cos */
    GXM_FN_ATAN2 = 2,         /* atan2_f(y, x) */
    GXM_FN_EXP = 3,           /* exp_f(x) */
    GXM_FN_LOG = 4,           /* log_f(x) */
    GXM_FN_TANH = 5,          /* tanh_f(x) */
    GXM_FN_RCP_UNSCALED = 6,  /* rcp_unscaled(x) */
    GXM_FN_DIV_BIN16 = 7,     /* div_bin16(x) */
    GXM_FN_DIV = 8,           /* x / y as the compiler lowers it */
    GXM_FN_RCP = 9,           /* 1.0f / x as the compiler lowers it */
    GXM_FN_SQRT = 10,         /* sqrtf(x) as the compiler lowers it */
    GXM_FN_COUNT = 11
} gxm_fn;

/* gxm_sweep's `pair`: a fast form against its plain form, compared by their bits (two NaNs are equal) */
typedef enum gxm_pair {
    GXM_PAIR_RCP = 0,    /* rcp_unscaled(d) against 1.0f / d */
    GXM_PAIR_TANH = 1,   /* tanh_f(x) against the checker's statement: NaN through; t = 1 - 2 / (exp_f(2|x|) + 1)
                            with the IEEE division for |x| <= 9, else 1; the sign of x */
    GXM_PAIR_SINCOS = 2, /* sincos_f<true>(x) against sincos_f<false>(x), both outputs */
    GXM_PAIR_DIV_BIN16 = 3, /* div_bin16(x) against x / kBinSize16 */
    GXM_PAIR_COUNT = 4
} gxm_pair;

#define GXM_REPORT_LOWEST 16
/* The report of gxm_sweep, 80 bytes.  Before the first call the caller sets mismatches = 0 and every word of
 * lowest[] to 0xFFFFFFFF; calls over disjoint ranges may share one report.  Afterwards the first
 * min(mismatches, 16) words of lowest[] are the lowest mismatching patterns, ascending. */
typedef struct gxm_sweep_report {
    uint64_t mismatches;
    uint32_t lowest[GXM_REPORT_LOWEST];
    uint32_t reserved[2];
} gxm_sweep_report;

const char* gxm_last_error(void);
/* sha256 (24 hex digits) over the library's sources, headers, flags and compiler (guardx_amd/build.py) */
const char* gxm_build_id(void);

/* d_out0[i] (and d_out1[i]) = fn(d_x[i] (, d_y[i])) for i < n, one thread per element.  n == 0 launches nothing. */
gxm_status gxm_eval(int32_t fn, int32_t n, const float* d_x, const float* d_y, float* d_out0, float* d_out1, void* stream);

/* normal_pair(seed0, seed1, d_env[i], d_ctr[i]) -> d_z0[i], d_z1[i] for i < n.  n == 0 launches nothing. */
gxm_status gxm_normal_pair(uint32_t seed0, uint32_t seed1, int32_t n, const uint32_t* d_env, const uint32_t* d_ctr,
                           float* d_z0, float* d_z1, void* stream);

/* The `count` consecutive fp32 bit patterns from first_bits (first_bits + count <= 2^32), a grid-stride loop:
 * every pattern whose fast and plain form differ in their bits is counted in d_report.  count == 0 launches nothing. */
gxm_status gxm_sweep(int32_t pair, uint32_t first_bits, uint64_t count, gxm_sweep_report* d_report, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GUARDX_MATHPROBE_H */
