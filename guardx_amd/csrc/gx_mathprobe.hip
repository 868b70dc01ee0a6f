// gx_mathprobe.hip -- libguardx_mathprobe.so (include/guardx_mathprobe.h): the fp32 primitives of gx_device.h and
// gx_policy.h evaluated by themselves.  TEST INFRASTRUCTURE (tests/test_gpu_math64.py): nothing in the product calls it.
//
// Three entries.  gxm_eval: one thread per element through one primitive -- or through a plain `/`, `1.0f / x`, sqrtf,
// which is how the build's "correctly rounded lowering" and denormal mode are pinned.  gxm_normal_pair: the Box-Muller of
// the closed-loop rollouts on explicit (env, counter) arrays.  gxm_sweep: a grid-stride loop over consecutive fp32 bit
// patterns that compares a fast form with its plain form bit for bit and reports how many patterns differ and the 16
// lowest of them; the whole 2^32 takes a few milliseconds of vector work and copies back 80 bytes.
//
// Both headers are included unchanged and the flags are the other libraries', so a primitive compiles here to what
// the kernels get (each is __forceinline__: there is no shared object code to link against instead).
#include "../../include/guardx_mathprobe.h"
#include "gx_policy.h"
#include <hip/hip_runtime.h>
#include <string>

#ifndef GXM_BUILD_ID
#define GXM_BUILD_ID "unknown"
#endif

namespace {

using namespace gx;

thread_local std::string g_err;

gxm_status fail(gxm_status st, const std::string& msg)
{
    g_err = msg;
    return st;
}

constexpr int kThreads = 256;
constexpr unsigned kSweepBlocks = 2048; // 8 workgroups on each of 256 CUs; 2^32 patterns are 8192 per thread

template <int FN>
__global__ __launch_bounds__(kThreads) void eval_kernel(int n, const float* __restrict__ x, const float* __restrict__ y,
                                                        float* __restrict__ o0, float* __restrict__ o1)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float a = x[i];
    if constexpr (FN == GXM_FN_SINCOS) {
        float s, c;
        sincos_f<false>(a, s, c);
        o0[i] = s;
        o1[i] = c;
    } else if constexpr (FN == GXM_FN_SINCOS_FINITE) {
        float s, c;
        sincos_f<true>(a, s, c);
        o0[i] = s;
        o1[i] = c;
    } else if constexpr (FN == GXM_FN_ATAN2) o0[i] = atan2_f(y[i], a);
    else if constexpr (FN == GXM_FN_EXP) o0[i] = exp_f(a);
    else if constexpr (FN == GXM_FN_LOG) o0[i] = log_f(a);
    else if constexpr (FN == GXM_FN_TANH) o0[i] = tanh_f(a);
    else if constexpr (FN == GXM_FN_RCP_UNSCALED) o0[i] = rcp_unscaled(a);
    else if constexpr (FN == GXM_FN_DIV_BIN16) o0[i] = div_bin16(a);
    else if constexpr (FN == GXM_FN_DIV) o0[i] = a / y[i];
    else if constexpr (FN == GXM_FN_RCP) o0[i] = 1.0f / a;
    else o0[i] = sqrtf(a);
}

__global__ __launch_bounds__(kThreads) void normal_pair_kernel(uint32_t s0, uint32_t s1, int n, const uint32_t* __restrict__ env,
                                                               const uint32_t* __restrict__ ctr, float* __restrict__ z0,
                                                               float* __restrict__ z1)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    float a, b;
    normal_pair(s0, s1, env[i], ctr[i], a, b);
    z0[i] = a;
    z1[i] = b;
}

// the checker's tanh (oracle/gx_oracle.c:gx_tanh), operator for operator: exp_f with its guards, the IEEE division
GX_D float tanh_plain(float x)
{
    if (x != x) return x;
    const float ax = fabsf(x);
    float t = 1.0f;
    if (ax <= 9.0f) t = 1.0f - 2.0f / (exp_f(2.0f * ax) + 1.0f);
    return (f2u(x) >> 31) ? -t : t;
}

GX_D bool same_bits(float a, float b) { return f2u(a) == f2u(b) || (a != a && b != b); }

template <int PAIR>
GX_D bool pair_differs(float x)
{
    if constexpr (PAIR == GXM_PAIR_RCP) return !same_bits(rcp_unscaled(x), 1.0f / x);
    else if constexpr (PAIR == GXM_PAIR_TANH) return !same_bits(tanh_f(x), tanh_plain(x));
    else if constexpr (PAIR == GXM_PAIR_SINCOS) {
        float s0, c0, s1, c1;
        sincos_f<true>(x, s0, c0);
        sincos_f<false>(x, s1, c1);
        return !same_bits(s0, s1) || !same_bits(c0, c1);
    } else return !same_bits(div_bin16(x), x / kBinSize16);
}

// `v` into the ascending list of the 16 lowest patterns: an atomicMin per slot, the displaced (larger) value carried on to
// the next slot.  Every slot only ever decreases, so a value above the last slot's current content can never enter.
__device__ void report_pattern(gxm_sweep_report* rep, uint32_t v)
{
    if (v >= __atomic_load_n(&rep->lowest[GXM_REPORT_LOWEST - 1], __ATOMIC_RELAXED)) return;
    for (int s = 0; s < GXM_REPORT_LOWEST; ++s) {
        const uint32_t old = atomicMin(&rep->lowest[s], v);
        if (old == v) return;
        if (old > v) v = old;
        if (v == 0xFFFFFFFFu) return; // the empty slot's filler: nothing left to carry
    }
}

template <int PAIR>
__global__ __launch_bounds__(kThreads) void sweep_kernel(uint32_t first, unsigned long long count, gxm_sweep_report* rep)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * kThreads;
    unsigned long long mine = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; i < count; i += stride) {
        const uint32_t bits = first + (uint32_t)i;
        if (pair_differs<PAIR>(u2f(bits))) {
            ++mine;
            report_pattern(rep, bits);
        }
    }
    if (mine) atomicAdd(reinterpret_cast<unsigned long long*>(&rep->mismatches), mine);
}

gxm_status launched(const char* what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GXM_OK : fail(GXM_ERR_HIP, std::string(what) + " launch failed: " + hipGetErrorString(e));
}

template <int FN>
void launch_eval(int n, const float* x, const float* y, float* o0, float* o1, hipStream_t s)
{
    hipLaunchKernelGGL(eval_kernel<FN>, dim3((unsigned)(((long long)n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, n, x, y, o0, o1);
}

template <int PAIR>
void launch_sweep(uint32_t first, uint64_t count, gxm_sweep_report* rep, hipStream_t s)
{
    const uint64_t need = (count + kThreads - 1) / kThreads;
    const unsigned grid = (unsigned)(need < kSweepBlocks ? need : kSweepBlocks);
    hipLaunchKernelGGL(sweep_kernel<PAIR>, dim3(grid), dim3(kThreads), 0, s, first, (unsigned long long)count, rep);
}

} // namespace

extern "C" const char* gxm_last_error(void) { return g_err.c_str(); }

extern "C" const char* gxm_build_id(void) { return GXM_BUILD_ID; } // guardx_amd/build.py:LIBRARIES["mathprobe"].source_hash()

extern "C" gxm_status gxm_eval(int32_t fn, int32_t n, const float* d_x, const float* d_y, float* d_out0, float* d_out1,
                               void* stream)
{
    if (fn < 0 || fn >= GXM_FN_COUNT) return fail(GXM_ERR_ARG, "gxm_eval: unknown fn");
    if (n < 0) return fail(GXM_ERR_ARG, "gxm_eval: n must be >= 0");
    if (!d_x || !d_out0) return fail(GXM_ERR_ARG, "gxm_eval: null pointer");
    if ((fn == GXM_FN_ATAN2 || fn == GXM_FN_DIV) && !d_y) return fail(GXM_ERR_ARG, "gxm_eval: this fn reads d_y: null pointer");
    if ((fn == GXM_FN_SINCOS || fn == GXM_FN_SINCOS_FINITE) && !d_out1)
        return fail(GXM_ERR_ARG, "gxm_eval: this fn writes d_out1: null pointer");
    if (n == 0) return GXM_OK;
    hipStream_t s = (hipStream_t)stream;
    switch (fn) {
    case GXM_FN_SINCOS: launch_eval<GXM_FN_SINCOS>(n, d_x, d_y, d_out0, d_out1, s); break;
    case GXM_FN_SINCOS_FINITE: launch_eval<GXM_FN_SINCOS_FINITE>(n, d_x, d_y, d_out0, d_out1, s); break;
    case GXM_FN_ATAN2: launch_eval<GXM_FN_ATAN2>(n, d_x, d_y, d_out0, d_out1, s); break;
    case GXM_FN_EXP: launch_eval<GXM_FN_EXP>(n, d_x, d_y, d_out0, d_out1, s); break;
    case GXM_FN_LOG: launch_eval<GXM_FN_LOG>(n, d_x, d_y, d_out0, d_out1, s); break;
    case GXM_FN_TANH: launch_eval<GXM_FN_TANH>(n, d_x, d_y, d_out0, d_out1, s); break;
    case GXM_FN_RCP_UNSCALED: launch_eval<GXM_FN_RCP_UNSCALED>(n, d_x, d_y, d_out0, d_out1, s); break;
    case GXM_FN_DIV_BIN16: launch_eval<GXM_FN_DIV_BIN16>(n, d_x, d_y, d_out0, d_out1, s); break;
    case GXM_FN_DIV: launch_eval<GXM_FN_DIV>(n, d_x, d_y, d_out0, d_out1, s); break;
    case GXM_FN_RCP: launch_eval<GXM_FN_RCP>(n, d_x, d_y, d_out0, d_out1, s); break;
    default: launch_eval<GXM_FN_SQRT>(n, d_x, d_y, d_out0, d_out1, s); break;
    }
    return launched("gxm_eval");
}

extern "C" gxm_status gxm_normal_pair(uint32_t seed0, uint32_t seed1, int32_t n, const uint32_t* d_env, const uint32_t* d_ctr,
                                      float* d_z0, float* d_z1, void* stream)
{
    if (n < 0) return fail(GXM_ERR_ARG, "gxm_normal_pair: n must be >= 0");
    if (!d_env || !d_ctr || !d_z0 || !d_z1) return fail(GXM_ERR_ARG, "gxm_normal_pair: null pointer");
    if (n == 0) return GXM_OK;
    hipLaunchKernelGGL(normal_pair_kernel, dim3((unsigned)(((long long)n + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, seed0, seed1, n, d_env, d_ctr, d_z0, d_z1);
    return launched("gxm_normal_pair");
}

extern "C" gxm_status gxm_sweep(int32_t pair, uint32_t first_bits, uint64_t count, gxm_sweep_report* d_report, void* stream)
{
    if (pair < 0 || pair >= GXM_PAIR_COUNT) return fail(GXM_ERR_ARG, "gxm_sweep: unknown pair");
    if (!d_report) return fail(GXM_ERR_ARG, "gxm_sweep: null pointer");
    if (count > (1ull << 32) - first_bits) return fail(GXM_ERR_ARG, "gxm_sweep: first_bits + count must be <= 2^32");
    if (count == 0) return GXM_OK;
    hipStream_t s = (hipStream_t)stream;
    switch (pair) {
    case GXM_PAIR_RCP: launch_sweep<GXM_PAIR_RCP>(first_bits, count, d_report, s); break;
    case GXM_PAIR_TANH: launch_sweep<GXM_PAIR_TANH>(first_bits, count, d_report, s); break;
    case GXM_PAIR_SINCOS: launch_sweep<GXM_PAIR_SINCOS>(first_bits, count, d_report, s); break;
    default: launch_sweep<GXM_PAIR_DIV_BIN16>(first_bits, count, d_report, s); break;
    }
    return launched("gxm_sweep");
}
