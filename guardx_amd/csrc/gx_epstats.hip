// gx_epstats.hip -- libguardx_epstats.so (include/guardx_epstats.h): the learners' episode bookkeeping (EpRet, EpCost,
// EpLen, EpCostRet, MaxEpLenRet, VVals, the cost sum) over the (T, N) rew / cost / done a fused rollout returned, on
// the caller's stream and without a host synchronisation.  The header fixes the arithmetic; this file is its order of
// work:
//
//   scan_kernel     one lane per env and add chain walks its column in t (the per-env add order is the definition: T is
//                   never split across lanes; the three independent chains of an env run in three waves).  A row of
//                   a tensor is coalesced across the wave; the kRows rows of the next block are in flight during the
//                   adds of this one, because at N = 2000 there are only 32 waves per chain to hide a memory round
//                   trip with.  An emitted episode is written at its (t, n) slot of the staging arrays, and per
//                   (t, wave) the ballot of the lanes that emitted.
//   offsets_kernel  exclusive scan of the ballots' popcounts in (t, wave) order, one workgroup; the total is the
//                   episode count, which stays on the device.
//   scatter_kernel  (t, n) -> offs[t, wave] + popcount(ballot below the lane): the compact arrays in logger order.
//                   With val, one more workgroup of the same launch takes the VVals moments, which need nothing of the
//                   scan and would otherwise be the longest step after it.
//   moments_kernel  one 256-lane workgroup per key: lane s adds the entries s, s + 256, ... in order, the 256 partial
//                   sums fold with strides 128 .. 1; then the same for the squared deviations.  Integer arithmetic
//                   fixes every position and the float64 order is the header's, so the result has the bits of the
//                   host statement (guardx_amd/epstats.py).  No floating-point atomics.
#include "../../include/guardx_epstats.h"
#include <hip/hip_runtime.h>
#include <string>

#ifndef GXT_BUILD_ID
#define GXT_BUILD_ID "unknown"
#endif

namespace {

thread_local std::string g_err;

gxt_status fail(gxt_status st, const std::string& msg)
{
    g_err = msg;
    return st;
}

constexpr int kWave = 64;
constexpr int kRows = 16;        // rows of rew / cost / done loaded ahead of the adds that consume them
constexpr int kSlots = 256;      // the reduction's slots (the header's order)
constexpr int kAhead = 24;       // entries per slot loaded ahead of the adds
constexpr int kScanThreads = 1024;
constexpr int kMoments = 7;      // doubles per row of moments

using u64 = unsigned long long;

struct Work {
    double *ret, *cost, *cret, *cost_env;
    u64* mask;
    int32_t *len, *offs;
};

int64_t waves_of(int N) { return ((int64_t)N + kWave - 1) / kWave; }
bool too_large(int N, int T) { return (int64_t)T * waves_of(N) * kWave >= ((int64_t)1 << 31); }

int64_t work_bytes(int N, int T)
{
    const int64_t TN = (int64_t)T * N, TW = (int64_t)T * waves_of(N);
    return 8 * (3 * TN + N + TW) + 4 * (TN + TW);
}

Work carve(void* base, int N, int T)
{
    const int64_t TN = (int64_t)T * N, TW = (int64_t)T * waves_of(N);
    Work w;
    w.ret = static_cast<double*>(base);
    w.cost = w.ret + TN;
    w.cret = w.cost + TN;
    w.cost_env = w.cret + TN;
    w.mask = reinterpret_cast<u64*>(w.cost_env + N);
    w.len = reinterpret_cast<int32_t*>(w.mask + TW);
    w.offs = w.len + TN;
    return w;
}

struct ScanArgs {
    int N, T, t0, max_ep_len;
    const float *rew, *cost, *done;
    const double *gpow, *carry_in;
    const int32_t* len_in;
    double* carry;
    int32_t* carry_len;
    Work w;
    double* max_ret;
};

// One wave of the scan: 64 envs, one of the three independent add chains of an env.  ROLE 0: rew -> ep_ret, epoch_ret,
// and the bookkeeping all chains agree on (ep_len, the ballots); ROLE 1: cost -> ep_cost and the call's cost per env;
// ROLE 2: cost * g -> ep_cost_ret.  Every role follows done and ep_len itself, so no chain waits for another; a lone wave
// issues a dependent instruction every ~6 cycles, and three waves on three SIMDs run the three chains side by side.
// The rows of block k + 1 are loaded before the adds of block k.
template <int ROLE, bool ADDS>
__device__ __forceinline__ void scan_role(const ScanArgs a, int wave, int lane, int W)
{
    const int N = a.N, T = a.T, t0 = a.t0;
    const int n = wave * kWave + lane;
    const bool live = n < N;
    const int nn = live ? n : 0;
    const float* __restrict__ src = ROLE == 0 ? a.rew : a.cost;
    const float* __restrict__ done = a.done;
    const double* __restrict__ gpow = a.gpow;
    constexpr bool adds = ADDS;                                // without a table the third chain only follows the clears
    double* __restrict__ stage = ROLE == 0 ? a.w.ret : ROLE == 1 ? a.w.cost : a.w.cret;
    double acc = 0.0, run = 0.0;                               // the episode's sum; ROLE 0: epoch_ret, ROLE 1: the call's cost
    int len = 0;
    if (live && a.carry_in) {
        acc = a.carry_in[(size_t)ROLE * N + nn];
        if (ROLE == 0) run = a.carry_in[3 * (size_t)N + nn];
        len = a.len_in[nn];
    }
    const bool has_timeout = t0 + T == a.max_ep_len;           // then the time-out step is the call's last row

    float xa[kRows], da[kRows], xb[kRows], db[kRows];
    double ga[kRows], gb[kRows];
    auto load = [&](float* x, float* d, double* g, int tb) {
#pragma unroll
        for (int u = 0; u < kRows; ++u) {
            // every load is unconditional (the row clamped to the last one, the lane to env 0): rows() ignores what
            // lies past T, and no load hides under a branch from the waits of the loop below
            const int t = tb + u < T ? tb + u : T - 1;
            const size_t row = (size_t)t * N;                  // uniform: the row's base stays in scalar registers
            x[u] = adds ? (src + row)[nn] : 0.0f;
            d[u] = (done + row)[nn];
            g[u] = ROLE == 2 && adds ? gpow[t0 + t] : 0.0;
        }
    };
    auto rows = [&](const float* x, const float* d, const double* g, int tb) {
#pragma unroll
        for (int u = 0; u < kRows; ++u) {
            const int t = tb + u;
            if (t < T) {                                       // wave-uniform
                if (ROLE == 2) {
                    if (adds) acc += (double)x[u] * g[u];
                } else {
                    acc += (double)x[u];
                    run += (double)x[u];
                }
                len += 1;
                const bool emit = live && (has_timeout && t == T - 1 ? len == a.max_ep_len : d[u] == 1.0f);
                const size_t i = (size_t)t * N + nn;
                if (ROLE == 0) {
                    const u64 m = __ballot(emit);
                    if (lane == 0) a.w.mask[(size_t)t * W + wave] = m;
                    if (emit) a.w.len[i] = len;
                }
                if (emit) stage[i] = acc;
                acc = emit ? 0.0 : acc;
                len = emit ? 0 : len;
            }
        }
    };
    const int blocks = (T + kRows - 1) / kRows;                // T >= 1; straight-line loop body, as in ordered_walk
    load(xa, da, ga, 0);
    for (int p = 0; p < blocks / 2; ++p) {
        load(xb, db, gb, (2 * p + 1) * kRows);
        rows(xa, da, ga, 2 * p * kRows);
        load(xa, da, ga, (2 * p + 2 < blocks ? 2 * p + 2 : blocks - 1) * kRows);
        rows(xb, db, gb, (2 * p + 1) * kRows);
    }
    if (blocks & 1) rows(xa, da, ga, (blocks - 1) * kRows);
    if (!live) return;
    if (ROLE == 1) a.w.cost_env[nn] = run;
    if (has_timeout) {                                         // every env: MaxEpLenRet, and all accumulators cleared
        if (ROLE == 0) a.max_ret[nn] = run;
        acc = 0.0;
        run = 0.0;
        len = 0;
    }
    a.carry[(size_t)ROLE * N + nn] = acc;
    if (ROLE == 0) {
        a.carry[3 * (size_t)N + nn] = run;
        a.carry_len[nn] = len;
    }
}

// offs[k] = the episodes emitted before (t, wave) pair k; *count = all of them.  One workgroup: thread j owns the pairs
// [j chunk, (j + 1) chunk).
__global__ __launch_bounds__(kScanThreads) void offsets_kernel(int M, const u64* __restrict__ mask, int32_t* __restrict__ offs,
                                                               int32_t* __restrict__ count)
{
    __shared__ int part[2][kScanThreads];
    const int j = threadIdx.x;
    const int chunk = (M + kScanThreads - 1) / kScanThreads;
    const long long at0 = (long long)j * chunk;
    const int lo = at0 < M ? (int)at0 : M, hi = lo + chunk < M ? lo + chunk : M;
    int own = 0;
    for (int k = lo; k < hi; ++k) own += __popcll(mask[k]);
    part[0][j] = own;
    __syncthreads();
    int cur = 0;
    for (int step = 1; step < kScanThreads; step <<= 1) {
        part[cur ^ 1][j] = part[cur][j] + (j >= step ? part[cur][j - step] : 0);
        cur ^= 1;
        __syncthreads();
    }
    int at = part[cur][j] - own;
    for (int k = lo; k < hi; ++k) {
        offs[k] = at;
        at += __popcll(mask[k]);
    }
    if (j == kScanThreads - 1) *count = part[cur][j];
}

__global__ __launch_bounds__(256) void scatter_kernel(int N, int T, int t0, Work w, int32_t* __restrict__ env,
                                                      int32_t* __restrict__ t_end, double* __restrict__ ep_ret,
                                                      double* __restrict__ ep_cost, double* __restrict__ ep_cret,
                                                      int32_t* __restrict__ ep_len)
{
    const int W = (N + kWave - 1) / kWave;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long pair = idx / kWave;
    const int lane = (int)(idx % kWave);
    if (pair >= (long long)T * W) return;
    const int t = (int)(pair / W), wave = (int)(pair % W), n = wave * kWave + lane;
    const u64 m = w.mask[pair];
    if (n >= N || !((m >> lane) & 1ull)) return;
    const int pos = w.offs[pair] + __popcll(m & ((1ull << lane) - 1ull));
    const size_t i = (size_t)t * N + n;
    env[pos] = n;
    t_end[pos] = t0 + t;
    ep_ret[pos] = w.ret[i];
    ep_cost[pos] = w.cost[i];
    ep_cret[pos] = w.cret[i];
    ep_len[pos] = w.len[i];
}

// fold the 256 slots of `v` pairwise, strides 128 .. 1 (the header's order); every lane returns slot 0
__device__ __forceinline__ double fold_sum(double* v, int s, double x)
{
    __syncthreads();
    v[s] = x;
    __syncthreads();
    for (int stride = kSlots / 2; stride >= 1; stride >>= 1) {
        if (s < stride) v[s] = v[s] + v[s + stride];
        __syncthreads();
    }
    return v[0];
}

// the moments of x(0) .. x(n - 1), by one workgroup of kSlots lanes: out = n, S, mean, Q, min, max, std
struct Slots {
    double v[kSlots], vmin[kSlots], vmax[kSlots];
    int vnan[kSlots];
};

// use(e) for the entries s, s + 256, s + 512, .. < n of x in that order (x(base, off) = entry base + off, base uniform), with the loads of kAhead entries in flight
// while the kAhead before them are consumed (a lone wave per SIMD hides no latency by itself)
template <class F, class G>
__device__ __forceinline__ void ordered_walk(long long n, int s, F x, G use)
{
    const long long per = (long long)kAhead * kSlots, groups = n / per;
    double a[kAhead], b[kAhead];
    auto load = [&](double* e, long long g) {
#pragma unroll
        for (int u = 0; u < kAhead; ++u) e[u] = x(g * per, u * kSlots + s);
    };
    auto consume = [&](const double* e) {
#pragma unroll
        for (int u = 0; u < kAhead; ++u) use(e[u]);
    };
    // straight-line loop body (a load under a condition would make every wait in it a wait for all loads): groups
    // 2 p and 2 p + 1 per turn; the last turn's second load is clamped to the last group, which an odd count consumes
    // after the loop and an even one has consumed already
    if (groups > 0) load(a, 0);
    for (long long p = 0; p < groups / 2; ++p) {
        load(b, 2 * p + 1);
        consume(a);
        load(a, 2 * p + 2 < groups ? 2 * p + 2 : groups - 1);
        consume(b);
    }
    if (groups & 1) consume(a);
    const long long base = groups * per;                       // the last, partial group: guarded per lane
    const int left = (int)(n - base);
#pragma unroll
    for (int u = 0; u < kAhead; ++u) a[u] = u * kSlots + s < left ? x(base, u * kSlots + s) : 0.0;
#pragma unroll
    for (int u = 0; u < kAhead; ++u)
        if (u * kSlots + s < left) use(a[u]);
}

template <class F>
__device__ __forceinline__ void moments_block(Slots& sl, long long n, F x, double* __restrict__ out)
{
    double *v = sl.v, *vmin = sl.vmin, *vmax = sl.vmax;
    int* vnan = sl.vnan;
    const int s = threadIdx.x;
    const double inf = __builtin_huge_val();
    double acc = 0.0, mn = inf, mx = -inf;
    bool nan = false;
    ordered_walk(n, s, x, [&](double e) {
        acc += e;
        nan = nan || e != e;
        mn = __builtin_fmin(mn, e);                            // a NaN entry is ignored here and reported by `nan`;
        mx = __builtin_fmax(mx, e);                            // -0 < +0 (IEEE minimum / maximum), as the host has it
    });
    const double S = fold_sum(v, s, acc);
    vmin[s] = mn;
    vmax[s] = mx;
    vnan[s] = nan;
    __syncthreads();
    for (int stride = kSlots / 2; stride >= 1; stride >>= 1) {
        if (s < stride) {
            vmin[s] = __builtin_fmin(vmin[s], vmin[s + stride]);
            vmax[s] = __builtin_fmax(vmax[s], vmax[s + stride]);
            vnan[s] |= vnan[s + stride];
        }
        __syncthreads();
    }
    const double mean = S / (double)n;
    acc = 0.0;
    ordered_walk(n, s, x, [&](double e) {
        const double dv = e - mean;
        acc += dv * dv;
    });
    const double Q = fold_sum(v, s, acc);
    if (s == 0) {
        const double qnan = __builtin_nan("");
        out[0] = (double)n;
        out[1] = S;
        out[2] = mean;
        out[3] = Q;
        out[4] = vnan[0] ? qnan : vmin[0];
        out[5] = vnan[0] ? qnan : vmax[0];
        out[6] = sqrt(Q / (double)n);
    }
}

__device__ double as_logged(double x) { return (double)(float)x; }     // np.array(x, dtype=np.float32)

struct Lists {
    const double *ep_ret, *ep_cost, *ep_cret, *max_ret, *cost_env;
    const int32_t *ep_len, *count;
    const float* val;
    int N, T, has_gpow, has_timeout;
};

// The scan's grid: one workgroup per 64 envs, whose first three waves are the three chains (the fourth has nothing to
// do), and with `val` one more workgroup that takes the VVals moments -- they do not depend on the scan, are the longest
// single piece of the call (T N entries through 256 lanes), and so run beside it instead of after it.
__global__ __launch_bounds__(kSlots) void scan_kernel(ScanArgs a, int W, const float* __restrict__ val, double* __restrict__ vvals)
{
    __shared__ Slots sl;
    if ((int)blockIdx.x == W) {
        moments_block(sl, (long long)a.T * a.N, [=](long long b, int o) { return (double)(val + b)[o]; }, vvals);
        return;
    }
    const int role = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), lane = threadIdx.x % kWave;
    if (role == 0) scan_role<0, true>(a, blockIdx.x, lane, W);
    else if (role == 1) scan_role<1, true>(a, blockIdx.x, lane, W);
    else if (role == 2 && a.gpow) scan_role<2, true>(a, blockIdx.x, lane, W);
    else if (role == 2) scan_role<2, false>(a, blockIdx.x, lane, W);
}

__global__ __launch_bounds__(kSlots) void moments_kernel(Lists a, double* __restrict__ moments)
{
    __shared__ Slots sl;
    const int key = blockIdx.x;
    double* out = moments + kMoments * key;
    const long long ne = *a.count;
    const double* const f64 = key == GXT_KEY_EP_RET ? a.ep_ret : key == GXT_KEY_EP_COST ? a.ep_cost :
                              key == GXT_KEY_EP_COST_RET ? a.ep_cret : key == GXT_KEY_MAX_RET ? a.max_ret : a.cost_env;
    const int32_t* const len = a.ep_len;
    switch (key) {
    case GXT_KEY_EP_LEN: moments_block(sl, ne, [=](long long b, int o) { return (double)(float)(len + b)[o]; }, out); break;
    case GXT_KEY_VVALS: break;                                 // taken beside the scan (scan_kernel)
    case GXT_KEY_COST_SUM: moments_block(sl, (long long)a.N, [=](long long b, int o) { return (f64 + b)[o]; }, out); break;
    default:
        if ((key != GXT_KEY_EP_COST_RET || a.has_gpow) && (key != GXT_KEY_MAX_RET || a.has_timeout))
            moments_block(sl, key == GXT_KEY_MAX_RET ? (long long)a.N : ne,
                          [=](long long b, int o) { return as_logged((f64 + b)[o]); }, out);
        break;
    }
}

template <class E>
__global__ __launch_bounds__(kSlots) void rows_moments_kernel(int n, const E* __restrict__ x, double* __restrict__ moments)
{
    __shared__ Slots sl;
    const E* row = x + (size_t)blockIdx.x * n;
    moments_block(sl, (long long)n, [=](long long b, int o) { return (double)(row + b)[o]; }, moments + kMoments * blockIdx.x);
}

gxt_status launched(const char* who)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GXT_OK : fail(GXT_ERR_HIP, std::string(who) + " launch failed: " + hipGetErrorString(e));
}

} // namespace

extern "C" const char* gxt_last_error(void) { return g_err.c_str(); }

extern "C" const char* gxt_build_id(void) { return GXT_BUILD_ID; } // guardx_amd/build.py:POST_LIBRARIES["epstats"].source_hash()

extern "C" int64_t gxt_work_bytes(int32_t N, int32_t T)
{
    return (N < 0 || T < 0 || too_large(N, T)) ? -1 : work_bytes(N, T);
}

extern "C" gxt_status gxt_episode_stats(int32_t N, int32_t T, int32_t t0, int32_t max_ep_len, const float* d_rew,
                                        const float* d_cost, const float* d_done, const float* d_val, void* d_gpow,
                                        void* d_carry_in, int32_t* d_carry_len_in, void* d_carry,
                                        int32_t* d_carry_len, void* d_work, int32_t* d_env,
                                        int32_t* d_t_end, void* d_ep_ret, void* d_ep_cost, void* d_ep_cost_ret,
                                        int32_t* d_ep_len, int32_t* d_count, void* d_max_ret, void* d_moments, void* stream)
{
    if (!d_rew || !d_cost || !d_done || !d_carry || !d_carry_len || !d_work || !d_env || !d_t_end || !d_ep_ret ||
        !d_ep_cost || !d_ep_cost_ret || !d_ep_len || !d_count || !d_max_ret || !d_moments)
        return fail(GXT_ERR_ARG, "gxt_episode_stats: null pointer");
    if (!d_carry_in != !d_carry_len_in) return fail(GXT_ERR_ARG, "gxt_episode_stats: d_carry_in and d_carry_len_in go together");
    if (N < 0 || T < 0 || t0 < 0 || max_ep_len < 0) return fail(GXT_ERR_ARG, "gxt_episode_stats: negative size");
    if ((int64_t)t0 + T > max_ep_len) return fail(GXT_ERR_ARG, "gxt_episode_stats: t0 + T > max_ep_len");
    if (too_large(N, T)) return fail(GXT_ERR_UNSUPPORTED, "gxt_episode_stats: T * N does not fit 31 bits");
    if (N == 0 || T == 0) return GXT_OK;
    hipStream_t s = (hipStream_t)stream;
    const Work w = carve(d_work, N, T);
    const int W = (int)waves_of(N), M = T * W;
    ScanArgs sa;
    sa.N = N;
    sa.T = T;
    sa.t0 = t0;
    sa.max_ep_len = max_ep_len;
    sa.rew = d_rew;
    sa.cost = d_cost;
    sa.done = d_done;
    sa.gpow = static_cast<const double*>(d_gpow);
    sa.carry_in = static_cast<const double*>(d_carry_in);
    sa.len_in = d_carry_len_in;
    sa.carry = static_cast<double*>(d_carry);
    sa.carry_len = d_carry_len;
    sa.w = w;
    sa.max_ret = static_cast<double*>(d_max_ret);
    double* const m = static_cast<double*>(d_moments);
    hipLaunchKernelGGL(scan_kernel, dim3(W + (d_val ? 1 : 0)), dim3(kSlots), 0, s, sa, W, d_val, m + kMoments * GXT_KEY_VVALS);
    hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(kScanThreads), 0, s, M, w.mask, w.offs, d_count);
    const long long lanes = (long long)M * kWave;
    hipLaunchKernelGGL(scatter_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, N, T, t0, w, d_env, d_t_end,
                       static_cast<double*>(d_ep_ret), static_cast<double*>(d_ep_cost), static_cast<double*>(d_ep_cost_ret),
                       d_ep_len);
    Lists a;
    a.ep_ret = static_cast<const double*>(d_ep_ret);
    a.ep_cost = static_cast<const double*>(d_ep_cost);
    a.ep_cret = static_cast<const double*>(d_ep_cost_ret);
    a.max_ret = static_cast<const double*>(d_max_ret);
    a.cost_env = w.cost_env;
    a.ep_len = d_ep_len;
    a.count = d_count;
    a.val = d_val;
    a.N = N;
    a.T = T;
    a.has_gpow = d_gpow != nullptr;
    a.has_timeout = (int64_t)t0 + T == max_ep_len;
    hipLaunchKernelGGL(moments_kernel, dim3(GXT_KEYS), dim3(kSlots), 0, s, a, static_cast<double*>(d_moments));
    return launched("gxt_episode_stats");
}

extern "C" gxt_status gxt_moments(int32_t rows, int32_t n, int32_t f64, void* d_x, void* d_moments, void* stream)
{
    if (!d_x || !d_moments) return fail(GXT_ERR_ARG, "gxt_moments: null pointer");
    if (rows < 0 || n < 0) return fail(GXT_ERR_ARG, "gxt_moments: negative size");
    if (rows == 0) return GXT_OK;
    hipStream_t s = (hipStream_t)stream;
    double* m = static_cast<double*>(d_moments);
    if (f64)
        hipLaunchKernelGGL(rows_moments_kernel<double>, dim3(rows), dim3(kSlots), 0, s, n, static_cast<const double*>(d_x), m);
    else
        hipLaunchKernelGGL(rows_moments_kernel<float>, dim3(rows), dim3(kSlots), 0, s, n, static_cast<const float*>(d_x), m);
    return launched("gxt_moments");
}
