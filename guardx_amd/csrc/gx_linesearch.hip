// gx_linesearch.hip -- libguardx_linesearch.so (include/guardx_linesearch.h): the learners' backtracking line search over the
// Gaussian MLP actor (hidden width 64), on the caller's stream and without a host synchronisation.  The header fixes the
// arithmetic; this file is its order of work:
//
//   eval_kernel    a persistent grid of 4-wave workgroups; workgroup g walks the 64-row tiles g, g + grid, ... of obs, in the
//                  shape of stages 1 to 3 of gx_fisher.hip:fvp_kernel.  The candidate theta - t d is formed while it is
//                  loaded: W2, W3 and the biases into LDS, W1 into registers (wave w owns the hidden units 16 w .. + 15, so
//                  a lane never shares its B operands), log_std as three float64 per action (ls, 1 / (v1 + EPS),
//                  1 / (2 v1)).  Per tile, with a workgroup barrier (LDS only) after each stage:
//                    1  z1 = o W1' + b1 -> h1            (K = pad4 D)
//                    2  z2 = h1 W2' + b2 -> h2           (K = 64)
//                    3  mu = h2 W3' + b3                 (wave w: rows 16 w .. 16 w + 15)
//                    4  lane 4 i + p of wave w: row 16 w + i, the actions p, p + 4, ...: the terms of kl_row and logp in
//                       float64; the four lanes of a row add their parts as (p0 + p1) + (p2 + p3); the four row values
//                       (float32) are selected to zero past B and added over the wave's 16 rows (float64, a fixed tree)
//                       to the wave's running sums.
//                  The row's batch entries and the next tile's obs are loaded while the stages run.  The workgroup adds its
//                  waves' sums in wave order and writes one partial of four float64.
//   decide_kernel  one workgroup: the partials added in workgroup order, the means; then, by mode, the row of gxb_evaluate's
//                  output, the t = 0 evaluation of the search (which also resets the flag and copies theta), or the
//                  acceptance test of candidate j (which on success sets the flag and writes theta_j and the means).
// No atomics anywhere: the same arguments give the same bits.  tanh_act and sum_acc are gx_fisher.hip's, restated: ratio
// is judged by its relative error, so mu needs the same care as the product's tangents.
#include "../../include/guardx_linesearch.h"
#include "gx_policy.h"
#include <string>

#ifndef GXB_BUILD_ID
#define GXB_BUILD_ID "unknown"
#endif

namespace {

using gx::mfma_f4;
using gx::wg_sync_lds;

thread_local std::string g_err;

gxb_status fail(gxb_status st, const std::string& msg)
{
    g_err = msg;
    return st;
}

constexpr int kH = gx::kPolHd;   // hidden width
constexpr int kTile = 64;        // rows of obs per tile
constexpr int kThreads = 256;    // four waves; wave w owns the hidden units 16 w .. 16 w + 15 and the rows 16 w .. 16 w + 15
constexpr int kAp = 16;          // the action width padded to one MFMA tile
constexpr int kSW = 66;          // LDS row stride of everything 64 wide: 16 rows x 2 k of a ds_read_b32 group hit 32 banks
constexpr int kSU = 18;          // ... of mu (64 x 16)
constexpr int kDefaultWg = 256;  // one workgroup per CU of the MI355X ...
constexpr int kTwoKS1 = 16;      // ... two where pad4(D) / 4 <= 16 (D <= 64): their registers (<= 256) and LDS images (2 x 78 KB) fit a CU
                                 // together, and one workgroup's MFMA chains run under the other's tanh and row terms
constexpr int kMaxWg = 4096;
constexpr int kMaxD = 128;
constexpr int kDecideThreads = 1024;
constexpr int kAcc = 4;          // interleaved chains of a layer's sum: see sum_acc
constexpr int kDbl = 3 * kAp + 16;   // float64 at the head of LDS: ls, 1 / (v1 + EPS), 1 / (2 v1) per action; the waves' sums
constexpr double kEps = 1e-8;
constexpr double kHalfLog2Pi = 0.91893853320467274178;

// row stride of the obs tile: = 2 mod 32, at least pad4 D
constexpr int obs_stride(int KS1) { return (4 * KS1 - 2 + 31) / 32 * 32 + 2; }
constexpr int lds_floats(int KS1) { return 2 * kDbl + kH * kSW + kAp * kSW + 2 * kH + kAp + kTile * obs_stride(KS1) + 2 * kTile * kSW + kTile * kSU; }

int64_t param_count(int D, int A, int h) { return (int64_t)A + (int64_t)h * D + h + (int64_t)h * h + h + (int64_t)A * h + A; }
int tiles_of(int B) { return (int)(((int64_t)B + kTile - 1) / kTile); }
int default_workgroups(int B, int D)
{
    const int most = (D + 3) / 4 <= kTwoKS1 ? 2 * kDefaultWg : kDefaultWg;
    return tiles_of(B) < most ? tiles_of(B) : most;
}

struct State {
    double pi_l_old, surr_cost_old;   // rounded to float32, as the learners' .item() gives them
    int32_t flag, pad[3];
};
static_assert(sizeof(State) == 32, "gxb_work_bytes states it");

struct EvalArgs {
    int B, D, A, tiles;
    const float *theta, *dir, *obs, *act, *adv, *logp_old, *mu_old, *logstd_old, *adc;   // adc may be null
    double t;
    double* partial;   // [grid][4]
    const State* st;   // the search's state, or null: flag set -> nothing to do
};

#define GXB_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0)

__device__ __forceinline__ mfma_f4 splat(float v) { return mfma_f4{v, v, v, v}; }

// theta_t[i]: one product and one difference in float64 (the build has -ffp-contract=off), rounded once; theta itself at
// t = 0, whatever d holds
__device__ __forceinline__ float candidate(const float* __restrict__ th, const float* __restrict__ d, int i, double t)
{
    const float v = th[i];
    return t == 0.0 ? v : (float)((double)v - t * (double)d[i]);
}

// gx_fisher.hip:sum_acc: four chains round 16 times each at half the size of one chain's running sum
__device__ __forceinline__ mfma_f4 sum_acc(const mfma_f4 (&a)[kAcc])
{
    static_assert(kAcc == 4, "pairwise over four");
    return (a[0] + a[1]) + (a[2] + a[3]);
}

// gx_fisher.hip:tanh_act: gx::tanh_f has a small absolute error, which below |x| ~ 0.6 is a large relative one; there the odd
// polynomial of the Cephes single-precision tanh (public domain, S. Moshier) takes over: 2.3 ulp at worst over the whole line
__device__ __forceinline__ float tanh_act(float x)
{
    const float z = x * x;
    float p = fmaf(z, -5.70498872745e-3f, 2.06390887954e-2f);
    p = fmaf(z, p, -5.37397155531e-2f);
    p = fmaf(z, p, 1.33314422036e-1f);
    p = fmaf(z, p, -3.33332819422e-1f);
    const float small = fmaf(z * x, p, x);
    return fabsf(x) < 0.625f ? copysignf(small, x) : gx::tanh_f(x);
}

template <int KS1>
__global__ __launch_bounds__(kThreads, (KS1 <= kTwoKS1 ? 2 : 1)) void eval_kernel(EvalArgs a)
{
    constexpr int SO = obs_stride(KS1);
    extern __shared__ double lds_d[];
    double* const LS = lds_d;              // the candidate's log_std
    double* const I1 = LS + kAp;           // 1 / (v1 + EPS)
    double* const I2 = I1 + kAp;           // 1 / (2 v1)
    double* const WS = I2 + kAp;           // [wave][4]
    float* const W2 = reinterpret_cast<float*>(lds_d + kDbl);
    float* const W3 = W2 + kH * kSW;
    float* const b1 = W3 + kAp * kSW;
    float* const b2 = b1 + kH;
    float* const b3 = b2 + kH;
    float* const O = b3 + kAp;
    float* const H1 = O + kTile * SO;
    float* const H2 = H1 + kTile * kSW;
    float* const MU = H2 + kTile * kSW;

    if (a.st && a.st->flag) return;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, c = lane & 15, q = lane >> 4;
    const int D = a.D, A = a.A;
    const int oW1 = A, ob1 = oW1 + kH * D, oW2 = ob1 + kH, ob2 = oW2 + kH * kH, oW3 = ob2 + kH, ob3 = oW3 + A * kH;
    const float* __restrict__ th = a.theta;
    const float* __restrict__ dr = a.dir;
    const double ts = a.t;

    // ---- the LDS image of the candidate, and this lane's W1 operands
    // (unrolled, so that the loads of theta and d are in flight together)
    static_assert(kH * kH % kThreads == 0 && kAp * kH % kThreads == 0, "whole passes");
#pragma unroll
    for (int p = 0; p < kH * kH / kThreads; ++p) {
        const int i = tid + kThreads * p;
        W2[(i >> 6) * kSW + (i & 63)] = candidate(th, dr, oW2 + i, ts);
    }
#pragma unroll
    for (int p = 0; p < kAp * kH / kThreads; ++p) {
        const int i = tid + kThreads * p;
        W3[(i >> 6) * kSW + (i & 63)] = (i >> 6) < A ? candidate(th, dr, oW3 + i, ts) : 0.0f;
    }
    if (tid < kH) {
        b1[tid] = candidate(th, dr, ob1 + tid, ts);
        b2[tid] = candidate(th, dr, ob2 + tid, ts);
    }
    if (tid < kAp) {
        const bool in = tid < A;
        b3[tid] = in ? candidate(th, dr, ob3 + tid, ts) : 0.0f;
        const double ls = in ? (double)candidate(th, dr, tid, ts) : 0.0;
        const double v1 = exp(2.0 * ls);
        LS[tid] = ls;
        I1[tid] = 1.0 / (v1 + kEps);
        I2[tid] = 1.0 / (2.0 * v1);
    }
    for (int i = tid; i < kTile * SO; i += kThreads) O[i] = 0.0f;   // the columns past D stay zero
    float w1[KS1];
#pragma unroll
    for (int s = 0; s < KS1; ++s) {
        const int k = 4 * s + q;
        w1[s] = k < D ? candidate(th, dr, oW1 + (16 * w + c) * D + k, ts) : 0.0f;
    }
    // element tid + 256 j of a tile (its rows are contiguous in obs) -> its place in O; the same for every tile
    int off[KS1];
#pragma unroll
    for (int j = 0; j < KS1; ++j) {
        const int i = tid + kThreads * j;
        off[j] = i < kTile * D ? (i / D) * SO + (i % D) : -1;
    }
    float pf[KS1];
    auto load_tile = [&](int t) {
        const float* __restrict__ src = a.obs + (size_t)t * kTile * D;
        const int rows = a.B - t * kTile < kTile ? a.B - t * kTile : kTile;
        const int n = rows * D;                                 // nothing past row B - 1 is read
#pragma unroll
        for (int j = 0; j < KS1; ++j) pf[j] = tid + kThreads * j < n ? src[tid + kThreads * j] : 0.0f;
    };

    const int row = tid >> 2, part = tid & 3;                   // stage 4: row 16 w + (lane >> 2), the actions part, part + 4, ...
    double run[4] = {0.0, 0.0, 0.0, 0.0};                       // the wave's running sums

    int t = blockIdx.x;
    if (t < a.tiles) load_tile(t);
    wg_sync_lds();                                              // O is zero before the first rows land in it
    while (t < a.tiles) {
#pragma unroll
        for (int j = 0; j < KS1; ++j)
            if (off[j] >= 0) O[off[j]] = pf[j];
        const int tn = t + gridDim.x;
        if (tn < a.tiles) load_tile(tn);                        // in flight during the stages
        // this lane's share of its row of the batch, in flight too; nothing past row B - 1 is read
        const int64_t grow = (int64_t)t * kTile + row;
        const bool valid = grow < a.B;
        float r_adv = 0.0f, r_lpo = 0.0f, r_adc = 0.0f, r_act[4], r_muo[4], r_lso[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ac = part + 4 * k;
            const bool in = valid && ac < A;
            r_act[k] = in ? a.act[grow * A + ac] : 0.0f;
            r_muo[k] = in ? a.mu_old[grow * A + ac] : 0.0f;
            r_lso[k] = in ? a.logstd_old[grow * A + ac] : 0.0f;
        }
        if (valid && part == 0) {
            r_adv = a.adv[grow];
            r_lpo = a.logp_old[grow];
            if (a.adc) r_adc = a.adc[grow];
        }
        wg_sync_lds();

        // ---- 1
        {
            const float bz = b1[16 * w + c];
            mfma_f4 acc[4][kAcc];
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int i = 0; i < kAcc; ++i) acc[rb][i] = splat(i == 0 ? bz : 0.0f);
#pragma unroll
            for (int s = 0; s < KS1; ++s) {
#pragma unroll
                for (int rb = 0; rb < 4; ++rb)
                    acc[rb][s % kAcc] = GXB_MFMA(O[(16 * rb + c) * SO + 4 * s + q], w1[s], acc[rb][s % kAcc]);
            }
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) {
                const mfma_f4 z = sum_acc(acc[rb]);
#pragma unroll
                for (int r = 0; r < 4; ++r) H1[(16 * rb + 4 * q + r) * kSW + 16 * w + c] = tanh_act(z[r]);
            }
        }
        wg_sync_lds();
        // ---- 2
        {
            const float bz = b2[16 * w + c];
            mfma_f4 acc[4][kAcc];
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int i = 0; i < kAcc; ++i) acc[rb][i] = splat(i == 0 ? bz : 0.0f);
#pragma unroll
            for (int s = 0; s < kH / 4; ++s) {
                const float bw = W2[(16 * w + c) * kSW + 4 * s + q];
#pragma unroll
                for (int rb = 0; rb < 4; ++rb)
                    acc[rb][s % kAcc] = GXB_MFMA(H1[(16 * rb + c) * kSW + 4 * s + q], bw, acc[rb][s % kAcc]);
            }
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) {
                const mfma_f4 z = sum_acc(acc[rb]);
#pragma unroll
                for (int r = 0; r < 4; ++r) H2[(16 * rb + 4 * q + r) * kSW + 16 * w + c] = tanh_act(z[r]);
            }
        }
        wg_sync_lds();
        // ---- 3: this wave's 16 rows
        {
            mfma_f4 acc[kAcc];
#pragma unroll
            for (int i = 0; i < kAcc; ++i) acc[i] = splat(i == 0 ? b3[c] : 0.0f);
#pragma unroll
            for (int s = 0; s < kH / 4; ++s)
                acc[s % kAcc] = GXB_MFMA(H2[(16 * w + c) * kSW + 4 * s + q], W3[c * kSW + 4 * s + q], acc[s % kAcc]);
            const mfma_f4 m = sum_acc(acc);
#pragma unroll
            for (int r = 0; r < 4; ++r) MU[(16 * w + 4 * q + r) * kSU + c] = m[r];
        }
        wg_sync_lds();
        // ---- 4: the rows
        {
            double kls = 0.0, lps = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int ac = part + 4 * k;
                if (ac < A) {
                    const double mu = (double)MU[row * kSU + ac], ls = LS[ac], lso = (double)r_lso[k];
                    const double dm = mu - (double)r_muo[k], da = (double)r_act[k] - mu;
                    kls += 0.5 * ((dm * dm + exp(2.0 * lso)) * I1[ac] - 1.0) + (ls - lso);
                    lps += -(da * da) * I2[ac] - ls - kHalfLog2Pi;
                }
            }
            kls += __shfl_xor(kls, 1);
            lps += __shfl_xor(lps, 1);
            kls += __shfl_xor(kls, 2);
            lps += __shfl_xor(lps, 2);
            const float klr = (float)kls, lp = (float)lps;
            const float diff = lp - r_lpo;
            const float ratio = (float)exp((double)diff);
            const bool on = valid && part == 0;                 // selection, never a product with zero
            double v[4];
            v[0] = on ? (double)klr : 0.0;
            v[1] = on ? (double)(ratio * r_adv) : 0.0;
            v[2] = on ? (double)(ratio * r_adc) : 0.0;
            v[3] = on ? (double)(r_lpo - lp) : 0.0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                double s = v[i];
#pragma unroll
                for (int m = 4; m < 64; m <<= 1) s += __shfl_xor(s, m);
                run[i] += s;
            }
        }
        t = tn;                                                 // the next tile's stage 3 writes MU after three barriers
    }

    // ---- the partial: the waves' sums in wave order
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) WS[4 * w + i] = run[i];
    }
    wg_sync_lds();
    if (tid < 4) a.partial[(size_t)blockIdx.x * 4 + tid] = ((WS[tid] + WS[4 + tid]) + WS[8 + tid]) + WS[12 + tid];
}

enum Mode { kEvaluate = 0, kFirst = 1, kCandidate = 2 };

struct DecideArgs {
    int mode, B, P, grid, j, has_adc;
    double t;
    const double* partial;
    const float *theta, *dir;
    const double* criteria;   // target_kl, cost_margin, need_loss
    State* st;
    double* row;              // where the four means go: gxb_evaluate's output row, or the trace's
    float* theta_new;
    int32_t* accepted;
    double* means;            // 6
};

__global__ __launch_bounds__(kDecideThreads) void decide_kernel(DecideArgs a)
{
    __shared__ double m[4], sh[kDecideThreads];
    if (a.mode == kCandidate && a.st->flag) return;             // uniform; nobody writes the flag before the barriers below
    const int tid = threadIdx.x;
    // the partials in workgroup order, 256 workgroups at a time through LDS: one load per lane, all in flight together
    // (read one after the other from memory, 256 partials cost 40 us)
    double s = 0.0;
    for (int base = 0; base < a.grid; base += kDecideThreads / 4) {
        const int n = a.grid - base < kDecideThreads / 4 ? a.grid - base : kDecideThreads / 4;
        if (tid < 4 * n) sh[tid] = a.partial[(size_t)base * 4 + tid];
        __syncthreads();
        if (tid < 4) {
#pragma unroll 16
            for (int g = 0; g < n; ++g) s += sh[4 * g + tid];
        }
        __syncthreads();
    }
    if (tid < 4) {
        s = s / (double)a.B;
        m[tid] = tid == 1 ? -s : s;
    }
    __syncthreads();
    if (tid < 4) a.row[tid] = m[tid];
    if (a.mode == kEvaluate) return;
    if (a.mode == kFirst) {
        for (int i = tid; i < a.P; i += kDecideThreads) a.theta_new[i] = a.theta[i];
        if (tid < 4) a.means[tid] = m[tid];
        if (tid == 0) {
            a.st->pi_l_old = (double)(float)m[1];
            a.st->surr_cost_old = (double)(float)m[2];
            a.st->flag = 0;
            *a.accepted = -1;
            a.means[4] = m[1];
            a.means[5] = m[2];
        }
        return;
    }
    const double kl = (double)(float)m[0], pi_l = (double)(float)m[1], surr = (double)(float)m[2];
    const double target_kl = a.criteria[0], margin = a.criteria[1], need_loss = a.criteria[2];
    const bool ok = kl <= target_kl && (need_loss == 0.0 || pi_l <= a.st->pi_l_old) &&
                    (!a.has_adc || surr - a.st->surr_cost_old <= margin);
    if (!ok) return;
    for (int i = tid; i < a.P; i += kDecideThreads) a.theta_new[i] = candidate(a.theta, a.dir, i, a.t);
    if (tid < 4) a.means[tid] = m[tid];
    if (tid == 0) {
        *a.accepted = a.j;
        a.st->flag = 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
gxb_status check_shape(const char* who, int B, int D, int A, int hidden, int workgroups)
{
    if (B < 1 || D < 1 || A < 1) return fail(GXB_ERR_ARG, std::string(who) + ": B, D and A must be at least 1");
    if (workgroups < 0 || workgroups > kMaxWg)
        return fail(GXB_ERR_ARG, std::string(who) + ": workgroups must be 0 (the default) .. " + std::to_string(kMaxWg));
    if (hidden != kH) return fail(GXB_ERR_UNSUPPORTED, std::string(who) + " supports hidden width 64, not " + std::to_string(hidden));
    if (D > kMaxD) return fail(GXB_ERR_UNSUPPORTED, std::string(who) + " supports an observation width <= 128, not " + std::to_string(D));
    if (A % 2 != 0 || A > kAp)
        return fail(GXB_ERR_UNSUPPORTED, std::string(who) + " supports an even action width <= 16, not " + std::to_string(A));
    return GXB_OK;
}

int64_t work_bytes(int grid) { return 32 * (int64_t)grid + (int64_t)sizeof(State); }

template <int KS1>
gxb_status launch_eval(const EvalArgs& a, int grid, hipStream_t s)
{
    constexpr int lds = lds_floats(KS1) * (int)sizeof(float);
    static_assert((KS1 <= kTwoKS1 ? 2 : 1) * lds <= 160 * 1024, "the LDS images fit one CU");
    static_assert(obs_stride(KS1) >= 4 * KS1, "a row of the obs tile holds every k-step");
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&eval_kernel<KS1>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (attr != hipSuccess) return fail(GXB_ERR_HIP, std::string("gxb: hipFuncSetAttribute failed: ") + hipGetErrorString(attr));
    hipLaunchKernelGGL(eval_kernel<KS1>, dim3(grid), dim3(kThreads), lds, s, a);
    return GXB_OK;
}

gxb_status evaluate_at(const EvalArgs& a, int grid, hipStream_t s)
{
    const int ks = (a.D + 3) / 4;   // k-steps of the first layer: the instantiations of gx_fisher.hip
    if (ks <= 4) return launch_eval<4>(a, grid, s);
    if (ks <= 8) return launch_eval<8>(a, grid, s);
    if (ks <= 11) return launch_eval<11>(a, grid, s);
    if (ks <= 12) return launch_eval<12>(a, grid, s);
    if (ks <= 16) return launch_eval<16>(a, grid, s);
    if (ks <= 18) return launch_eval<18>(a, grid, s);
    if (ks <= 24) return launch_eval<24>(a, grid, s);
    return launch_eval<32>(a, grid, s);
}

gxb_status launched(const char* who)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GXB_OK : fail(GXB_ERR_HIP, std::string(who) + " launch failed: " + hipGetErrorString(e));
}

} // namespace

extern "C" const char* gxb_last_error(void) { return g_err.c_str(); }

extern "C" const char* gxb_build_id(void) { return GXB_BUILD_ID; } // guardx_amd/build.py:UPDATE_LIBRARIES["linesearch"].source_hash()

extern "C" int64_t gxb_param_count(int32_t D, int32_t A, int32_t hidden)
{
    return (D < 1 || A < 1 || hidden < 1) ? -1 : param_count(D, A, hidden);
}

extern "C" int32_t gxb_default_workgroups(int32_t B, int32_t D) { return (B < 1 || D < 1) ? 0 : default_workgroups(B, D); }

extern "C" int64_t gxb_work_bytes(int32_t B, int32_t D, int32_t A, int32_t workgroups)
{
    if (check_shape("gxb_work_bytes", B, D, A, kH, workgroups) != GXB_OK) return -1;
    return work_bytes(workgroups ? workgroups : default_workgroups(B, D));
}

extern "C" gxb_status gxb_evaluate(int32_t B, int32_t D, int32_t A, int32_t hidden, const float* d_theta, const float* d_dir,
                                   const float* d_obs, const float* d_act, const float* d_adv, const float* d_logp_old,
                                   const float* d_mu_old, const float* d_logstd_old, const float* d_adc, int32_t n_steps,
                                   void* h_steps, int32_t workgroups, void* d_work, void* d_out, void* stream)
{
    if (!d_theta || !d_dir || !d_obs || !d_act || !d_adv || !d_logp_old || !d_mu_old || !d_logstd_old || !h_steps || !d_work || !d_out)
        return fail(GXB_ERR_ARG, "gxb_evaluate: null pointer");
    if (n_steps < 1) return fail(GXB_ERR_ARG, "gxb_evaluate: n_steps must be at least 1");
    const gxb_status st = check_shape("gxb_evaluate", B, D, A, hidden, workgroups);
    if (st != GXB_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    const int grid = workgroups ? workgroups : default_workgroups(B, D);
    const double* steps = static_cast<const double*>(h_steps);
    EvalArgs e{B, D, A, tiles_of(B), d_theta, d_dir, d_obs, d_act, d_adv, d_logp_old, d_mu_old, d_logstd_old, d_adc, 0.0,
               static_cast<double*>(d_work), nullptr};
    DecideArgs dc{};
    dc.mode = kEvaluate;
    dc.B = B;
    dc.grid = grid;
    dc.partial = e.partial;
    for (int k = 0; k < n_steps; ++k) {
        e.t = steps[k];
        const gxb_status se = evaluate_at(e, grid, s);
        if (se != GXB_OK) return se;
        dc.row = static_cast<double*>(d_out) + 4 * (size_t)k;
        hipLaunchKernelGGL(decide_kernel, dim3(1), dim3(kDecideThreads), 0, s, dc);
    }
    return launched("gxb_evaluate");
}

extern "C" gxb_status gxb_search(int32_t B, int32_t D, int32_t A, int32_t hidden, const float* d_theta, const float* d_dir,
                                 const float* d_obs, const float* d_act, const float* d_adv, const float* d_logp_old,
                                 const float* d_mu_old, const float* d_logstd_old, const float* d_adc, int32_t iters,
                                 void* h_steps, void* d_criteria, int32_t workgroups, void* d_work, float* d_theta_new,
                                 int32_t* d_accepted, void* d_means, void* d_trace, void* stream)
{
    if (!d_theta || !d_dir || !d_obs || !d_act || !d_adv || !d_logp_old || !d_mu_old || !d_logstd_old || !d_criteria || !d_work ||
        !d_theta_new || !d_accepted || !d_means || !d_trace)
        return fail(GXB_ERR_ARG, "gxb_search: null pointer");
    if (iters < 0) return fail(GXB_ERR_ARG, "gxb_search: negative iters");
    if (iters > 0 && !h_steps) return fail(GXB_ERR_ARG, "gxb_search: null pointer");
    if (d_theta_new == d_theta || d_theta_new == d_dir) return fail(GXB_ERR_ARG, "gxb_search: d_theta_new may not alias d_theta or d_dir");
    const gxb_status st = check_shape("gxb_search", B, D, A, hidden, workgroups);
    if (st != GXB_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    const int grid = workgroups ? workgroups : default_workgroups(B, D);
    const double* steps = static_cast<const double*>(h_steps);
    State* state = reinterpret_cast<State*>(static_cast<char*>(d_work) + 32 * (size_t)grid);
    EvalArgs e{B, D, A, tiles_of(B), d_theta, d_dir, d_obs, d_act, d_adv, d_logp_old, d_mu_old, d_logstd_old, d_adc, 0.0,
               static_cast<double*>(d_work), nullptr};
    DecideArgs dc{};
    dc.mode = kFirst;
    dc.B = B;
    dc.P = (int)param_count(D, A, kH);
    dc.grid = grid;
    dc.has_adc = d_adc != nullptr;
    dc.partial = e.partial;
    dc.theta = d_theta;
    dc.dir = d_dir;
    dc.criteria = static_cast<const double*>(d_criteria);
    dc.st = state;
    dc.row = static_cast<double*>(d_trace);
    dc.theta_new = d_theta_new;
    dc.accepted = d_accepted;
    dc.means = static_cast<double*>(d_means);
    gxb_status se = evaluate_at(e, grid, s);                    // t = 0: whatever flag an earlier call left is not looked at
    if (se != GXB_OK) return se;
    hipLaunchKernelGGL(decide_kernel, dim3(1), dim3(kDecideThreads), 0, s, dc);
    e.st = state;
    dc.mode = kCandidate;
    for (int j = 0; j < iters; ++j) {
        e.t = dc.t = steps[j];
        dc.j = j;
        dc.row = static_cast<double*>(d_trace) + 4 * (size_t)(j + 1);
        se = evaluate_at(e, grid, s);
        if (se != GXB_OK) return se;
        hipLaunchKernelGGL(decide_kernel, dim3(1), dim3(kDecideThreads), 0, s, dc);
    }
    return launched("gxb_search");
}
