// gx_vfit.hip -- libguardx_vfit.so (include/guardx_vfit.h): the learners' fit of a value critic (MLP, hidden width 64, one
// linear output) by Adam on the MSE loss, on the caller's stream and without a host synchronisation.  The header fixes the
// arithmetic; this file is its order of work, two launches per iteration:
//
//   grad_kernel    a persistent grid of 4-wave workgroups; workgroup g walks the 64-row tiles g, g + grid, ... of obs, in the
//                  shape of gx_fisher.hip:fvp_kernel without its tangent.  LDS holds W2, W3 and the biases, the tile of obs,
//                  of ret and its activations; W1 is a B operand that a lane never shares (wave w owns the hidden units
//                  16 w .. + 15), so each lane keeps its KS1 of them in registers.  Per tile, with a workgroup barrier (LDS
//                  only) after each stage:
//                    1  z1 = o W1' + b1 -> h1                       (K = pad4 D; four chains: sum_acc)
//                    2  z2 = h1 W2' + b2 -> h2                      (K = 64; four chains)
//                    3  val = h2 W3' + b3 (wave w: rows 16 w ..; W3 is the one live column of the B operand) -> e = val - ret,
//                       u = 2 e / B, 0 for rows past B; e^2 to the wave's running float64 sum
//                    4  gz2 = (u W3)(1 - h2^2) (an outer product: plain float32);  gW3 += u' h2, gb3 += u' 1   (K = 64 rows)
//                    5  gW2 += gz2' h1, gb2 += gz2' 1;  gz1 = (gz2 W2)(1 - h1^2) -> where h2 was
//                    6  gW1 += gz1' o, gb1 += gz1' 1
//                  A bias gradient is one more chain on the A operand its weight gradient loads anyway (B = 1).  The sums
//                  over a tile's 64 rows start from zero and are added to the workgroup's running sums after the stage, so
//                  that no float32 chain is longer than a tile, whatever B is.  The next tile's rows are loaded into
//                  registers while this one is computed.  The workgroup writes its running sums as one partial vector of P
//                  floats and its sum of e^2 (the waves' in wave order) as one float64.
//   step_kernel    one lane per entry of theta: the partial vectors' entries added in workgroup order (float64, rounded once:
//                  g), then Adam in place.  Adam works entry by entry, so the reduction's grid of ceil(P / 256) workgroups
//                  carries it and none waits on another (a single workgroup would read all grid x P partials through one CU).
//                  Workgroup 0 also adds the workgroups' e^2 in workgroup order, staged through LDS 256 at a time, and writes
//                  the loss.  The same kernel serves gxv_gradient (no Adam: g and the loss are written) and gxv_adam_step (no
//                  reduction: g is read).
// No atomics anywhere: the same arguments give the same bits.  tanh_act and sum_acc are gx_fisher.hip's, restated (a shared
// header would move the build ids of the libraries that hold them).
#include "../../include/guardx_vfit.h"
#include "gx_policy.h"
#include <cmath>
#include <string>

#ifndef GXV_BUILD_ID
#define GXV_BUILD_ID "unknown"
#endif

namespace {

using gx::mfma_f4;
using gx::wg_sync_lds;

thread_local std::string g_err;

gxv_status fail(gxv_status st, const std::string& msg)
{
    g_err = msg;
    return st;
}

constexpr int kH = gx::kPolHd;   // hidden width
constexpr int kTile = 64;        // rows of obs per tile
constexpr int kThreads = 256;    // four waves; wave w owns the hidden units 16 w .. 16 w + 15 and, in stage 3, the rows 16 w ..
constexpr int kSW = 66;          // LDS row stride of everything 64 wide: 16 rows x 2 k of a ds_read_b32 group hit 32 banks
constexpr int kDefaultWg = 256;  // one workgroup per CU of the MI355X: W2, the obs tile and three 64 x 64 tiles of
                                 // activations are 84 KB at D <= 64, so two workgroups' images do not fit a CU's 160 KB
constexpr int kMaxWg = 4096;
constexpr int kMaxD = 128;
constexpr int kAcc = 4;          // interleaved chains of a forward product (stages 1 to 3): see sum_acc
constexpr int kDbl = 4;          // float64 at the head of LDS: the waves' sums of e^2

// row stride of the obs tile: at least the 16 NT1 columns stage 6 reads, = 2 mod 32
constexpr int nt1_of(int KS1) { return (KS1 + 3) / 4; }
constexpr int obs_stride(int KS1) { return (16 * nt1_of(KS1) - 2 + 31) / 32 * 32 + 2; }
constexpr int lds_floats(int KS1) { return 2 * kDbl + kH * kSW + 3 * kH + 4 + kTile * obs_stride(KS1) + 3 * kTile * kSW + 2 * kTile; }

int64_t param_count(int D, int h) { return (int64_t)h * D + h + (int64_t)h * h + h + h + 1; }
int tiles_of(int B) { return (int)(((int64_t)B + kTile - 1) / kTile); }
int default_workgroups(int B) { return tiles_of(B) < kDefaultWg ? tiles_of(B) : kDefaultWg; }

struct GradArgs {
    int B, D, tiles;
    const float *obs, *ret, *theta;
    float* partial;     // [grid][P]
    double* sq;         // [grid]
    double two_over_b;  // 2 / B
};

#define GXV_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0)

__device__ __forceinline__ mfma_f4 splat(float v) { return mfma_f4{v, v, v, v}; }

// gx_fisher.hip:sum_acc: the sums over a layer's inputs are kAcc chains, k-step s on chain s mod kAcc, the bias on chain 0,
// added pairwise.  One chain rounds 64 times at the size of its running sum; four round 16 times each at half that size,
// which halves the error of the sum (the Fisher product's record: 7 x its yardstick at B = 1 with one chain, 1.3 x with four).
__device__ __forceinline__ mfma_f4 sum_acc(const mfma_f4 (&a)[kAcc])
{
    static_assert(kAcc == 4, "pairwise over four");
    return (a[0] + a[1]) + (a[2] + a[3]);
}

// gx_fisher.hip:tanh_act: gx::tanh_f has a small absolute error, which below |x| ~ 0.6 is a large relative one, and here every
// activation multiplies gradients; there the odd polynomial x + x^3 P(x^2) of the Cephes single-precision tanh (public
// domain, S. Moshier) takes over: 2.3 ulp at worst over the whole line
__device__ __forceinline__ float tanh_act(float x)
{
    const float z = x * x;
    float p = fmaf(z, -5.70498872745e-3f, 2.06390887954e-2f);
    p = fmaf(z, p, -5.37397155531e-2f);
    p = fmaf(z, p, 1.33314422036e-1f);
    p = fmaf(z, p, -3.33332819422e-1f);
    const float small = fmaf(z * x, p, x);                      // x = -0: (+0) + (-0) = +0, hence the copysignf
    return fabsf(x) < 0.625f ? copysignf(small, x) : gx::tanh_f(x);
}

// test infrastructure (gxv_tanh_act): tanh_act by itself, one lane per element
__global__ __launch_bounds__(kThreads) void tanh_act_kernel(int n, const float* __restrict__ x, float* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) out[i] = tanh_act(x[i]);
}

template <int KS1>
__global__ __launch_bounds__(kThreads) void grad_kernel(GradArgs a)
{
    constexpr int NT1 = nt1_of(KS1), SO = obs_stride(KS1);
    extern __shared__ double lds_d[];
    double* const WS = lds_d;              // [wave]
    float* const W2 = reinterpret_cast<float*>(lds_d + kDbl);
    float* const W3 = W2 + kH * kSW;
    float* const b1 = W3 + kH;
    float* const b2 = b1 + kH;
    float* const b3 = b2 + kH;             // 1 (4 reserved)
    float* const O = b3 + 4;
    float* const H1 = O + kTile * SO;
    float* const H2 = H1 + kTile * kSW;    // h2, then gz1
    float* const GZ2 = H2 + kTile * kSW;
    float* const U = GZ2 + kTile * kSW;    // 64
    float* const R = U + kTile;            // 64: the tile of ret

    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, c = lane & 15, q = lane >> 4;
    const int D = a.D;
    const int P = kH * D + kH + kH * kH + kH + kH + 1;
    const int oW1 = 0, ob1 = oW1 + kH * D, oW2 = ob1 + kH, ob2 = oW2 + kH * kH, oW3 = ob2 + kH, ob3 = oW3 + kH;
    const float* __restrict__ th = a.theta;

    // ---- the LDS image of theta, and this lane's W1 operands
    static_assert(kH * kH % kThreads == 0, "whole passes");
#pragma unroll
    for (int p = 0; p < kH * kH / kThreads; ++p) {
        const int i = tid + kThreads * p;
        W2[(i >> 6) * kSW + (i & 63)] = th[oW2 + i];
    }
    if (tid < kH) {
        b1[tid] = th[ob1 + tid];
        b2[tid] = th[ob2 + tid];
        W3[tid] = th[oW3 + tid];
    }
    if (tid == 0) b3[0] = th[ob3];
    for (int i = tid; i < kTile * SO; i += kThreads) O[i] = 0.0f;   // the columns past D stay zero
    float w1[KS1];
#pragma unroll
    for (int s = 0; s < KS1; ++s) {
        const int k = 4 * s + q;
        w1[s] = k < D ? th[oW1 + (16 * w + c) * D + k] : 0.0f;
    }
    // element tid + 256 j of a tile (its rows are contiguous in obs) -> its place in O; the same for every tile
    int off[KS1];
#pragma unroll
    for (int j = 0; j < KS1; ++j) {
        const int i = tid + kThreads * j;
        off[j] = i < kTile * D ? (i / D) * SO + (i % D) : -1;
    }
    float pf[KS1], pr = 0.0f;
    auto load_tile = [&](int t) {
        const float* __restrict__ src = a.obs + (size_t)t * kTile * D;
        const int rows = a.B - t * kTile < kTile ? a.B - t * kTile : kTile;
        const int n = rows * D;                                 // nothing past row B - 1 is read
#pragma unroll
        for (int j = 0; j < KS1; ++j) pf[j] = tid + kThreads * j < n ? src[tid + kThreads * j] : 0.0f;
        pr = tid < rows ? a.ret[(size_t)t * kTile + tid] : 0.0f;
    };

    // the workgroup's running sums: W1 (NT1 column tiles), W2 (4), W3 (row 0 of this wave's tile), the three biases
    mfma_f4 rW1[NT1], rW2[4], rW3 = splat(0.0f), rb1 = splat(0.0f), rb2 = splat(0.0f), rb3 = splat(0.0f);
#pragma unroll
    for (int n = 0; n < NT1; ++n) rW1[n] = splat(0.0f);
#pragma unroll
    for (int n = 0; n < 4; ++n) rW2[n] = splat(0.0f);
    double run = 0.0;                                           // the wave's sum of e^2

    int t = blockIdx.x;
    if (t < a.tiles) load_tile(t);
    wg_sync_lds();                                              // O is zero before the first rows land in it
    while (t < a.tiles) {
#pragma unroll
        for (int j = 0; j < KS1; ++j)
            if (off[j] >= 0) O[off[j]] = pf[j];
        if (tid < kTile) R[tid] = pr;
        const int tn = t + gridDim.x;
        if (tn < a.tiles) load_tile(tn);                        // in flight during the six stages
        wg_sync_lds();

        float d1[4][4], d2[4][4];                               // 1 - h1^2, 1 - h2^2 of this lane's outputs
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
                    acc[rb][s % kAcc] = GXV_MFMA(O[(16 * rb + c) * SO + 4 * s + q], w1[s], acc[rb][s % kAcc]);
            }
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) {
                const mfma_f4 z = sum_acc(acc[rb]);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float h = tanh_act(z[r]);
                    d1[rb][r] = fmaf(-h, h, 1.0f);
                    H1[(16 * rb + 4 * q + r) * kSW + 16 * w + c] = h;
                }
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
                    acc[rb][s % kAcc] = GXV_MFMA(H1[(16 * rb + c) * kSW + 4 * s + q], bw, acc[rb][s % kAcc]);
            }
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) {
                const mfma_f4 z = sum_acc(acc[rb]);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float h = tanh_act(z[r]);
                    d2[rb][r] = fmaf(-h, h, 1.0f);
                    H2[(16 * rb + 4 * q + r) * kSW + 16 * w + c] = h;
                }
            }
        }
        wg_sync_lds();
        // ---- 3: this wave's 16 rows; column 0 of the product is val
        {
            mfma_f4 acc[kAcc];
#pragma unroll
            for (int i = 0; i < kAcc; ++i) acc[i] = splat(i == 0 ? b3[0] : 0.0f);
#pragma unroll
            for (int s = 0; s < kH / 4; ++s) {
                const float bw = c == 0 ? W3[4 * s + q] : 0.0f;
                acc[s % kAcc] = GXV_MFMA(H2[(16 * w + c) * kSW + 4 * s + q], bw, acc[s % kAcc]);
            }
            const mfma_f4 val = sum_acc(acc);
            double sq = 0.0;
            if (c == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * w + 4 * q + r;
                    const bool valid = (int64_t)t * kTile + row < a.B;      // selection, never a product with zero
                    const float e = val[r] - R[row];
                    U[row] = valid ? (float)((double)e * a.two_over_b) : 0.0f;
                    sq += valid ? (double)e * (double)e : 0.0;
                }
            }
            sq += __shfl_xor(sq, 16);
            sq += __shfl_xor(sq, 32);
            run += sq;                                          // the lanes c == 0 of the wave hold its sum
        }
        wg_sync_lds();
        // ---- 4
        {
            const float w3 = W3[16 * w + c];
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * rb + 4 * q + r;
                    GZ2[row * kSW + 16 * w + c] = (U[row] * w3) * d2[rb][r];
                }
            mfma_f4 t3 = splat(0.0f), tb = splat(0.0f);
#pragma unroll
            for (int s = 0; s < kTile / 4; ++s) {
                const float av = c == 0 ? U[4 * s + q] : 0.0f;  // row 0 of the A operand: the critic's one output
                t3 = GXV_MFMA(av, H2[(4 * s + q) * kSW + 16 * w + c], t3);
                tb = GXV_MFMA(av, 1.0f, tb);
            }
            rW3 += t3;
            rb3 += tb;
        }
        wg_sync_lds();
        // ---- 5
        {
            mfma_f4 t2[4], tb = splat(0.0f), z[4];
#pragma unroll
            for (int n = 0; n < 4; ++n) t2[n] = splat(0.0f);
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) z[rb] = splat(0.0f);
#pragma unroll
            for (int s = 0; s < kTile / 4; ++s) {
                const float av = GZ2[(4 * s + q) * kSW + 16 * w + c];
#pragma unroll
                for (int n = 0; n < 4; ++n) t2[n] = GXV_MFMA(av, H1[(4 * s + q) * kSW + 16 * n + c], t2[n]);
                tb = GXV_MFMA(av, 1.0f, tb);
                const float bv = W2[(4 * s + q) * kSW + 16 * w + c];
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) z[rb] = GXV_MFMA(GZ2[(16 * rb + c) * kSW + 4 * s + q], bv, z[rb]);
            }
#pragma unroll
            for (int n = 0; n < 4; ++n) rW2[n] += t2[n];
            rb2 += tb;
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)                      // h2 was last read in stage 4
#pragma unroll
                for (int r = 0; r < 4; ++r) H2[(16 * rb + 4 * q + r) * kSW + 16 * w + c] = z[rb][r] * d1[rb][r];
        }
        wg_sync_lds();
        // ---- 6
        {
            mfma_f4 t1[NT1], tb = splat(0.0f);
#pragma unroll
            for (int n = 0; n < NT1; ++n) t1[n] = splat(0.0f);
#pragma unroll
            for (int s = 0; s < kTile / 4; ++s) {
                const float av = H2[(4 * s + q) * kSW + 16 * w + c];
#pragma unroll
                for (int n = 0; n < NT1; ++n) t1[n] = GXV_MFMA(av, O[(4 * s + q) * SO + 16 * n + c], t1[n]);
                tb = GXV_MFMA(av, 1.0f, tb);
            }
#pragma unroll
            for (int n = 0; n < NT1; ++n) rW1[n] += t1[n];
            rb1 += tb;
        }
        wg_sync_lds();                                          // O, R and gz1 are free for the next tile
        t = tn;
    }

    // ---- the partial vector: an accumulator's entry r is row 4 q + r, column c of its 16 x 16 tile
    float* __restrict__ out = a.partial + (size_t)blockIdx.x * P;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int unit = 16 * w + 4 * q + r;
#pragma unroll
        for (int n = 0; n < NT1; ++n)
            if (16 * n + c < D) out[oW1 + unit * D + 16 * n + c] = rW1[n][r];
#pragma unroll
        for (int n = 0; n < 4; ++n) out[oW2 + unit * kH + 16 * n + c] = rW2[n][r];
        if (c == 0) {
            out[ob1 + unit] = rb1[r];
            out[ob2 + unit] = rb2[r];
        }
    }
    if (q == 0) {
        out[oW3 + 16 * w + c] = rW3[0];
        if (w == 0 && c == 0) out[ob3] = rb3[0];
    }
    if (lane == 0) WS[w] = run;
    wg_sync_lds();
    if (tid == 0) a.sq[blockIdx.x] = ((WS[0] + WS[1]) + WS[2]) + WS[3];
}

struct StepArgs {
    int P, grid, B, adam;
    const float* partial;   // [grid][P], or null: the gradient is g_in
    const double* sq;       // [grid], or null: no loss
    const float* g_in;
    float *g_out, *loss_out;                                    // either may be null
    float *theta, *m, *v;                                       // adam != 0
    double b1, b2, omb1, omb2, eps, step_size, bc2_sqrt;        // 1 - b1, 1 - b2, lr / (1 - b1^t), sqrt(1 - b2^t)
};

__global__ __launch_bounds__(kThreads) void step_kernel(StepArgs a)
{
    __shared__ double sh[kThreads];
    const int tid = threadIdx.x, i = blockIdx.x * kThreads + tid;
    if (i < a.P) {
        float gi;
        if (a.partial) {
            double s = 0.0;
#pragma unroll 8
            for (int g = 0; g < a.grid; ++g) s += (double)a.partial[(size_t)g * a.P + i];
            gi = (float)s;
        } else {
            gi = a.g_in[i];
        }
        if (a.g_out) a.g_out[i] = gi;
        if (a.adam) {
            const double g = (double)gi;
            const double M = a.b1 * (double)a.m[i] + a.omb1 * g;
            const double V = a.b2 * (double)a.v[i] + a.omb2 * (g * g);
            const double T = (double)a.theta[i] - a.step_size * (M / (sqrt(V) / a.bc2_sqrt + a.eps));
            a.m[i] = (float)M;
            a.v[i] = (float)V;
            a.theta[i] = (float)T;
        }
    }
    if (blockIdx.x != 0 || !a.sq || !a.loss_out) return;        // uniform over the workgroup
    // the workgroups' sums of e^2 in workgroup order, 256 at a time through LDS: one load per lane, all in flight together
    double s = 0.0;
    for (int base = 0; base < a.grid; base += kThreads) {
        const int n = a.grid - base < kThreads ? a.grid - base : kThreads;
        if (tid < n) sh[tid] = a.sq[base + tid];
        __syncthreads();
        if (tid == 0) {
#pragma unroll 16
            for (int g = 0; g < n; ++g) s += sh[g];
        }
        __syncthreads();
    }
    if (tid == 0) a.loss_out[0] = (float)(s / (double)a.B);
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
gxv_status check_shape(const char* who, int B, int D, int hidden, int workgroups)
{
    if (B < 1 || D < 1) return fail(GXV_ERR_ARG, std::string(who) + ": B and D must be at least 1");
    if (workgroups < 0 || workgroups > kMaxWg)
        return fail(GXV_ERR_ARG, std::string(who) + ": workgroups must be 0 (the default) .. " + std::to_string(kMaxWg));
    if (hidden != kH) return fail(GXV_ERR_UNSUPPORTED, std::string(who) + " supports hidden width 64, not " + std::to_string(hidden));
    if (D > kMaxD) return fail(GXV_ERR_UNSUPPORTED, std::string(who) + " supports an observation width <= 128, not " + std::to_string(D));
    return GXV_OK;
}

int64_t partial_bytes(int64_t P, int grid) { return (4 * (int64_t)grid * P + 7) / 8 * 8; }
int64_t work_bytes(int64_t P, int grid) { return partial_bytes(P, grid) + 8 * (int64_t)grid; }

template <int KS1>
gxv_status launch_grad(const GradArgs& a, int grid, hipStream_t s)
{
    constexpr int lds = lds_floats(KS1) * (int)sizeof(float);
    static_assert(lds <= 160 * 1024, "the LDS image fits one CU");
    static_assert(obs_stride(KS1) >= 4 * KS1 && obs_stride(KS1) >= 16 * nt1_of(KS1), "a row of the obs tile holds what stages 1 and 6 read");
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&grad_kernel<KS1>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (attr != hipSuccess) return fail(GXV_ERR_HIP, std::string("gxv: hipFuncSetAttribute failed: ") + hipGetErrorString(attr));
    hipLaunchKernelGGL(grad_kernel<KS1>, dim3(grid), dim3(kThreads), lds, s, a);
    return GXV_OK;
}

gxv_status gradient_at(const GradArgs& a, int grid, hipStream_t s)
{
    const int ks = (a.D + 3) / 4;   // k-steps of the first layer: the instantiations of gx_fisher.hip
    if (ks <= 4) return launch_grad<4>(a, grid, s);
    if (ks <= 8) return launch_grad<8>(a, grid, s);
    if (ks <= 11) return launch_grad<11>(a, grid, s);
    if (ks <= 12) return launch_grad<12>(a, grid, s);
    if (ks <= 16) return launch_grad<16>(a, grid, s);
    if (ks <= 18) return launch_grad<18>(a, grid, s);
    if (ks <= 24) return launch_grad<24>(a, grid, s);
    return launch_grad<32>(a, grid, s);
}

GradArgs grad_args(int B, int D, const float* obs, const float* ret, const float* theta, void* work, int grid)
{
    GradArgs a;
    a.B = B;
    a.D = D;
    a.tiles = tiles_of(B);
    a.obs = obs;
    a.ret = ret;
    a.theta = theta;
    a.partial = static_cast<float*>(work);
    a.sq = reinterpret_cast<double*>(static_cast<char*>(work) + partial_bytes(param_count(D, kH), grid));
    a.two_over_b = 2.0 / (double)B;
    return a;
}

// the hyperparameters of one step: h = lr, b1, b2, eps; p = b1^t, b2^t
void set_adam(StepArgs& st, const double* h, const double* p)
{
    st.adam = 1;
    st.b1 = h[1];
    st.b2 = h[2];
    st.omb1 = 1.0 - h[1];
    st.omb2 = 1.0 - h[2];
    st.eps = h[3];
    st.step_size = h[0] / (1.0 - p[0]);
    st.bc2_sqrt = std::sqrt(1.0 - p[1]);
}

void launch_step(const StepArgs& st, hipStream_t s)
{
    hipLaunchKernelGGL(step_kernel, dim3((st.P + kThreads - 1) / kThreads), dim3(kThreads), 0, s, st);
}

gxv_status launched(const char* who)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GXV_OK : fail(GXV_ERR_HIP, std::string(who) + " launch failed: " + hipGetErrorString(e));
}

} // namespace

extern "C" const char* gxv_last_error(void) { return g_err.c_str(); }

extern "C" const char* gxv_build_id(void) { return GXV_BUILD_ID; } // guardx_amd/build.py:FIT_LIBRARIES["vfit"].source_hash()

extern "C" int64_t gxv_param_count(int32_t D, int32_t hidden) { return (D < 1 || hidden < 1) ? -1 : param_count(D, hidden); }

extern "C" int32_t gxv_default_workgroups(int32_t B) { return B < 1 ? 0 : default_workgroups(B); }

extern "C" int64_t gxv_work_bytes(int32_t B, int32_t D, int32_t workgroups)
{
    if (check_shape("gxv_work_bytes", B, D, kH, workgroups) != GXV_OK) return -1;
    return work_bytes(param_count(D, kH), workgroups ? workgroups : default_workgroups(B));
}

extern "C" gxv_status gxv_tanh_act(int32_t n, const float* d_x, float* d_out, void* stream)
{
    if (!d_x || !d_out) return fail(GXV_ERR_ARG, "gxv_tanh_act: null pointer");
    if (n < 0) return fail(GXV_ERR_ARG, "gxv_tanh_act: negative n");
    if (n == 0) return GXV_OK;
    const unsigned blocks = (unsigned)(((int64_t)n + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(tanh_act_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, n, d_x, d_out);
    return launched("gxv_tanh_act");
}

extern "C" gxv_status gxv_gradient(int32_t B, int32_t D, int32_t hidden, const float* d_theta, const float* d_obs,
                                   const float* d_ret, int32_t workgroups, void* d_work, float* d_g, float* d_loss, void* stream)
{
    if (!d_theta || !d_obs || !d_ret || !d_work || !d_g || !d_loss) return fail(GXV_ERR_ARG, "gxv_gradient: null pointer");
    const gxv_status sc = check_shape("gxv_gradient", B, D, hidden, workgroups);
    if (sc != GXV_OK) return sc;
    hipStream_t s = (hipStream_t)stream;
    const int grid = workgroups ? workgroups : default_workgroups(B);
    const GradArgs a = grad_args(B, D, d_obs, d_ret, d_theta, d_work, grid);
    const gxv_status sg = gradient_at(a, grid, s);
    if (sg != GXV_OK) return sg;
    StepArgs st{};
    st.P = (int)param_count(D, kH);
    st.grid = grid;
    st.B = B;
    st.partial = a.partial;
    st.sq = a.sq;
    st.g_out = d_g;
    st.loss_out = d_loss;
    launch_step(st, s);
    return launched("gxv_gradient");
}

extern "C" gxv_status gxv_adam_step(int32_t P, float* d_theta, float* d_m, float* d_v, const float* d_g, void* h_hyper, void* stream)
{
    if (!d_theta || !d_m || !d_v || !d_g || !h_hyper) return fail(GXV_ERR_ARG, "gxv_adam_step: null pointer");
    if (P < 1) return fail(GXV_ERR_ARG, "gxv_adam_step: P must be at least 1");
    const double* h = static_cast<const double*>(h_hyper);
    StepArgs st{};
    st.P = P;
    st.g_in = d_g;
    st.theta = d_theta;
    st.m = d_m;
    st.v = d_v;
    set_adam(st, h, h + 4);
    launch_step(st, (hipStream_t)stream);
    return launched("gxv_adam_step");
}

extern "C" gxv_status gxv_fit(int32_t B, int32_t D, int32_t hidden, float* d_theta, float* d_m, float* d_v, int64_t step0,
                              const float* d_obs, const float* d_ret, int32_t iters, void* h_hyper, int32_t workgroups,
                              void* d_work, float* d_loss, void* stream)
{
    if (!d_theta || !d_m || !d_v || !d_obs || !d_ret || !h_hyper || !d_work || !d_loss) return fail(GXV_ERR_ARG, "gxv_fit: null pointer");
    if (iters < 0) return fail(GXV_ERR_ARG, "gxv_fit: negative iters");
    if (step0 < 0) return fail(GXV_ERR_ARG, "gxv_fit: negative step0");
    const gxv_status sc = check_shape("gxv_fit", B, D, hidden, workgroups);
    if (sc != GXV_OK) return sc;
    if (iters == 0) return GXV_OK;
    hipStream_t s = (hipStream_t)stream;
    const int grid = workgroups ? workgroups : default_workgroups(B);
    const double* h = static_cast<const double*>(h_hyper);
    const GradArgs a = grad_args(B, D, d_obs, d_ret, d_theta, d_work, grid);
    StepArgs st{};
    st.P = (int)param_count(D, kH);
    st.grid = grid;
    st.B = B;
    st.partial = a.partial;
    st.sq = a.sq;
    st.theta = d_theta;
    st.m = d_m;
    st.v = d_v;
    for (int i = 0; i < iters; ++i) {
        const gxv_status sg = gradient_at(a, grid, s);
        if (sg != GXV_OK) return sg;
        set_adam(st, h, h + 4 + 2 * (size_t)i);
        st.loss_out = d_loss + i;
        launch_step(st, s);
    }
    return launched("gxv_fit");
}
