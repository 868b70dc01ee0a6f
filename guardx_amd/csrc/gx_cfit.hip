// gx_cfit.hip -- libguardx_cfit.so (include/guardx_cfit.h): the fit of the safety critics (usl / lpg's c_net and scpo's v_net
// under Softplus, safelayer's g_net under its dot product with the action) by Adam on a row-weighted squared loss, on the
// caller's stream and without a host synchronisation.  The header fixes the arithmetic; this file is its order of work, two
// launches per iteration:
//
//   grad_kernel<KS1, DOT>   a persistent grid of 4-wave workgroups; workgroup g walks the 64-row tiles g, g + grid, ... of x, in
//                  the shape of gx_vfit.hip:grad_kernel (DOT = false: one output, identity or Softplus by an argument) and of
//                  gx_pgrad.hip:grad_kernel in its one-gradient form (DOT = true: the 16-column head).  LDS holds W2, W3 and
//                  the biases, the tile of x, of y, of the weights and of the offsets, and the activations; W1 is a B operand
//                  that a lane never shares (wave w owns the hidden units 16 w .. + 15), so each lane keeps its KS1 of them in
//                  registers.  Per tile, with a workgroup barrier (LDS only) after each stage:
//                    0  the tile's weights land in LDS; then its rows of x, those of a row whose weight is 0 as zeros
//                    1  z1 = x W1' + b1 -> h1                       (K = pad4 Din; four chains: sum_acc)
//                    2  z2 = h1 W2' + b2 -> h2                      (K = 64; four chains)
//                    3  z = h2 W3' + b3                             (wave w: rows 16 w ..)
//                    R  the lanes that own a row: f, e = f - y, the row's weight, dz = 2 w e f' (0 for a dead row, by
//                       selection), w e^2 and w to the lane's running float64 sums.  One output: the lanes c == 0 of stage 3,
//                       inside it.  DOT: lane 4 i + p of wave w has row 16 w + i and the actions p, p + 4, ...
//                    4  gz2 = (dz W3)(1 - h2^2);  gW3 += dz' h2, gb3 += dz' 1
//                    5  gW2 += gz2' h1, gb2 += gz2' 1;  gz1 = (gz2 W2)(1 - h1^2) -> where h2 was
//                    6  gW1 += gz1' x, gb1 += gz1' 1
//                  The sums over a tile's 64 rows start from zero and are added to the workgroup's running sums after the
//                  stage, so that no float32 chain is longer than a tile.  The next tile's rows are loaded into registers
//                  while this one is computed.  The workgroup writes its running sums as one partial vector of P floats, not
//                  yet divided by W, and two float64: its sums of w e^2 and of w.
//   step_kernel    one lane per entry of theta.  Every workgroup adds the workgroups' sums of w in workgroup order (staged
//                  through LDS 256 at a time) to W; then the partial vectors' entries added in workgroup order in float64,
//                  divided by W, rounded once: g; then Adam in place.  Workgroup 0 adds the sums of w e^2 the same way and
//                  writes the loss and W.  The same kernel serves gxq_gradient (no Adam: g is written).
// No atomics anywhere: the same arguments give the same bits.  tanh_act and sum_acc are gx_fisher.hip's, softplus_f is
// gx_step.h's and softplus_grad_f gx_qcritic.h's, restated: those two headers carry the step libraries' host side and the Q
// libraries' workgroup size with them.  gxq_softplus_probe and tests/test_gpu_cfit.py hold the restatements to the bits.
#include "../../include/guardx_cfit.h"
#include "gx_policy.h"
#include <cmath>
#include <string>

#ifndef GXQ_BUILD_ID
#define GXQ_BUILD_ID "unknown"
#endif

namespace {

using gx::mfma_f4;
using gx::wg_sync_lds;

thread_local std::string g_err;

gxq_status fail(gxq_status st, const std::string& msg)
{
    g_err = msg;
    return st;
}

constexpr int kH = gx::kPolHd;   // hidden width
constexpr int kTile = 64;        // rows of x per tile
constexpr int kThreads = 256;    // four waves; wave w owns the hidden units 16 w .. 16 w + 15 and, in stage 3, the rows 16 w ..
constexpr int kAp = 16;          // the output width of the DOT head padded to one MFMA tile
constexpr int kSW = 66;          // LDS row stride of everything 64 wide: 16 rows x 2 k of a ds_read_b32 group hit 32 banks
constexpr int kSU = 18;          // ... of z and dz of the DOT head (64 x 16)
constexpr int kDefaultWg = 256;  // one workgroup per CU of the MI355X: the LDS image is over half a CU's 160 KB
constexpr int kMaxWg = 4096;
constexpr int kMaxD = 128;
constexpr int kAcc = 4;          // interleaved chains of a forward product (stages 1 to 3): see sum_acc
constexpr int kDbl = 8;          // float64 at the head of LDS: the waves' sums of w e^2 and of w

// row stride of the x tile: at least the 16 NT1 columns stage 6 reads, = 2 mod 32
constexpr int nt1_of(int KS1) { return (KS1 + 3) / 4; }
constexpr int obs_stride(int KS1) { return (16 * nt1_of(KS1) - 2 + 31) / 32 * 32 + 2; }
// W2, W3, b1 b2 b3, X, H1, H2 (then gz1), GZ2, the tile's y, weights and offsets, then U (one output) or Z and DZ (DOT)
constexpr int lds_floats(int KS1, bool DOT)
{
    return 2 * kDbl + kH * kSW + (DOT ? kAp * kSW : kH) + 2 * kH + kAp + kTile * obs_stride(KS1) + 3 * kTile * kSW + 3 * kTile +
           (DOT ? 2 * kTile * kSU : kTile);
}

int64_t param_count(int D, int A, int h) { return (int64_t)h * D + h + (int64_t)h * h + h + (int64_t)A * h + A; }
int tiles_of(int B) { return (int)(((int64_t)B + kTile - 1) / kTile); }
int default_workgroups(int B) { return tiles_of(B) < kDefaultWg ? tiles_of(B) : kDefaultWg; }

struct GradArgs {
    int B, D, A, tiles, softplus;
    const float *theta, *x, *y, *w, *act, *off;   // w and off may be null; act is read by the DOT head alone
    float* partial;     // [grid][P]
    double* sums;       // [grid][2]: w e^2, w
};

#define GXQ_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0)

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

// gx_step.h:softplus_f: Softplus as torch evaluates it (beta = 1, threshold = 20): x > 20 ? x : log1p(exp(x)), in the form
// that neither overflows nor loses the small tail: max(x, 0) + log1p(exp(-|x|)), log1p(u) through the project's log:
// w = fl(1 + u); log(w) u / (w - 1), and u itself once 1 + u rounds to 1.  A NaN comes out as a NaN.
__device__ __forceinline__ float softplus_f(float x)
{
    if (x > 20.0f) return x;
    const float u = gx::exp_f(-fabsf(x));
    const float w = 1.0f + u;
    const float l1p = (w == 1.0f) ? u : gx::log_f(w) * (u / (w - 1.0f));
    return (x > 0.0f ? x : 0.0f) + l1p;
}

// gx_qcritic.h:softplus_grad_f: the derivative of Softplus as torch's backward evaluates it
__device__ __forceinline__ float softplus_grad_f(float x)
{
    if (x > 20.0f) return 1.0f;
    const float e = gx::exp_f(x);
    return __fdiv_rn(e, __fadd_rn(e, 1.0f));
}

// test infrastructure (gxq_softplus_probe): the two functions by themselves, one lane per element
__global__ __launch_bounds__(kThreads) void softplus_kernel(int n, const float* __restrict__ x, float* __restrict__ f, float* __restrict__ df)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) {
        f[i] = softplus_f(x[i]);
        df[i] = softplus_grad_f(x[i]);
    }
}

template <int KS1, bool DOT>
__global__ __launch_bounds__(kThreads) void grad_kernel(GradArgs a)
{
    constexpr int NT1 = nt1_of(KS1), SO = obs_stride(KS1);
    extern __shared__ double lds_d[];
    double* const WS = lds_d;              // [wave][2]
    float* const W2 = reinterpret_cast<float*>(lds_d + kDbl);
    float* const W3 = W2 + kH * kSW;       // one output: [kH]; DOT: [kAp][kSW], the rows past A zero
    float* const b1 = W3 + (DOT ? kAp * kSW : kH);
    float* const b2 = b1 + kH;
    float* const b3 = b2 + kH;             // [kAp], the entries past A zero
    float* const O = b3 + kAp;
    float* const H1 = O + kTile * SO;
    float* const H2 = H1 + kTile * kSW;    // h2, then gz1
    float* const GZ2 = H2 + kTile * kSW;
    float* const R = GZ2 + kTile * kSW;    // 64: the tile of y
    float* const WT = R + kTile;           // 64: the tile of weights, 0 for the rows past B
    float* const OF = WT + kTile;          // 64: the tile of offsets
    float* const U = OF + kTile;           // one output: dz [64];  DOT: Z [64][kSU], then DZ [64][kSU], the columns past A zero
    float* const DZ = U + kTile * kSU;

    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, c = lane & 15, q = lane >> 4;
    const int D = a.D, A = a.A;
    const int P = kH * D + kH + kH * kH + kH + A * kH + A;
    const int oW1 = 0, ob1 = oW1 + kH * D, oW2 = ob1 + kH, ob2 = oW2 + kH * kH, oW3 = ob2 + kH, ob3 = oW3 + A * kH;
    const float* __restrict__ th = a.theta;

    // ---- the LDS image of theta, and this lane's W1 operands
    static_assert(kH * kH % kThreads == 0 && kAp * kH % kThreads == 0, "whole passes");
#pragma unroll
    for (int p = 0; p < kH * kH / kThreads; ++p) {
        const int i = tid + kThreads * p;
        W2[(i >> 6) * kSW + (i & 63)] = th[oW2 + i];
    }
    if constexpr (DOT) {
#pragma unroll
        for (int p = 0; p < kAp * kH / kThreads; ++p) {
            const int i = tid + kThreads * p;
            W3[(i >> 6) * kSW + (i & 63)] = (i >> 6) < A ? th[oW3 + i] : 0.0f;
        }
        for (int i = tid; i < kTile * kSU; i += kThreads) DZ[i] = 0.0f;    // the columns past A stay zero
    } else {
        if (tid < kH) W3[tid] = th[oW3 + tid];
    }
    if (tid < kH) {
        b1[tid] = th[ob1 + tid];
        b2[tid] = th[ob2 + tid];
    }
    if (tid < kAp) b3[tid] = tid < A ? th[ob3 + tid] : 0.0f;
    for (int i = tid; i < kTile * SO; i += kThreads) O[i] = 0.0f;          // the columns past D stay zero
    float w1[KS1];
#pragma unroll
    for (int s = 0; s < KS1; ++s) {
        const int k = 4 * s + q;
        w1[s] = k < D ? th[oW1 + (16 * w + c) * D + k] : 0.0f;
    }
    // element tid + 256 j of a tile (its rows are contiguous in x) sits in row (tid + 256 j) / D, column (tid + 256 j) % D of O:
    // walked from j = 0 by steps of 256 = dr D + dc at every tile (gx_pgrad.hip)
    const int row0 = tid / D, col0 = tid % D, dr = kThreads / D, dc = kThreads % D;
    float pf[KS1], pr = 0.0f, pw = 0.0f, po = 0.0f;
    auto load_tile = [&](int t) {
        const float* __restrict__ src = a.x + (size_t)t * kTile * D;
        const int rows = a.B - t * kTile < kTile ? a.B - t * kTile : kTile;
        const int n = rows * D;                                 // nothing past row B - 1 is read
#pragma unroll
        for (int j = 0; j < KS1; ++j) pf[j] = tid + kThreads * j < n ? src[tid + kThreads * j] : 0.0f;
        pr = pw = po = 0.0f;
        if (tid < rows) {
            const size_t i = (size_t)t * kTile + tid;
            pr = a.y[i];
            pw = a.w ? a.w[i] : 1.0f;
            if (DOT && a.off) po = a.off[i];
        }
    };

    // the workgroup's running sums: W1 (NT1 column tiles), W2 (4), W3 (one output: row 0 of this wave's tile), the three biases
    mfma_f4 rW1[NT1], rW2[4], rW3 = splat(0.0f), rb1 = splat(0.0f), rb2 = splat(0.0f), rb3 = splat(0.0f);
#pragma unroll
    for (int n = 0; n < NT1; ++n) rW1[n] = splat(0.0f);
#pragma unroll
    for (int n = 0; n < 4; ++n) rW2[n] = splat(0.0f);
    double run_sq = 0.0, run_w = 0.0;                           // this lane's sums of w e^2 and of w over the rows it owns
    const int row = tid >> 2, part = tid & 3;                   // DOT, stage R: row 16 w + (lane >> 2), the actions part, part + 4, ...

    int t = blockIdx.x;
    if (t < a.tiles) load_tile(t);
    wg_sync_lds();                                              // O and DZ are zero before the first rows land in them
    while (t < a.tiles) {
        // ---- 0
        if (tid < kTile) {
            R[tid] = pr;
            WT[tid] = pw;
            OF[tid] = po;
        }
        wg_sync_lds();
        {
            int rr = row0, cc = col0;
#pragma unroll
            for (int j = 0; j < KS1; ++j) {
                if (rr < kTile) O[rr * SO + cc] = WT[rr] != 0.0f ? pf[j] : 0.0f;   // selection: a dead row's x is never a factor
                cc += dc;
                rr += dr;
                if (cc >= D) {
                    cc -= D;
                    ++rr;
                }
            }
        }
        const int tn = t + gridDim.x;
        if (tn < a.tiles) load_tile(tn);                        // in flight during the stages
        float r_act[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (DOT) {                                    // this lane's share of its row of act, in flight too
            const int64_t grow = (int64_t)t * kTile + row;
            if (grow < a.B) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int ac = part + 4 * k;
                    if (ac < A) r_act[k] = a.act[grow * A + ac];
                }
            }
        }
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
                    acc[rb][s % kAcc] = GXQ_MFMA(O[(16 * rb + c) * SO + 4 * s + q], w1[s], acc[rb][s % kAcc]);
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
                    acc[rb][s % kAcc] = GXQ_MFMA(H1[(16 * rb + c) * kSW + 4 * s + q], bw, acc[rb][s % kAcc]);
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
        if constexpr (!DOT) {
            // ---- 3 and R: this wave's 16 rows; column 0 of the product is z, and the lanes c == 0 own the rows 16 w + 4 q ..
            {
                mfma_f4 acc[kAcc];
#pragma unroll
                for (int i = 0; i < kAcc; ++i) acc[i] = splat(i == 0 ? b3[0] : 0.0f);
#pragma unroll
                for (int s = 0; s < kH / 4; ++s) {
                    const float bw = c == 0 ? W3[4 * s + q] : 0.0f;
                    acc[s % kAcc] = GXQ_MFMA(H2[(16 * w + c) * kSW + 4 * s + q], bw, acc[s % kAcc]);
                }
                const mfma_f4 val = sum_acc(acc);
                if (c == 0) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int rw = 16 * w + 4 * q + r;
                        const float wt = WT[rw];
                        const bool live = wt != 0.0f;           // selection, never a product with zero
                        const float z = val[r];
                        const float f = a.softplus ? softplus_f(z) : z;
                        const float fp = a.softplus ? softplus_grad_f(z) : 1.0f;
                        const float e = f - R[rw];
                        U[rw] = live ? (float)(((2.0 * (double)wt) * (double)e) * (double)fp) : 0.0f;
                        run_sq += live ? (double)wt * ((double)e * (double)e) : 0.0;
                        run_w += live ? (double)wt : 0.0;
                    }
                }
            }
            wg_sync_lds();
            // ---- 4
            {
                const float w3 = W3[16 * w + c];
#pragma unroll
                for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int rw = 16 * rb + 4 * q + r;
                        GZ2[rw * kSW + 16 * w + c] = (U[rw] * w3) * d2[rb][r];
                    }
                mfma_f4 t3 = splat(0.0f), tb = splat(0.0f);
#pragma unroll
                for (int s = 0; s < kTile / 4; ++s) {
                    const float av = c == 0 ? U[4 * s + q] : 0.0f;  // row 0 of the A operand: the one output
                    t3 = GXQ_MFMA(av, H2[(4 * s + q) * kSW + 16 * w + c], t3);
                    tb = GXQ_MFMA(av, 1.0f, tb);
                }
                rW3 += t3;
                rb3 += tb;
            }
        } else {
            float* const Z = U;
            // ---- 3: this wave's 16 rows
            {
                mfma_f4 acc[kAcc];
#pragma unroll
                for (int i = 0; i < kAcc; ++i) acc[i] = splat(i == 0 ? b3[c] : 0.0f);
#pragma unroll
                for (int s = 0; s < kH / 4; ++s)
                    acc[s % kAcc] = GXQ_MFMA(H2[(16 * w + c) * kSW + 4 * s + q], W3[c * kSW + 4 * s + q], acc[s % kAcc]);
                const mfma_f4 m = sum_acc(acc);
#pragma unroll
                for (int r = 0; r < 4; ++r) Z[(16 * w + 4 * q + r) * kSU + c] = m[r];
            }
            wg_sync_lds();
            // ---- R: the rows
            {
                const float wt = WT[row];
                const bool live = wt != 0.0f;                   // selection, never a product with zero
                double fs = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int ac = part + 4 * k;
                    if (ac < A) fs += (double)Z[row * kSU + ac] * (double)r_act[k];
                }
                fs += __shfl_xor(fs, 1);
                fs += __shfl_xor(fs, 2);
                const float f = (float)(fs + (double)OF[row]);
                const float e = f - R[row];
                const double cd = (2.0 * (double)wt) * (double)e;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int ac = part + 4 * k;
                    if (ac < A) DZ[row * kSU + ac] = live ? (float)(cd * (double)r_act[k]) : 0.0f;
                }
                const bool on = live && part == 0;
                run_sq += on ? (double)wt * ((double)e * (double)e) : 0.0;
                run_w += on ? (double)wt : 0.0;
            }
            wg_sync_lds();
            // ---- 4
            {
                mfma_f4 z[4];
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) z[rb] = splat(0.0f);
#pragma unroll
                for (int s = 0; s < kAp / 4; ++s) {
                    const float bv = W3[(4 * s + q) * kSW + 16 * w + c];
#pragma unroll
                    for (int rb = 0; rb < 4; ++rb) z[rb] = GXQ_MFMA(DZ[(16 * rb + c) * kSU + 4 * s + q], bv, z[rb]);
                }
                mfma_f4 t3 = splat(0.0f), tb = splat(0.0f);
#pragma unroll
                for (int s = 0; s < kTile / 4; ++s) {
                    const float av = DZ[(4 * s + q) * kSU + c];
                    t3 = GXQ_MFMA(av, H2[(4 * s + q) * kSW + 16 * w + c], t3);
                    tb = GXQ_MFMA(av, 1.0f, tb);
                }
                rW3 += t3;
                rb3 += tb;
#pragma unroll
                for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) GZ2[(16 * rb + 4 * q + r) * kSW + 16 * w + c] = z[rb][r] * d2[rb][r];
            }
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
                for (int n = 0; n < 4; ++n) t2[n] = GXQ_MFMA(av, H1[(4 * s + q) * kSW + 16 * n + c], t2[n]);
                tb = GXQ_MFMA(av, 1.0f, tb);
                const float bv = W2[(4 * s + q) * kSW + 16 * w + c];
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) z[rb] = GXQ_MFMA(GZ2[(16 * rb + c) * kSW + 4 * s + q], bv, z[rb]);
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
                for (int n = 0; n < NT1; ++n) t1[n] = GXQ_MFMA(av, O[(4 * s + q) * SO + 16 * n + c], t1[n]);
                tb = GXQ_MFMA(av, 1.0f, tb);
            }
#pragma unroll
            for (int n = 0; n < NT1; ++n) rW1[n] += t1[n];
            rb1 += tb;
        }
        wg_sync_lds();                                          // O, R, WT, OF and gz1 are free for the next tile
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
        if constexpr (DOT) {
            const int act = 4 * q + r;
            if (act < A) {
                out[oW3 + act * kH + 16 * w + c] = rW3[r];
                if (w == 0 && c == 0) out[ob3 + act] = rb3[r];
            }
        }
    }
    if constexpr (!DOT) {
        if (q == 0) {
            out[oW3 + 16 * w + c] = rW3[0];
            if (w == 0 && c == 0) out[ob3] = rb3[0];
        }
    }
    // ---- the float64 sums: a wave's lanes as a tree, then the waves in wave order
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        run_sq += __shfl_xor(run_sq, m);
        run_w += __shfl_xor(run_w, m);
    }
    if (lane == 0) {
        WS[2 * w] = run_sq;
        WS[2 * w + 1] = run_w;
    }
    wg_sync_lds();
    if (tid < 2) a.sums[(size_t)blockIdx.x * 2 + tid] = ((WS[tid] + WS[2 + tid]) + WS[4 + tid]) + WS[6 + tid];
}

struct StepArgs {
    int P, grid, adam;
    const float* partial;   // [grid][P]
    const double* sums;     // [grid][2]
    float *g_out, *loss_out;                                    // either may be null
    double* w_out;                                              // may be null
    float *theta, *m, *v;                                       // adam != 0
    double b1, b2, omb1, omb2, eps, step_size, bc2_sqrt;        // 1 - b1, 1 - b2, lr / (1 - b1^t), sqrt(1 - b2^t)
};

__global__ __launch_bounds__(kThreads) void step_kernel(StepArgs a)
{
    __shared__ double sh[2][kThreads];
    __shared__ double tot[2];
    const int tid = threadIdx.x, i = blockIdx.x * kThreads + tid;
    // the workgroups' sums of w e^2 and of w in workgroup order, 256 at a time through LDS: one load per lane, all in flight
    // together; lane 0 adds w e^2 (workgroup 0 alone needs it), lane 1 adds w
    const bool first = blockIdx.x == 0;                         // uniform over the workgroup
    double s = 0.0;
    for (int base = 0; base < a.grid; base += kThreads) {
        const int n = a.grid - base < kThreads ? a.grid - base : kThreads;
        if (tid < n) {
            if (first) sh[0][tid] = a.sums[2 * (size_t)(base + tid)];
            sh[1][tid] = a.sums[2 * (size_t)(base + tid) + 1];
        }
        __syncthreads();
        if (tid == 1 || (tid == 0 && first)) {
#pragma unroll 16
            for (int g = 0; g < n; ++g) s += sh[tid][g];
        }
        __syncthreads();
    }
    if (tid < 2) tot[tid] = s;
    __syncthreads();
    const double W = tot[1];
    if (i < a.P) {
        double gs = 0.0;
#pragma unroll 8
        for (int g = 0; g < a.grid; ++g) gs += (double)a.partial[(size_t)g * a.P + i];
        const float gi = (float)(gs / W);                       // W == 0: 0 / 0, the mean of an empty selection
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
    if (first && tid == 0) {
        if (a.loss_out) a.loss_out[0] = (float)(tot[0] / W);
        if (a.w_out) a.w_out[0] = W;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
gxq_status check_shape(const char* who, int B, int D, int A, int hidden, int head, int workgroups)
{
    if (B < 1 || D < 1 || A < 1) return fail(GXQ_ERR_ARG, std::string(who) + ": B, Din and A must be at least 1");
    if (workgroups < 0 || workgroups > kMaxWg)
        return fail(GXQ_ERR_ARG, std::string(who) + ": workgroups must be 0 (the default) .. " + std::to_string(kMaxWg));
    if (head != GXQ_HEAD_IDENTITY && head != GXQ_HEAD_SOFTPLUS && head != GXQ_HEAD_DOT)
        return fail(GXQ_ERR_ARG, std::string(who) + ": unknown head " + std::to_string(head));
    if (hidden != kH) return fail(GXQ_ERR_UNSUPPORTED, std::string(who) + " supports hidden width 64, not " + std::to_string(hidden));
    if (D > kMaxD) return fail(GXQ_ERR_UNSUPPORTED, std::string(who) + " supports an input width <= 128, not " + std::to_string(D));
    if (head == GXQ_HEAD_DOT) {
        if (A % 2 || A > kAp) return fail(GXQ_ERR_UNSUPPORTED, std::string(who) + " supports an even action width <= 16, not " + std::to_string(A));
    } else if (A != 1) {
        return fail(GXQ_ERR_UNSUPPORTED, std::string(who) + " supports one output under this head, not " + std::to_string(A));
    }
    return GXQ_OK;
}

int64_t partial_bytes(int64_t P, int grid) { return (4 * (int64_t)grid * P + 7) / 8 * 8; }
int64_t work_bytes(int64_t P, int grid) { return partial_bytes(P, grid) + 16 * (int64_t)grid; }

template <int KS1, bool DOT>
gxq_status launch_grad(const GradArgs& a, int grid, hipStream_t s)
{
    constexpr int lds = lds_floats(KS1, DOT) * (int)sizeof(float);
    static_assert(lds <= 160 * 1024, "the LDS image fits one CU");
    static_assert(obs_stride(KS1) >= 4 * KS1 && obs_stride(KS1) >= 16 * nt1_of(KS1), "a row of the x tile holds what stages 1 and 6 read");
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&grad_kernel<KS1, DOT>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (attr != hipSuccess) return fail(GXQ_ERR_HIP, std::string("gxq: hipFuncSetAttribute failed: ") + hipGetErrorString(attr));
    hipLaunchKernelGGL((grad_kernel<KS1, DOT>), dim3(grid), dim3(kThreads), lds, s, a);
    return GXQ_OK;
}

template <bool DOT>
gxq_status gradient_of(const GradArgs& a, int grid, hipStream_t s)
{
    const int ks = (a.D + 3) / 4;   // k-steps of the first layer: the instantiations of gx_fisher.hip
    if (ks <= 4) return launch_grad<4, DOT>(a, grid, s);
    if (ks <= 8) return launch_grad<8, DOT>(a, grid, s);
    if (ks <= 11) return launch_grad<11, DOT>(a, grid, s);
    if (ks <= 12) return launch_grad<12, DOT>(a, grid, s);
    if (ks <= 16) return launch_grad<16, DOT>(a, grid, s);
    if (ks <= 18) return launch_grad<18, DOT>(a, grid, s);
    if (ks <= 24) return launch_grad<24, DOT>(a, grid, s);
    return launch_grad<32, DOT>(a, grid, s);
}

gxq_status gradient_at(const GradArgs& a, int head, int grid, hipStream_t s)
{
    return head == GXQ_HEAD_DOT ? gradient_of<true>(a, grid, s) : gradient_of<false>(a, grid, s);
}

GradArgs grad_args(int B, int D, int A, int head, const float* theta, const float* x, const float* y, const float* w,
                   const float* act, const float* off, void* work, int grid)
{
    GradArgs a;
    a.B = B;
    a.D = D;
    a.A = A;
    a.tiles = tiles_of(B);
    a.softplus = head == GXQ_HEAD_SOFTPLUS;
    a.theta = theta;
    a.x = x;
    a.y = y;
    a.w = w;
    a.act = act;
    a.off = off;
    a.partial = static_cast<float*>(work);
    a.sums = reinterpret_cast<double*>(static_cast<char*>(work) + partial_bytes(param_count(D, A, kH), grid));
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

gxq_status launched(const char* who)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GXQ_OK : fail(GXQ_ERR_HIP, std::string(who) + " launch failed: " + hipGetErrorString(e));
}

} // namespace

extern "C" const char* gxq_last_error(void) { return g_err.c_str(); }

extern "C" const char* gxq_build_id(void) { return GXQ_BUILD_ID; } // guardx_amd/build.py:SAFETY_LIBRARIES["cfit"].source_hash()

extern "C" int64_t gxq_param_count(int32_t Din, int32_t A, int32_t hidden)
{
    return (Din < 1 || A < 1 || hidden < 1) ? -1 : param_count(Din, A, hidden);
}

extern "C" int32_t gxq_default_workgroups(int32_t B) { return B < 1 ? 0 : default_workgroups(B); }

extern "C" int64_t gxq_work_bytes(int32_t B, int32_t Din, int32_t A, int32_t head, int32_t workgroups)
{
    if (check_shape("gxq_work_bytes", B, Din, A, kH, head, workgroups) != GXQ_OK) return -1;
    return work_bytes(param_count(Din, A, kH), workgroups ? workgroups : default_workgroups(B));
}

extern "C" gxq_status gxq_softplus_probe(int32_t n, const float* d_x, float* d_f, float* d_df, void* stream)
{
    if (!d_x || !d_f || !d_df) return fail(GXQ_ERR_ARG, "gxq_softplus_probe: null pointer");
    if (n < 0) return fail(GXQ_ERR_ARG, "gxq_softplus_probe: negative n");
    if (n == 0) return GXQ_OK;
    const unsigned blocks = (unsigned)(((int64_t)n + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(softplus_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, n, d_x, d_f, d_df);
    return launched("gxq_softplus_probe");
}

extern "C" gxq_status gxq_gradient(int32_t B, int32_t Din, int32_t A, int32_t hidden, int32_t head, const float* d_theta,
                                   const float* d_x, const float* d_y, const float* d_w, const float* d_act, const float* d_offset,
                                   int32_t workgroups, void* d_work, float* d_g, float* d_loss, void* d_wsum, void* stream)
{
    if (!d_theta || !d_x || !d_y || !d_work || !d_g || !d_loss || !d_wsum) return fail(GXQ_ERR_ARG, "gxq_gradient: null pointer");
    const gxq_status sc = check_shape("gxq_gradient", B, Din, A, hidden, head, workgroups);
    if (sc != GXQ_OK) return sc;
    if (head == GXQ_HEAD_DOT && !d_act) return fail(GXQ_ERR_ARG, "gxq_gradient: null pointer (d_act, which GXQ_HEAD_DOT reads)");
    hipStream_t s = (hipStream_t)stream;
    const int grid = workgroups ? workgroups : default_workgroups(B);
    const GradArgs a = grad_args(B, Din, A, head, d_theta, d_x, d_y, d_w, d_act, d_offset, d_work, grid);
    const gxq_status sg = gradient_at(a, head, grid, s);
    if (sg != GXQ_OK) return sg;
    StepArgs st{};
    st.P = (int)param_count(Din, A, kH);
    st.grid = grid;
    st.partial = a.partial;
    st.sums = a.sums;
    st.g_out = d_g;
    st.loss_out = d_loss;
    st.w_out = static_cast<double*>(d_wsum);
    launch_step(st, s);
    return launched("gxq_gradient");
}

extern "C" gxq_status gxq_fit(int32_t B, int32_t Din, int32_t A, int32_t hidden, int32_t head, float* d_theta, float* d_m, float* d_v,
                              int64_t step0, const float* d_x, const float* d_y, const float* d_w, int64_t w_stride,
                              const float* d_act, const float* d_offset, int32_t iters, void* h_hyper, int32_t workgroups,
                              void* d_work, float* d_loss, void* d_wsum, void* stream)
{
    if (!d_theta || !d_m || !d_v || !d_x || !d_y || !h_hyper || !d_work || !d_loss || !d_wsum) return fail(GXQ_ERR_ARG, "gxq_fit: null pointer");
    if (iters < 0) return fail(GXQ_ERR_ARG, "gxq_fit: negative iters");
    if (step0 < 0) return fail(GXQ_ERR_ARG, "gxq_fit: negative step0");
    const gxq_status sc = check_shape("gxq_fit", B, Din, A, hidden, head, workgroups);
    if (sc != GXQ_OK) return sc;
    if (head == GXQ_HEAD_DOT && !d_act) return fail(GXQ_ERR_ARG, "gxq_fit: null pointer (d_act, which GXQ_HEAD_DOT reads)");
    if (w_stride != 0 && w_stride != B) return fail(GXQ_ERR_ARG, "gxq_fit: w_stride must be 0 or B");
    if (iters == 0) return GXQ_OK;
    hipStream_t s = (hipStream_t)stream;
    const int grid = workgroups ? workgroups : default_workgroups(B);
    const double* h = static_cast<const double*>(h_hyper);
    GradArgs a = grad_args(B, Din, A, head, d_theta, d_x, d_y, d_w, d_act, d_offset, d_work, grid);
    StepArgs st{};
    st.P = (int)param_count(Din, A, kH);
    st.grid = grid;
    st.partial = a.partial;
    st.sums = a.sums;
    st.theta = d_theta;
    st.m = d_m;
    st.v = d_v;
    for (int i = 0; i < iters; ++i) {
        a.w = d_w ? d_w + (size_t)i * (size_t)w_stride : nullptr;
        const gxq_status sg = gradient_at(a, head, grid, s);
        if (sg != GXQ_OK) return sg;
        set_adam(st, h, h + 4 + 2 * (size_t)i);
        st.loss_out = d_loss + i;
        st.w_out = static_cast<double*>(d_wsum) + i;
        launch_step(st, s);
    }
    return launched("gxq_fit");
}
