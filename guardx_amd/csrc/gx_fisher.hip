// gx_fisher.hip -- libguardx_fisher.so (include/guardx_fisher.h): y = H x for the Hessian H of the learners' KL at the
// old policy (a Gauss-Newton form over the Gaussian MLP actor, hidden width 64) and the learners' cg around it, on the
// caller's stream and without a host synchronisation.  The header fixes the arithmetic; this file is its order of work:
//
//   fvp_kernel     a persistent grid of 4-wave workgroups; workgroup g walks the 64-row tiles g, g + grid, ... of obs.
//                  LDS holds W2, W3, the biases and their tangents (the x side), the tile of obs and its activations;
//                  W1 and dW1 are B operands that a lane never shares (wave w owns the hidden units 16 w .. + 15), so
//                  each lane keeps its 2 x KS1 of them in registers.  Per tile six stages, each a set of
//                  v_mfma_f32_16x16x4_f32 chains (four interleaved ones per sum in stages 1 to 3: sum_acc), with a
//                  workgroup barrier (LDS only) between them:
//                    1  z1, t1 = o W1' + b1, o dW1' + db1            -> h1, dh1                      (K = pad4 D)
//                    2  z2, t2 = h1 W2' + b2, h1 dW2' + dh1 W2' + db2 -> h2, dh2                      (K = 64)
//                    3  dmu = h2 dW3' + dh2 W3' + db3 -> u = dmu / ((v + eps) B), 0 for rows past B   (wave w: rows 16 w ..)
//                    4  gz2 = (u W3)(1 - h2^2);  gW3 += u' h2, gb3 += u' 1                            (K = 16; K = 64 rows)
//                    5  gW2 += gz2' h1, gb2 += gz2' 1;  gz1 = (gz2 W2)(1 - h1^2)
//                    6  gW1 += gz1' o, gb1 += gz1' 1
//                  A bias gradient is one more chain on the A operand its weight gradient loads anyway (B = 1).  The
//                  sums over a tile's 64 rows start from zero and are added to the workgroup's running sums after the
//                  stage, so that no float32 chain is longer than a tile, whatever B is.  The next tile's rows are
//                  loaded into registers while this one is computed (the barriers do not wait for global loads).
//                  The workgroup writes its running sums as one partial vector of P floats.  The activations are
//                  tanh_act below, not the rollout's tanh_f: see there.
//   reduce_kernel  y[i] = the partial vectors' entries i added in workgroup order (float64, rounded once), the
//                  log_std block, + damping x.
//   cg_*_kernel    one 1024-lane workgroup over P: the dots (float64, fixed tree), alpha, the three updates, the stop.
// No atomics anywhere: the same arguments give the same bits.
#include "../../include/guardx_fisher.h"
#include "gx_policy.h"
#include <string>

#ifndef GXF_BUILD_ID
#define GXF_BUILD_ID "unknown"
#endif

namespace {

using gx::mfma_f4;
using gx::wg_sync_lds;

thread_local std::string g_err;

gxf_status fail(gxf_status st, const std::string& msg)
{
    g_err = msg;
    return st;
}

constexpr int kH = gx::kPolHd;   // hidden width
constexpr int kTile = 64;        // rows of obs per tile
constexpr int kThreads = 256;    // four waves; wave w owns the hidden units 16 w .. 16 w + 15
constexpr int kAp = 16;          // the action width padded to one MFMA tile
constexpr int kSW = 66;          // LDS row stride of everything 64 wide: 16 rows x 2 k of a ds_read_b32 group hit 32 banks
constexpr int kSU = 18;          // ... of u (64 x 16)
constexpr int kDefaultWg = 256;  // one workgroup per CU of the MI355X: the LDS image leaves room for one
constexpr int kMaxWg = 4096;
constexpr int kMaxD = 128;
constexpr int kCgThreads = 1024;
constexpr int kAcc = 4;          // interleaved chains of a forward product (stages 1 to 3): see sum_acc

// row stride of the obs tile: at least the 16 NT1 columns stage 6 reads, = 2 mod 32
constexpr int nt1_of(int KS1) { return (KS1 + 3) / 4; }
constexpr int obs_stride(int KS1) { return (16 * nt1_of(KS1) - 2 + 31) / 32 * 32 + 2; }
constexpr int lds_floats(int KS1) { return 2 * kH * kSW + 2 * kAp * kSW + 4 * kH + 3 * kAp + kTile * obs_stride(KS1) + 4 * kTile * kSW + kTile * kSU; }

int64_t param_count(int D, int A, int h) { return (int64_t)A + (int64_t)h * D + h + (int64_t)h * h + h + (int64_t)A * h + A; }
int tiles_of(int B) { return (int)(((int64_t)B + kTile - 1) / kTile); }
int default_workgroups(int B) { return tiles_of(B) < kDefaultWg ? tiles_of(B) : kDefaultWg; }

struct FvpArgs {
    int B, D, A, tiles;
    const float *obs, *theta, *x;
    float* partial;    // [grid][P]
    const int* stop;   // the solve's flag, or null: set -> nothing to do
    double eps;
};

#define GXF_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0)

__device__ __forceinline__ mfma_f4 splat(float v) { return mfma_f4{v, v, v, v}; }

// The products over a layer's inputs (z, t and dmu: K = pad4 D, 64 and 128 terms) are taken as kAcc chains, k-step s on chain
// s mod kAcc, the bias on chain 0, added pairwise at the end.  One chain rounds 64 times at the size of its running sum;
// four round 16 times each at half that size, which halves the error of the sum.  It shows where dmu nearly cancels: one
// row, one tangent whose dmu is 1/50 of the sum of its terms' sizes -- 1.6e-6 of the product's norm with one chain, against
// 2e-7 of the learners' double backward (whose BLAS sums in blocks), 3e-7 with four.
__device__ __forceinline__ mfma_f4 sum_acc(const mfma_f4 (&a)[kAcc])
{
    static_assert(kAcc == 4, "pairwise over four");
    return (a[0] + a[1]) + (a[2] + a[3]);
}

// tanh for the activations.  gx::tanh_f is 1 - 2 / (exp(2 |x|) + 1): its ABSOLUTE error is a few 1e-8 everywhere, which is
// what a rollout needs of it, but below |x| ~ 0.6 the subtraction cancels and the relative error grows like 1e-7 / |x|
// (0.7 % at the smallest arguments) -- and here every activation multiplies tangents and gradients, so the product is
// measured by its relative error.  Below 0.625 the odd polynomial x + x^3 P(x^2) of the Cephes single-precision tanh
// (public domain, S. Moshier) takes over: 2.3 ulp at worst over the whole line, against 1e5 ulp.
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

// test infrastructure (gxf_tanh_act): tanh_act by itself, one lane per element
__global__ __launch_bounds__(kThreads) void tanh_act_kernel(int n, const float* __restrict__ x, float* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) out[i] = tanh_act(x[i]);
}

template <int KS1>
__global__ __launch_bounds__(kThreads) void fvp_kernel(FvpArgs a)
{
    constexpr int NT1 = nt1_of(KS1), SO = obs_stride(KS1);
    extern __shared__ float lds[];
    float* const W2 = lds;
    float* const dW2 = W2 + kH * kSW;
    float* const W3 = dW2 + kH * kSW;
    float* const dW3 = W3 + kAp * kSW;
    float* const b1 = dW3 + kAp * kSW;
    float* const db1 = b1 + kH;
    float* const b2 = db1 + kH;
    float* const db2 = b2 + kH;
    float* const b3 = db2 + kH;
    float* const db3 = b3 + kAp;
    float* const inv = db3 + kAp;
    float* const O = inv + kAp;
    float* const H1 = O + kTile * SO;
    float* const H2 = H1 + kTile * kSW;
    float* const DH1 = H2 + kTile * kSW;   // dh1, then gz1
    float* const DH2 = DH1 + kTile * kSW;  // dh2, then gz2
    float* const U = DH2 + kTile * kSW;

    if (a.stop && *a.stop) return;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, c = lane & 15, q = lane >> 4;
    const int D = a.D, A = a.A;
    const int P = A + kH * D + kH + kH * kH + kH + A * kH + A;
    const int oW1 = A, ob1 = oW1 + kH * D, oW2 = ob1 + kH, ob2 = oW2 + kH * kH, oW3 = ob2 + kH, ob3 = oW3 + A * kH;
    const float* __restrict__ th = a.theta;
    const float* __restrict__ x = a.x;

    // ---- the LDS image of theta and x, and this lane's W1 / dW1 operands
    for (int i = tid; i < kH * kH; i += kThreads) {
        W2[(i >> 6) * kSW + (i & 63)] = th[oW2 + i];
        dW2[(i >> 6) * kSW + (i & 63)] = x[oW2 + i];
    }
    for (int i = tid; i < kAp * kH; i += kThreads) {
        const bool in = (i >> 6) < A;
        W3[(i >> 6) * kSW + (i & 63)] = in ? th[oW3 + i] : 0.0f;
        dW3[(i >> 6) * kSW + (i & 63)] = in ? x[oW3 + i] : 0.0f;
    }
    if (tid < kH) {
        b1[tid] = th[ob1 + tid];
        db1[tid] = x[ob1 + tid];
        b2[tid] = th[ob2 + tid];
        db2[tid] = x[ob2 + tid];
    }
    if (tid < kAp) {
        const bool in = tid < A;
        b3[tid] = in ? th[ob3 + tid] : 0.0f;
        db3[tid] = in ? x[ob3 + tid] : 0.0f;
        inv[tid] = in ? (float)(1.0 / ((exp(2.0 * (double)th[tid]) + a.eps) * (double)a.B)) : 0.0f;
    }
    for (int i = tid; i < kTile * SO; i += kThreads) O[i] = 0.0f;   // the columns past D stay zero
    float w1[KS1], dw1[KS1];
#pragma unroll
    for (int s = 0; s < KS1; ++s) {
        const int k = 4 * s + q;
        w1[s] = k < D ? th[oW1 + (16 * w + c) * D + k] : 0.0f;
        dw1[s] = k < D ? x[oW1 + (16 * w + c) * D + k] : 0.0f;
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

    // the workgroup's running sums: W1 (NT1 column tiles), W2 (4), W3 (this wave's tile), the three biases
    mfma_f4 rW1[NT1], rW2[4], rW3 = splat(0.0f), rb1 = splat(0.0f), rb2 = splat(0.0f), rb3 = splat(0.0f);
#pragma unroll
    for (int n = 0; n < NT1; ++n) rW1[n] = splat(0.0f);
#pragma unroll
    for (int n = 0; n < 4; ++n) rW2[n] = splat(0.0f);

    int t = blockIdx.x;
    if (t < a.tiles) load_tile(t);
    wg_sync_lds();                                              // O is zero before the first rows land in it
    while (t < a.tiles) {
#pragma unroll
        for (int j = 0; j < KS1; ++j)
            if (off[j] >= 0) O[off[j]] = pf[j];
        const int tn = t + gridDim.x;
        if (tn < a.tiles) load_tile(tn);                        // in flight during the six stages
        wg_sync_lds();

        mfma_f4 z[4], tt[4];
        float d1[4][4], d2[4][4];                               // 1 - h1^2, 1 - h2^2 of this lane's outputs
        // ---- 1
        {
            const float bz = b1[16 * w + c], bt = db1[16 * w + c];
            // z, then its tangent: the 4 x kAcc accumulators of one of them at a time (the rows are read from LDS twice)
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {
                mfma_f4 acc[4][kAcc];
#pragma unroll
                for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                    for (int i = 0; i < kAcc; ++i) acc[rb][i] = splat(i != 0 ? 0.0f : pass == 0 ? bz : bt);
#pragma unroll
                for (int s = 0; s < KS1; ++s) {
#pragma unroll
                    for (int rb = 0; rb < 4; ++rb)
                        acc[rb][s % kAcc] = GXF_MFMA(O[(16 * rb + c) * SO + 4 * s + q], pass == 0 ? w1[s] : dw1[s], acc[rb][s % kAcc]);
                }
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) (pass == 0 ? z[rb] : tt[rb]) = sum_acc(acc[rb]);
            }
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float h = tanh_act(z[rb][r]);
                    d1[rb][r] = fmaf(-h, h, 1.0f);
                    H1[(16 * rb + 4 * q + r) * kSW + 16 * w + c] = h;
                    DH1[(16 * rb + 4 * q + r) * kSW + 16 * w + c] = d1[rb][r] * tt[rb][r];
                }
        }
        wg_sync_lds();
        // ---- 2
        {
            const float bz = b2[16 * w + c], bt = db2[16 * w + c];
            {                                                   // z
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
                        acc[rb][s % kAcc] = GXF_MFMA(H1[(16 * rb + c) * kSW + 4 * s + q], bw, acc[rb][s % kAcc]);
                }
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) z[rb] = sum_acc(acc[rb]);
            }
            {                                                   // its tangent: per k-step h1 dW2', then dh1 W2'
                mfma_f4 acc[4][kAcc];
#pragma unroll
                for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                    for (int i = 0; i < kAcc; ++i) acc[rb][i] = splat(i == 0 ? bt : 0.0f);
#pragma unroll
                for (int s = 0; s < kH / 4; ++s) {
                    const float bw = W2[(16 * w + c) * kSW + 4 * s + q], bd = dW2[(16 * w + c) * kSW + 4 * s + q];
#pragma unroll
                    for (int rb = 0; rb < 4; ++rb)
                        acc[rb][s % kAcc] = GXF_MFMA(H1[(16 * rb + c) * kSW + 4 * s + q], bd, acc[rb][s % kAcc]);
#pragma unroll
                    for (int rb = 0; rb < 4; ++rb)
                        acc[rb][s % kAcc] = GXF_MFMA(DH1[(16 * rb + c) * kSW + 4 * s + q], bw, acc[rb][s % kAcc]);
                }
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) tt[rb] = sum_acc(acc[rb]);
            }
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float h = tanh_act(z[rb][r]);
                    d2[rb][r] = fmaf(-h, h, 1.0f);
                    H2[(16 * rb + 4 * q + r) * kSW + 16 * w + c] = h;
                    DH2[(16 * rb + 4 * q + r) * kSW + 16 * w + c] = d2[rb][r] * tt[rb][r];
                }
        }
        wg_sync_lds();
        // ---- 3: this wave's 16 rows
        {
            mfma_f4 m0a[kAcc], m1a[kAcc];
#pragma unroll
            for (int i = 0; i < kAcc; ++i) { m0a[i] = splat(i == 0 ? db3[c] : 0.0f); m1a[i] = splat(0.0f); }
#pragma unroll
            for (int s = 0; s < kH / 4; ++s) {
                m0a[s % kAcc] = GXF_MFMA(H2[(16 * w + c) * kSW + 4 * s + q], dW3[c * kSW + 4 * s + q], m0a[s % kAcc]);
                m1a[s % kAcc] = GXF_MFMA(DH2[(16 * w + c) * kSW + 4 * s + q], W3[c * kSW + 4 * s + q], m1a[s % kAcc]);
            }
            const mfma_f4 m0 = sum_acc(m0a), m1 = sum_acc(m1a);
            const float iv = inv[c];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * w + 4 * q + r;
                const float u = (m0[r] + m1[r]) * iv;
                U[row * kSU + c] = (int64_t)t * kTile + row < a.B ? u : 0.0f;
            }
        }
        wg_sync_lds();
        // ---- 4
        {
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) z[rb] = splat(0.0f);
#pragma unroll
            for (int s = 0; s < kAp / 4; ++s) {
                const float bv = W3[(4 * s + q) * kSW + 16 * w + c];
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) z[rb] = GXF_MFMA(U[(16 * rb + c) * kSU + 4 * s + q], bv, z[rb]);
            }
            mfma_f4 t3 = splat(0.0f), tb = splat(0.0f);
#pragma unroll
            for (int s = 0; s < kTile / 4; ++s) {
                const float av = U[(4 * s + q) * kSU + c];
                t3 = GXF_MFMA(av, H2[(4 * s + q) * kSW + 16 * w + c], t3);
                tb = GXF_MFMA(av, 1.0f, tb);
            }
            rW3 += t3;
            rb3 += tb;
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int r = 0; r < 4; ++r) DH2[(16 * rb + 4 * q + r) * kSW + 16 * w + c] = z[rb][r] * d2[rb][r];
        }
        wg_sync_lds();
        // ---- 5
        {
            mfma_f4 t2[4], tb = splat(0.0f);
#pragma unroll
            for (int n = 0; n < 4; ++n) t2[n] = splat(0.0f);
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) z[rb] = splat(0.0f);
#pragma unroll
            for (int s = 0; s < kTile / 4; ++s) {
                const float av = DH2[(4 * s + q) * kSW + 16 * w + c];
#pragma unroll
                for (int n = 0; n < 4; ++n) t2[n] = GXF_MFMA(av, H1[(4 * s + q) * kSW + 16 * n + c], t2[n]);
                tb = GXF_MFMA(av, 1.0f, tb);
                const float bv = W2[(4 * s + q) * kSW + 16 * w + c];
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) z[rb] = GXF_MFMA(DH2[(16 * rb + c) * kSW + 4 * s + q], bv, z[rb]);
            }
#pragma unroll
            for (int n = 0; n < 4; ++n) rW2[n] += t2[n];
            rb2 += tb;
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int r = 0; r < 4; ++r) DH1[(16 * rb + 4 * q + r) * kSW + 16 * w + c] = z[rb][r] * d1[rb][r];
        }
        wg_sync_lds();
        // ---- 6
        {
            mfma_f4 t1[NT1], tb = splat(0.0f);
#pragma unroll
            for (int n = 0; n < NT1; ++n) t1[n] = splat(0.0f);
#pragma unroll
            for (int s = 0; s < kTile / 4; ++s) {
                const float av = DH1[(4 * s + q) * kSW + 16 * w + c];
#pragma unroll
                for (int n = 0; n < NT1; ++n) t1[n] = GXF_MFMA(av, O[(4 * s + q) * SO + 16 * n + c], t1[n]);
                tb = GXF_MFMA(av, 1.0f, tb);
            }
#pragma unroll
            for (int n = 0; n < NT1; ++n) rW1[n] += t1[n];
            rb1 += tb;
        }
        wg_sync_lds();                                          // O and gz1 are free for the next tile
        t = tn;
    }

    // ---- the partial vector: an accumulator's entry r is row 4 q + r, column c of its 16 x 16 tile
    float* __restrict__ out = a.partial + (size_t)blockIdx.x * P;
    if (tid < A) out[tid] = 0.0f;                               // log_std: reduce_kernel's
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
        const int act = 4 * q + r;
        if (act < A) {
            out[oW3 + act * kH + 16 * w + c] = rW3[r];
            if (w == 0 && c == 0) out[ob3 + act] = rb3[r];
        }
    }
}

__global__ __launch_bounds__(kThreads) void reduce_kernel(int P, int A, int grid, const float* __restrict__ partial,
                                                          const float* __restrict__ theta, const float* __restrict__ x,
                                                          double eps, float damping, float* __restrict__ y,
                                                          const int* __restrict__ stop)
{
    if (stop && *stop) return;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= P) return;
    double s = 0.0;
    for (int g = 0; g < grid; ++g) s += (double)partial[(size_t)g * P + i];
    if (i < A) {
        const double v = exp(2.0 * (double)theta[i]), ve = v + eps;
        s = 0.5 * v * (-4.0 * v / (ve * ve) + 8.0 * v * v / (ve * ve * ve)) * (double)x[i];
    }
    float yi = (float)s;
    if (damping != 0.0f) {
        const float dx = damping * x[i];
        yi = yi + dx;
    }
    y[i] = yi;
}

// ---------------------------------------------------------------------------------------------------------------------
// cg: one workgroup over P
// ---------------------------------------------------------------------------------------------------------------------
struct CgState {
    double rr;
    int32_t stop, iters;
};

// sum of every lane's v, on every lane: a fixed tree (strides 512 .. 1)
__device__ __forceinline__ double block_sum(double* sh, double v)
{
    const int s = threadIdx.x;
    __syncthreads();
    sh[s] = v;
    __syncthreads();
    for (int stride = kCgThreads / 2; stride >= 1; stride >>= 1) {
        if (s < stride) sh[s] = sh[s] + sh[s + stride];
        __syncthreads();
    }
    return sh[0];
}

__global__ __launch_bounds__(kCgThreads) void cg_init_kernel(int P, const float* __restrict__ g, float* __restrict__ x,
                                                            float* __restrict__ r, float* __restrict__ p, CgState* st)
{
    __shared__ double sh[kCgThreads];
    double acc = 0.0;
    for (int i = threadIdx.x; i < P; i += kCgThreads) {
        const float gi = g[i];
        x[i] = 0.0f;
        r[i] = gi;
        p[i] = gi;
        acc += (double)gi * (double)gi;
    }
    const double rr = block_sum(sh, acc);
    if (threadIdx.x == 0) {
        st->rr = rr;
        st->stop = !(rr != 0.0 && rr == rr && rr - rr == 0.0);  // zero or not finite: nothing to iterate on
        st->iters = 0;
    }
}

__global__ __launch_bounds__(kCgThreads) void cg_step_kernel(int P, const float* __restrict__ z, float* __restrict__ x,
                                                            float* __restrict__ r, float* __restrict__ p, CgState* st, double eps)
{
    __shared__ double sh[kCgThreads];
    if (st->stop) return;                                       // uniform: every lane reads the same word
    const double rr = st->rr;
    double acc = 0.0;
    for (int i = threadIdx.x; i < P; i += kCgThreads) acc += (double)p[i] * (double)z[i];
    const double alpha = rr / (block_sum(sh, acc) + eps);
    acc = 0.0;
    for (int i = threadIdx.x; i < P; i += kCgThreads) {
        x[i] = (float)((double)x[i] + alpha * (double)p[i]);
        const float ri = (float)((double)r[i] - alpha * (double)z[i]);
        r[i] = ri;
        acc += (double)ri * (double)ri;
    }
    const double rr_new = block_sum(sh, acc);
    const double beta = rr_new / rr;
    acc = 0.0;
    for (int i = threadIdx.x; i < P; i += kCgThreads) {
        const float pi = (float)((double)r[i] + beta * (double)p[i]);
        p[i] = pi;
        acc += (double)pi * (double)pi;
    }
    const double pp = block_sum(sh, acc);
    if (threadIdx.x == 0) {
        st->rr = rr_new;
        st->iters += 1;
        st->stop = !(sqrt(pp) >= eps) || rr_new == 0.0;         // the learners' early stop; a NaN stops too
    }
}

__global__ __launch_bounds__(kCgThreads) void cg_finish_kernel(int P, const float* __restrict__ x, const float* __restrict__ z,
                                                              const CgState* st, float* __restrict__ s_out,
                                                              float* __restrict__ rdot_out, int32_t* __restrict__ iters_out)
{
    __shared__ double sh[kCgThreads];
    double acc = 0.0;
    for (int i = threadIdx.x; i < P; i += kCgThreads) acc += (double)x[i] * (double)z[i];
    const double s = block_sum(sh, acc);
    if (threadIdx.x == 0) {
        *s_out = (float)s;
        *rdot_out = (float)st->rr;
        *iters_out = st->iters;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
gxf_status check_shape(const char* who, int B, int D, int A, int hidden, int workgroups)
{
    if (B < 1 || D < 1 || A < 1) return fail(GXF_ERR_ARG, std::string(who) + ": B, D and A must be at least 1");
    if (workgroups < 0 || workgroups > kMaxWg)
        return fail(GXF_ERR_ARG, std::string(who) + ": workgroups must be 0 (the default) .. " + std::to_string(kMaxWg));
    if (hidden != kH) return fail(GXF_ERR_UNSUPPORTED, std::string(who) + " supports hidden width 64, not " + std::to_string(hidden));
    if (D > kMaxD) return fail(GXF_ERR_UNSUPPORTED, std::string(who) + " supports an observation width <= 128, not " + std::to_string(D));
    if (A % 2 != 0 || A > kAp)
        return fail(GXF_ERR_UNSUPPORTED, std::string(who) + " supports an even action width <= 16, not " + std::to_string(A));
    return GXF_OK;
}

struct Work {
    float *partial, *z, *r, *p;
    CgState* st;
};

int64_t work_bytes(int64_t P, int grid) { return (4 * ((int64_t)grid * P + 3 * P) + 7) / 8 * 8 + (int64_t)sizeof(CgState); }

Work carve(void* base, int64_t P, int grid)
{
    Work w;
    w.partial = static_cast<float*>(base);
    w.z = w.partial + (int64_t)grid * P;
    w.r = w.z + P;
    w.p = w.r + P;
    w.st = reinterpret_cast<CgState*>(static_cast<char*>(base) + (4 * ((int64_t)grid * P + 3 * P) + 7) / 8 * 8);
    return w;
}

template <int KS1>
gxf_status launch_fvp(const FvpArgs& a, int grid, hipStream_t s)
{
    constexpr int lds = lds_floats(KS1) * (int)sizeof(float);
    static_assert(lds <= 160 * 1024, "the LDS image fits one CU");
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&fvp_kernel<KS1>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (attr != hipSuccess) return fail(GXF_ERR_HIP, std::string("gxf_fvp: hipFuncSetAttribute failed: ") + hipGetErrorString(attr));
    hipLaunchKernelGGL(fvp_kernel<KS1>, dim3(grid), dim3(kThreads), lds, s, a);
    return GXF_OK;
}

// y = H x + damping x through w.partial; `stop`: the solve's flag
gxf_status product(int B, int D, int A, const float* obs, const float* theta, const float* x, double eps, float damping,
                   int grid, const Work& w, float* y, const int* stop, hipStream_t s)
{
    FvpArgs a;
    a.B = B;
    a.D = D;
    a.A = A;
    a.tiles = tiles_of(B);
    a.obs = obs;
    a.theta = theta;
    a.x = x;
    a.partial = w.partial;
    a.stop = stop;
    a.eps = eps;
    const int ks = (D + 3) / 4;   // k-steps of the first layer: the default tasks' widths (43 / 44, 46, 64, 70) exactly, the rest rounded up
    gxf_status st;
    if (ks <= 4) st = launch_fvp<4>(a, grid, s);
    else if (ks <= 8) st = launch_fvp<8>(a, grid, s);
    else if (ks <= 11) st = launch_fvp<11>(a, grid, s);
    else if (ks <= 12) st = launch_fvp<12>(a, grid, s);
    else if (ks <= 16) st = launch_fvp<16>(a, grid, s);
    else if (ks <= 18) st = launch_fvp<18>(a, grid, s);
    else if (ks <= 24) st = launch_fvp<24>(a, grid, s);
    else st = launch_fvp<32>(a, grid, s);
    if (st != GXF_OK) return st;
    const int P = (int)param_count(D, A, kH);
    hipLaunchKernelGGL(reduce_kernel, dim3((P + kThreads - 1) / kThreads), dim3(kThreads), 0, s, P, A, grid, w.partial, theta, x,
                       eps, damping, y, stop);
    return GXF_OK;
}

gxf_status launched(const char* who)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GXF_OK : fail(GXF_ERR_HIP, std::string(who) + " launch failed: " + hipGetErrorString(e));
}

} // namespace

extern "C" const char* gxf_last_error(void) { return g_err.c_str(); }

extern "C" const char* gxf_build_id(void) { return GXF_BUILD_ID; } // guardx_amd/build.py:LEARNER_LIBRARIES["fisher"].source_hash()

extern "C" int64_t gxf_param_count(int32_t D, int32_t A, int32_t hidden)
{
    return (D < 1 || A < 1 || hidden < 1) ? -1 : param_count(D, A, hidden);
}

extern "C" int32_t gxf_default_workgroups(int32_t B) { return B < 1 ? 0 : default_workgroups(B); }

extern "C" int64_t gxf_work_bytes(int32_t B, int32_t D, int32_t A, int32_t workgroups)
{
    if (check_shape("gxf_work_bytes", B, D, A, kH, workgroups) != GXF_OK) return -1;
    return work_bytes(param_count(D, A, kH), workgroups ? workgroups : default_workgroups(B));
}

extern "C" gxf_status gxf_tanh_act(int32_t n, const float* d_x, float* d_out, void* stream)
{
    if (!d_x || !d_out) return fail(GXF_ERR_ARG, "gxf_tanh_act: null pointer");
    if (n < 0) return fail(GXF_ERR_ARG, "gxf_tanh_act: negative n");
    if (n == 0) return GXF_OK;
    const unsigned blocks = (unsigned)(((int64_t)n + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(tanh_act_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, n, d_x, d_out);
    return launched("gxf_tanh_act");
}

extern "C" gxf_status gxf_fvp(int32_t B, int32_t D, int32_t A, int32_t hidden, const float* d_obs, const float* d_theta,
                              const float* d_x, float eps, float damping, int32_t workgroups, void* d_work, float* d_y,
                              void* stream)
{
    if (!d_obs || !d_theta || !d_x || !d_work || !d_y) return fail(GXF_ERR_ARG, "gxf_fvp: null pointer");
    if (d_y == d_x) return fail(GXF_ERR_ARG, "gxf_fvp: d_y may not alias d_x");
    const gxf_status st = check_shape("gxf_fvp", B, D, A, hidden, workgroups);
    if (st != GXF_OK) return st;
    const int grid = workgroups ? workgroups : default_workgroups(B);
    const Work w = carve(d_work, param_count(D, A, kH), grid);
    const gxf_status sp = product(B, D, A, d_obs, d_theta, d_x, (double)eps, damping, grid, w, d_y, nullptr, (hipStream_t)stream);
    return sp != GXF_OK ? sp : launched("gxf_fvp");
}

extern "C" gxf_status gxf_cg(int32_t B, int32_t D, int32_t A, int32_t hidden, const float* d_obs, const float* d_theta,
                             const float* d_g, float eps, float damping, int32_t iters, int32_t workgroups, void* d_work,
                             float* d_xhat, float* d_s, float* d_rdot, int32_t* d_iters, void* stream)
{
    if (!d_obs || !d_theta || !d_g || !d_work || !d_xhat || !d_s || !d_rdot || !d_iters)
        return fail(GXF_ERR_ARG, "gxf_cg: null pointer");
    if (iters < 0) return fail(GXF_ERR_ARG, "gxf_cg: negative iters");
    const gxf_status st = check_shape("gxf_cg", B, D, A, hidden, workgroups);
    if (st != GXF_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    const int grid = workgroups ? workgroups : default_workgroups(B);
    const int P = (int)param_count(D, A, kH);
    const Work w = carve(d_work, P, grid);
    hipLaunchKernelGGL(cg_init_kernel, dim3(1), dim3(kCgThreads), 0, s, P, d_g, d_xhat, w.r, w.p, w.st);
    for (int it = 0; it < iters; ++it) {
        const gxf_status sp = product(B, D, A, d_obs, d_theta, w.p, (double)eps, damping, grid, w, w.z, &w.st->stop, s);
        if (sp != GXF_OK) return sp;
        hipLaunchKernelGGL(cg_step_kernel, dim3(1), dim3(kCgThreads), 0, s, P, w.z, d_xhat, w.r, w.p, w.st, (double)eps);
    }
    const gxf_status sp = product(B, D, A, d_obs, d_theta, d_xhat, (double)eps, damping, grid, w, w.z, nullptr, s);
    if (sp != GXF_OK) return sp;
    hipLaunchKernelGGL(cg_finish_kernel, dim3(1), dim3(kCgThreads), 0, s, P, d_xhat, w.z, w.st, d_s, d_rdot, d_iters);
    return launched("gxf_cg");
}
