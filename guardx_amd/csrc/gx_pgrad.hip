// gx_pgrad.hip -- libguardx_pgrad.so (include/guardx_pgrad.h): the flat gradients of the learners' two surrogate losses over
// the Gaussian MLP actor (hidden width 64) and CPO's step direction, on the caller's stream and without a host
// synchronisation.  The header fixes the arithmetic; this file is its order of work:
//
//   grad_kernel<KS1, NG>   a persistent grid of 4-wave workgroups; workgroup g walks the 64-row tiles g, g + grid, ... of obs,
//                  in the shape of gx_vfit.hip:grad_kernel.  NG = 1: the gradient of loss_pi; NG = 2: that of surr_cost as
//                  well, from the same forward pass.  LDS holds W2, W3 and the biases, the tile of obs and its activations;
//                  W1 is a B operand that a lane never shares (wave w owns the hidden units 16 w .. + 15), so each lane keeps
//                  its KS1 of them in registers.  Per tile, with a workgroup barrier (LDS only) after each stage:
//                    1  z1 = o W1' + b1 -> h1                       (K = pad4 D; four chains: sum_acc)
//                    2  z2 = h1 W2' + b2 -> h2                      (K = 64; four chains)
//                    3  mu = h2 W3' + b3                            (wave w: rows 16 w ..)
//                    R  lane 4 i + p of wave w: row 16 w + i, the actions p, p + 4, ...: logp and ratio in the line search's
//                       words, the row weights c, this lane's entries of dmu (0 for rows past B) and its terms of dlog_std
//                    4  gz2 = (dmu W3)(1 - h2^2)  (K = 16, the padded action width);  gW3 += dmu' h2, gb3 += dmu' 1
//                    5  gW2 += gz2' h1, gb2 += gz2' 1;  gz1 = (gz2 W2)(1 - h1^2)
//                    6  gW1 += gz1' o, gb1 += gz1' 1
//                  Stages 4 to 6 run once per gradient inside the stage, on tiles of their own (dmu, gz2, gz1 per gradient):
//                  the two backwards share the forward's h1, h2, 1 - h^2 and the operands W3, W2, o, and their chains are
//                  independent, so one's MFMAs issue under the other's.  (The two dmu are not packed into one 16-column
//                  tile: that would save stage 4's 32 weight-gradient MFMAs per wave of some 600 and needs a second path for
//                  A > 8.)  The sums over a tile's 64 rows start from zero and are added to the workgroup's running sums
//                  after the stage, so that no float32 chain is longer than a tile.  The next tile's rows are loaded into
//                  registers while this one is computed.  The workgroup writes NG partial vectors of P floats (their log_std
//                  entries zero) and kSums float64: the three sums of the means and NG x 16 of dlog_std.  Past D = 72
//                  (KS1 = 24, 32) the compiler spills NG = 2 to scratch (36 and 132 bytes per lane), so there the second
//                  gradient is a second launch of NG = 1 with adc as the row weight: the same arithmetic, a second forward.
//   reduce_kernel  one lane per entry of a gradient: the partial vectors' entries (the float64 ones for log_std) added in
//                  workgroup order in float64, rounded once.  Workgroup (0, 0) also adds the sums of the means, staged
//                  through LDS, and writes info.
//   cpo_kernel     one workgroup: the three float64 dots in a fixed order, the ladder on lane 0, x_direction by all lanes.
// No atomics anywhere: the same arguments give the same bits.  tanh_act and sum_acc are gx_fisher.hip's, restated (a shared
// header would move the build ids of the libraries that hold them).
#include "../../include/guardx_pgrad.h"
#include "gx_policy.h"
#include <cmath>
#include <string>

#ifndef GXG_BUILD_ID
#define GXG_BUILD_ID "unknown"
#endif

namespace {

using gx::mfma_f4;
using gx::wg_sync_lds;

thread_local std::string g_err;

gxg_status fail(gxg_status st, const std::string& msg)
{
    g_err = msg;
    return st;
}

constexpr int kH = gx::kPolHd;   // hidden width
constexpr int kTile = 64;        // rows of obs per tile
constexpr int kThreads = 256;    // four waves; wave w owns the hidden units 16 w .. 16 w + 15 and the rows 16 w .. 16 w + 15
constexpr int kAp = 16;          // the action width padded to one MFMA tile
constexpr int kSW = 66;          // LDS row stride of everything 64 wide: 16 rows x 2 k of a ds_read_b32 group hit 32 banks
constexpr int kSU = 18;          // ... of mu and dmu (64 x 16)
constexpr int kDefaultWg = 256;  // one workgroup per CU of the MI355X: the LDS image is over half a CU's 160 KB
constexpr int kMaxWg = 4096;
constexpr int kMaxD = 128;
constexpr int kAcc = 4;          // interleaved chains of a forward product (stages 1 to 3): see sum_acc
constexpr int kSums = 4 + 2 * kAp;   // float64 per workgroup: sum ratio adv, sum ratio adc, sum l - logp, (unused), dlog_std of g, of b
constexpr int kDbl = 3 * kAp + 4 * kSums;   // float64 at the head of LDS: log_std, 1 / v1, 1 / (2 v1) per action; the waves' sums
constexpr int kFusedKS1 = 18;    // the widest first layer (in k-steps) whose two-gradient kernel stays out of scratch
constexpr int kCpoThreads = 1024;
constexpr double kEps = 1e-8;
constexpr double kHalfLog2Pi = 0.91893853320467274178;

// row stride of the obs tile: at least the 16 NT1 columns stage 6 reads, = 2 mod 32
constexpr int nt1_of(int KS1) { return (KS1 + 3) / 4; }
constexpr int obs_stride(int KS1) { return (16 * nt1_of(KS1) - 2 + 31) / 32 * 32 + 2; }
// W2, W3, b1 b2 b3, O, H1, H2 (then gz1 of g), GZ2 per gradient, gz1 of b, MU, DMU per gradient
constexpr int lds_floats(int KS1, int NG)
{
    return 2 * kDbl + kH * kSW + kAp * kSW + 2 * kH + kAp + kTile * obs_stride(KS1) + (2 + NG + (NG - 1)) * kTile * kSW + (1 + NG) * kTile * kSU;
}

int64_t param_count(int D, int A, int h) { return (int64_t)A + (int64_t)h * D + h + (int64_t)h * h + h + (int64_t)A * h + A; }
int tiles_of(int B) { return (int)(((int64_t)B + kTile - 1) / kTile); }
int default_workgroups(int B) { return tiles_of(B) < kDefaultWg ? tiles_of(B) : kDefaultWg; }

struct GradArgs {
    int B, D, A, tiles;
    const float *theta, *obs, *act, *adv, *logp_old, *adc;   // adc may be null where NG == 1
    int cost, vectors;  // NG == 1: the gradient of surr_cost (slot 1) instead of loss_pi's (slot 0); partial vectors per workgroup
    float* partial;     // [grid][vectors][P]
    double* sums;       // [grid][kSums]
    double inv_b;       // 1 / B
};

#define GXG_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0)

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

template <int KS1, int NG>
__global__ __launch_bounds__(kThreads) void grad_kernel(GradArgs a)
{
    constexpr int NT1 = nt1_of(KS1), SO = obs_stride(KS1);
    extern __shared__ double lds_d[];
    double* const LS = lds_d;              // log_std
    double* const IV = LS + kAp;           // 1 / v1
    double* const I2 = IV + kAp;           // 1 / (2 v1)
    double* const WS = I2 + kAp;           // [wave][kSums]
    float* const W2 = reinterpret_cast<float*>(lds_d + kDbl);
    float* const W3 = W2 + kH * kSW;       // [kAp][kSW], the rows past A zero
    float* const b1 = W3 + kAp * kSW;
    float* const b2 = b1 + kH;
    float* const b3 = b2 + kH;
    float* const O = b3 + kAp;
    float* const H1 = O + kTile * SO;
    float* const H2 = H1 + kTile * kSW;    // h2, then gz1 of gradient 0
    float* const GZ2 = H2 + kTile * kSW;   // [NG]
    float* const GZ1B = GZ2 + NG * kTile * kSW;                 // gz1 of gradient 1 (NG - 1 tiles)
    float* const MU = GZ1B + (NG - 1) * kTile * kSW;
    float* const DMU = MU + kTile * kSU;   // [NG], the columns past A zero

    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, c = lane & 15, q = lane >> 4;
    const int D = a.D, A = a.A;
    const int P = A + kH * D + kH + kH * kH + kH + A * kH + A;
    const int oW1 = A, ob1 = oW1 + kH * D, oW2 = ob1 + kH, ob2 = oW2 + kH * kH, oW3 = ob2 + kH, ob3 = oW3 + A * kH;
    const float* __restrict__ th = a.theta;

    // ---- the LDS image of theta, and this lane's W1 operands
    static_assert(kH * kH % kThreads == 0 && kAp * kH % kThreads == 0, "whole passes");
#pragma unroll
    for (int p = 0; p < kH * kH / kThreads; ++p) {
        const int i = tid + kThreads * p;
        W2[(i >> 6) * kSW + (i & 63)] = th[oW2 + i];
    }
#pragma unroll
    for (int p = 0; p < kAp * kH / kThreads; ++p) {
        const int i = tid + kThreads * p;
        W3[(i >> 6) * kSW + (i & 63)] = (i >> 6) < A ? th[oW3 + i] : 0.0f;
    }
    if (tid < kH) {
        b1[tid] = th[ob1 + tid];
        b2[tid] = th[ob2 + tid];
    }
    if (tid < kAp) {
        const bool in = tid < A;
        b3[tid] = in ? th[ob3 + tid] : 0.0f;
        const double ls = in ? (double)th[tid] : 0.0;
        const double v1 = exp(2.0 * ls);
        LS[tid] = ls;
        IV[tid] = 1.0 / v1;
        I2[tid] = 1.0 / (2.0 * v1);
    }
    for (int i = tid; i < kTile * SO; i += kThreads) O[i] = 0.0f;          // the columns past D stay zero
    for (int i = tid; i < NG * kTile * kSU; i += kThreads) DMU[i] = 0.0f;  // the columns past A stay zero
    float w1[KS1];
#pragma unroll
    for (int s = 0; s < KS1; ++s) {
        const int k = 4 * s + q;
        w1[s] = k < D ? th[oW1 + (16 * w + c) * D + k] : 0.0f;
    }
    // element tid + 256 j of a tile (its rows are contiguous in obs) sits in row (tid + 256 j) / D, column (tid + 256 j) % D of O:
    // walked from j = 0 by steps of 256 = dr D + dc at every tile (a table of KS1 offsets per lane costs KS1 registers)
    const int row0 = tid / D, col0 = tid % D, dr = kThreads / D, dc = kThreads % D;
    float pf[KS1];
    auto load_tile = [&](int t) {
        const float* __restrict__ src = a.obs + (size_t)t * kTile * D;
        const int rows = a.B - t * kTile < kTile ? a.B - t * kTile : kTile;
        const int n = rows * D;                                 // nothing past row B - 1 is read
#pragma unroll
        for (int j = 0; j < KS1; ++j) pf[j] = tid + kThreads * j < n ? src[tid + kThreads * j] : 0.0f;
    };

    // the workgroup's running sums, per gradient: W1 (NT1 column tiles), W2 (4), W3 (this wave's units), the three biases
    mfma_f4 rW1[NG][NT1], rW2[NG][4], rW3[NG], rb1[NG], rb2[NG], rb3[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
#pragma unroll
        for (int n = 0; n < NT1; ++n) rW1[g][n] = splat(0.0f);
#pragma unroll
        for (int n = 0; n < 4; ++n) rW2[g][n] = splat(0.0f);
        rW3[g] = rb1[g] = rb2[g] = rb3[g] = splat(0.0f);
    }
    const int row = tid >> 2, part = tid & 3;                   // stage R: row 16 w + (lane >> 2), the actions part, part + 4, ...
    double run[3] = {0.0, 0.0, 0.0};                            // this lane's sums of ratio adv, ratio adc, l - logp (part 0 only)
    double dls[NG][4];                                          // ... of its actions' terms of dlog_std
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int k = 0; k < 4; ++k) dls[g][k] = 0.0;

    int t = blockIdx.x;
    if (t < a.tiles) load_tile(t);
    wg_sync_lds();                                              // O and DMU are zero before the first rows land in them
    while (t < a.tiles) {
        {
            int rr = row0, cc = col0;
#pragma unroll
            for (int j = 0; j < KS1; ++j) {
                if (rr < kTile) O[rr * SO + cc] = pf[j];
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
        // this lane's share of its row of the batch, in flight too; nothing past row B - 1 is read
        const int64_t grow = (int64_t)t * kTile + row;
        const bool valid = grow < a.B;
        float r_adv = 0.0f, r_lpo = 0.0f, r_adc = 0.0f, r_act[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ac = part + 4 * k;
            r_act[k] = valid && ac < A ? a.act[grow * A + ac] : 0.0f;
        }
        if (valid) {
            r_adv = a.adv[grow];
            r_lpo = a.logp_old[grow];
            if (a.adc) r_adc = a.adc[grow];
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
                    acc[rb][s % kAcc] = GXG_MFMA(O[(16 * rb + c) * SO + 4 * s + q], w1[s], acc[rb][s % kAcc]);
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
                    acc[rb][s % kAcc] = GXG_MFMA(H1[(16 * rb + c) * kSW + 4 * s + q], bw, acc[rb][s % kAcc]);
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
        // ---- 3: this wave's 16 rows
        {
            mfma_f4 acc[kAcc];
#pragma unroll
            for (int i = 0; i < kAcc; ++i) acc[i] = splat(i == 0 ? b3[c] : 0.0f);
#pragma unroll
            for (int s = 0; s < kH / 4; ++s)
                acc[s % kAcc] = GXG_MFMA(H2[(16 * w + c) * kSW + 4 * s + q], W3[c * kSW + 4 * s + q], acc[s % kAcc]);
            const mfma_f4 m = sum_acc(acc);
#pragma unroll
            for (int r = 0; r < 4; ++r) MU[(16 * w + 4 * q + r) * kSU + c] = m[r];
        }
        wg_sync_lds();
        // ---- R: the rows
        {
            double lps = 0.0, da[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int ac = part + 4 * k;
                da[k] = 0.0;
                if (ac < A) {
                    da[k] = (double)r_act[k] - (double)MU[row * kSU + ac];
                    lps += -(da[k] * da[k]) * I2[ac] - LS[ac] - kHalfLog2Pi;
                }
            }
            lps += __shfl_xor(lps, 1);
            lps += __shfl_xor(lps, 2);
            const float lp = (float)lps;
            const float diff = lp - r_lpo;
            const float ratio = (float)exp((double)diff);
            float cw[NG];
            const float c_adv = (float)(-((double)r_adv * (double)ratio) * a.inv_b), c_adc = (float)(((double)r_adc * (double)ratio) * a.inv_b);
            cw[0] = NG == 1 && a.cost ? c_adc : c_adv;
            if (NG == 2) cw[1] = c_adc;
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const double cd = (double)cw[g];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int ac = part + 4 * k;
                    if (ac < A) {
                        const double iv = IV[ac];
                        DMU[g * kTile * kSU + row * kSU + ac] = valid ? (float)((cd * da[k]) * iv) : 0.0f;   // selection, never a product with zero
                        dls[g][k] += valid ? cd * ((da[k] * da[k]) * iv - 1.0) : 0.0;
                    }
                }
            }
            const bool on = valid && part == 0;
            run[0] += on ? (double)(ratio * r_adv) : 0.0;
            run[1] += on && a.adc ? (double)(ratio * r_adc) : 0.0;
            run[2] += on ? (double)(r_lpo - lp) : 0.0;
        }
        wg_sync_lds();
        // ---- 4
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const float* const dm = DMU + g * kTile * kSU;
            float* const gz2 = GZ2 + g * kTile * kSW;
            mfma_f4 z[4];
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) z[rb] = splat(0.0f);
#pragma unroll
            for (int s = 0; s < kAp / 4; ++s) {
                const float bv = W3[(4 * s + q) * kSW + 16 * w + c];
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) z[rb] = GXG_MFMA(dm[(16 * rb + c) * kSU + 4 * s + q], bv, z[rb]);
            }
            mfma_f4 t3 = splat(0.0f), tb = splat(0.0f);
#pragma unroll
            for (int s = 0; s < kTile / 4; ++s) {
                const float av = dm[(4 * s + q) * kSU + c];
                t3 = GXG_MFMA(av, H2[(4 * s + q) * kSW + 16 * w + c], t3);
                tb = GXG_MFMA(av, 1.0f, tb);
            }
            rW3[g] += t3;
            rb3[g] += tb;
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int r = 0; r < 4; ++r) gz2[(16 * rb + 4 * q + r) * kSW + 16 * w + c] = z[rb][r] * d2[rb][r];
        }
        wg_sync_lds();
        // ---- 5
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const float* const gz2 = GZ2 + g * kTile * kSW;
            float* const gz1 = g == 0 ? H2 : GZ1B;              // h2 was last read in stage 4
            mfma_f4 t2[4], tb = splat(0.0f), z[4];
#pragma unroll
            for (int n = 0; n < 4; ++n) t2[n] = splat(0.0f);
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) z[rb] = splat(0.0f);
#pragma unroll
            for (int s = 0; s < kTile / 4; ++s) {
                const float av = gz2[(4 * s + q) * kSW + 16 * w + c];
#pragma unroll
                for (int n = 0; n < 4; ++n) t2[n] = GXG_MFMA(av, H1[(4 * s + q) * kSW + 16 * n + c], t2[n]);
                tb = GXG_MFMA(av, 1.0f, tb);
                const float bv = W2[(4 * s + q) * kSW + 16 * w + c];
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) z[rb] = GXG_MFMA(gz2[(16 * rb + c) * kSW + 4 * s + q], bv, z[rb]);
            }
#pragma unroll
            for (int n = 0; n < 4; ++n) rW2[g][n] += t2[n];
            rb2[g] += tb;
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int r = 0; r < 4; ++r) gz1[(16 * rb + 4 * q + r) * kSW + 16 * w + c] = z[rb][r] * d1[rb][r];
        }
        wg_sync_lds();
        // ---- 6
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const float* const gz1 = g == 0 ? H2 : GZ1B;
            mfma_f4 t1[NT1], tb = splat(0.0f);
#pragma unroll
            for (int n = 0; n < NT1; ++n) t1[n] = splat(0.0f);
#pragma unroll
            for (int s = 0; s < kTile / 4; ++s) {
                const float av = gz1[(4 * s + q) * kSW + 16 * w + c];
#pragma unroll
                for (int n = 0; n < NT1; ++n) t1[n] = GXG_MFMA(av, O[(4 * s + q) * SO + 16 * n + c], t1[n]);
                tb = GXG_MFMA(av, 1.0f, tb);
            }
#pragma unroll
            for (int n = 0; n < NT1; ++n) rW1[g][n] += t1[n];
            rb1[g] += tb;
        }
        wg_sync_lds();                                          // O and gz1 are free for the next tile
        t = tn;
    }

    // ---- the partial vectors: an accumulator's entry r is row 4 q + r, column c of its 16 x 16 tile
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        float* __restrict__ out = a.partial + ((size_t)blockIdx.x * a.vectors + (NG == 2 ? g : a.cost)) * P;
        if (tid < A) out[tid] = 0.0f;                           // log_std: reduce_kernel takes it from the float64 sums
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int unit = 16 * w + 4 * q + r;
#pragma unroll
            for (int n = 0; n < NT1; ++n)
                if (16 * n + c < D) out[oW1 + unit * D + 16 * n + c] = rW1[g][n][r];
#pragma unroll
            for (int n = 0; n < 4; ++n) out[oW2 + unit * kH + 16 * n + c] = rW2[g][n][r];
            if (c == 0) {
                out[ob1 + unit] = rb1[g][r];
                out[ob2 + unit] = rb2[g][r];
            }
            const int act = 4 * q + r;
            if (act < A) {
                out[oW3 + act * kH + 16 * w + c] = rW3[g][r];
                if (w == 0 && c == 0) out[ob3 + act] = rb3[g][r];
            }
        }
    }
    // ---- the float64 sums: a wave's lanes as a tree (the rows of a part: lanes part + 4 i), then the waves in wave order
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double s = run[i];
#pragma unroll
        for (int m = 4; m < 64; m <<= 1) s += __shfl_xor(s, m);
        if (lane == 0) WS[w * kSums + i] = s;
    }
    if (lane == 0) WS[w * kSums + 3] = 0.0;
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double s = dls[g][k];
#pragma unroll
            for (int m = 4; m < 64; m <<= 1) s += __shfl_xor(s, m);
            if (lane < 4) WS[w * kSums + 4 + kAp * (NG == 2 ? g : a.cost) + lane + 4 * k] = s;   // lane = part: the action part + 4 k
        }
    wg_sync_lds();
    // what this launch owns: everything, or (NG == 1) the means and slot 0, or (a second launch for surr_cost) slot 1 alone
    const int first = NG == 1 && a.cost ? 4 + kAp : 0, last = NG == 1 && !a.cost ? 4 + kAp : kSums;
    if (tid >= first && tid < last)
        a.sums[(size_t)blockIdx.x * kSums + tid] = ((WS[tid] + WS[kSums + tid]) + WS[2 * kSums + tid]) + WS[3 * kSums + tid];
}

struct ReduceArgs {
    int P, A, NG, grid, B;
    const float* partial;   // [grid][NG][P]
    const double* sums;     // [grid][kSums]
    const float* theta;     // log_std at its head
    float *g_out, *b_out;   // b_out is null where NG == 1
    double* info;           // 4
};

__global__ __launch_bounds__(kThreads) void reduce_kernel(ReduceArgs a)
{
    __shared__ double sh[kThreads];
    const int tid = threadIdx.x, i = blockIdx.x * kThreads + tid, g = blockIdx.y;
    if (i < a.P) {
        double s = 0.0;
        if (i < a.A) {
#pragma unroll 8
            for (int wg = 0; wg < a.grid; ++wg) s += a.sums[(size_t)wg * kSums + 4 + kAp * g + i];
        } else {
#pragma unroll 8
            for (int wg = 0; wg < a.grid; ++wg) s += (double)a.partial[((size_t)wg * a.NG + g) * a.P + i];
        }
        (g == 0 ? a.g_out : a.b_out)[i] = (float)s;
    }
    if (blockIdx.x != 0 || g != 0) return;                      // uniform over the workgroup
    // the workgroups' sums of the means in workgroup order, 64 workgroups at a time through LDS
    double s = 0.0;
    for (int base = 0; base < a.grid; base += kThreads / 4) {
        const int n = a.grid - base < kThreads / 4 ? a.grid - base : kThreads / 4;
        if (tid < 4 * n) sh[tid] = a.sums[(size_t)(base + (tid >> 2)) * kSums + (tid & 3)];
        __syncthreads();
        if (tid < 3) {
#pragma unroll 16
            for (int wg = 0; wg < n; ++wg) s += sh[4 * wg + tid];
        }
        __syncthreads();
    }
    if (tid < 3) {
        s = s / (double)a.B;
        a.info[tid] = tid == 0 ? -s : s;
    }
    if (tid == 3) {
        double ent = 0.0;
        for (int k = 0; k < a.A; ++k) ent += (double)a.theta[k] + 0.5 + kHalfLog2Pi;
        a.info[3] = ent;
    }
}

struct CpoArgs {
    int P;
    const float *b, *hinv_g, *hinv_b, *approx_g, *s;
    const double* crit;     // c, target_kl
    float* x;
    int32_t* optim_case;
    double* out;            // lam nu q r s A B
};

// the sum of v over the workgroup's lanes in a fixed order (a tree over LDS), known to every lane
__device__ __forceinline__ double wg_sum(double v, double* sh)
{
    const int tid = threadIdx.x;
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
    for (int m = kCpoThreads / 2; m > 0; m >>= 1) {
        if (tid < m) sh[tid] += sh[tid + m];
        __syncthreads();
    }
    return sh[0];
}

// Python's min(u, x) and max(l, y) on floats: the first argument unless the second is smaller / larger
__device__ __forceinline__ double proj(double x, double lo, double hi)
{
    const double m = x < hi ? x : hi;
    return m > lo ? m : lo;
}

__global__ __launch_bounds__(kCpoThreads) void cpo_kernel(CpoArgs a)
{
    __shared__ double sh[kCpoThreads];
    __shared__ double res[2];
    __shared__ int oc;
    const int tid = threadIdx.x;
    double bb = 0.0, q = 0.0;
    for (int i = tid; i < a.P; i += kCpoThreads) {
        const double bi = (double)a.b[i];
        bb += bi * bi;
        q += (double)a.hinv_g[i] * (double)a.approx_g[i];
    }
    bb = wg_sum(bb, sh);
    q = wg_sum(q, sh);
    const double c = a.crit[0], tkl = a.crit[1];
    const bool no_b = bb <= 1e-8 && c < 0.0;                    // uniform: Hinv_b is not read
    double r = 0.0;
    if (!no_b)
        for (int i = tid; i < a.P; i += kCpoThreads) r += (double)a.hinv_b[i] * (double)a.approx_g[i];
    r = wg_sum(r, sh);
    if (tid == 0) {
        double s = 0.0, A = 0.0, B = 0.0, lam, nu;
        int oc_ = 4;
        if (no_b) {
            r = 0.0;
        } else {
            s = (double)a.s[0];
            A = q - r * r / s;
            B = 2.0 * tkl - c * c / s;
            if (c < 0.0 && B < 0.0) oc_ = 3;
            else if (c < 0.0 && B >= 0.0) oc_ = 2;
            else if (c >= 0.0 && B >= 0.0) oc_ = 1;
            else oc_ = 0;
        }
        if (oc_ == 3 || oc_ == 4) {
            lam = sqrt(q / (2.0 * tkl));
            nu = 0.0;
        } else if (oc_ == 1 || oc_ == 2) {
            const double rc = r / c, inf = __builtin_huge_val();
            const double la0 = c < 0.0 ? 0.0 : rc, la1 = c < 0.0 ? rc : inf;
            const double lb0 = c < 0.0 ? rc : 0.0, lb1 = c < 0.0 ? inf : rc;
            const double lam_a = proj(sqrt(A / B), la0, la1);
            const double lam_b = proj(sqrt(q / (2.0 * tkl)), lb0, lb1);
            const double f_a = -0.5 * (A / (lam_a + kEps) + B * lam_a) - r * c / (s + kEps);
            const double f_b = -0.5 * (q / (lam_b + kEps) + 2.0 * tkl * lam_b);
            lam = f_a >= f_b ? lam_a : lam_b;
            const double over = lam * c - r;
            nu = (over > 0.0 ? over : 0.0) / (s + kEps);
        } else {
            lam = 0.0;
            nu = sqrt(2.0 * tkl / (s + kEps));
        }
        a.optim_case[0] = oc_;
        a.out[0] = lam;
        a.out[1] = nu;
        a.out[2] = q;
        a.out[3] = r;
        a.out[4] = s;
        a.out[5] = A;
        a.out[6] = B;
        res[0] = lam;
        res[1] = nu;
        oc = oc_;
    }
    __syncthreads();
    const double lam = res[0], nu = res[1];
    const int oc_ = oc;
    const double scale = 1.0 / (lam + kEps);
    for (int i = tid; i < a.P; i += kCpoThreads) {
        const double hb = oc_ == 4 ? 0.0 : (double)a.hinv_b[i];  // selection: case 4 never reads Hinv_b
        const double hg = oc_ == 0 ? 0.0 : (double)a.hinv_g[i];
        a.x[i] = oc_ > 0 ? (float)(scale * (hg + nu * hb)) : (float)(nu * hb);
    }
}

__global__ __launch_bounds__(kThreads) void trpo_kernel(int P, const float* __restrict__ x_hat, const float* __restrict__ s,
                                                        const double* __restrict__ tkl, float* __restrict__ x)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= P) return;
    const double alpha = sqrt(2.0 * tkl[0] / ((double)s[0] + kEps));
    x[i] = (float)(alpha * (double)x_hat[i]);
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
gxg_status check_shape(const char* who, int B, int D, int A, int hidden, int workgroups)
{
    if (B < 1 || D < 1 || A < 1) return fail(GXG_ERR_ARG, std::string(who) + ": B, D and A must be at least 1");
    if (workgroups < 0 || workgroups > kMaxWg)
        return fail(GXG_ERR_ARG, std::string(who) + ": workgroups must be 0 (the default) .. " + std::to_string(kMaxWg));
    if (hidden != kH) return fail(GXG_ERR_UNSUPPORTED, std::string(who) + " supports hidden width 64, not " + std::to_string(hidden));
    if (D > kMaxD) return fail(GXG_ERR_UNSUPPORTED, std::string(who) + " supports an observation width <= 128, not " + std::to_string(D));
    if (A % 2 || A > kAp) return fail(GXG_ERR_UNSUPPORTED, std::string(who) + " supports an even action width <= 16, not " + std::to_string(A));
    return GXG_OK;
}

int64_t partial_bytes(int64_t P, int grid) { return (4 * 2 * (int64_t)grid * P + 7) / 8 * 8; }
int64_t work_bytes(int64_t P, int grid) { return partial_bytes(P, grid) + 8 * (int64_t)kSums * grid; }

template <int KS1, int NG>
gxg_status launch_grad(const GradArgs& a, int grid, hipStream_t s)
{
    constexpr int lds = lds_floats(KS1, NG) * (int)sizeof(float);
    static_assert(lds <= 160 * 1024, "the LDS image fits one CU");
    static_assert(obs_stride(KS1) >= 4 * KS1 && obs_stride(KS1) >= 16 * nt1_of(KS1), "a row of the obs tile holds what stages 1 and 6 read");
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&grad_kernel<KS1, NG>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (attr != hipSuccess) return fail(GXG_ERR_HIP, std::string("gxg: hipFuncSetAttribute failed: ") + hipGetErrorString(attr));
    hipLaunchKernelGGL((grad_kernel<KS1, NG>), dim3(grid), dim3(kThreads), lds, s, a);
    return GXG_OK;
}

template <int NG>
gxg_status gradient_at(const GradArgs& a, int grid, hipStream_t s)
{
    const int ks = (a.D + 3) / 4;   // k-steps of the first layer: the instantiations of gx_fisher.hip
    if (ks <= 4) return launch_grad<4, NG>(a, grid, s);
    if (ks <= 8) return launch_grad<8, NG>(a, grid, s);
    if (ks <= 11) return launch_grad<11, NG>(a, grid, s);
    if (ks <= 12) return launch_grad<12, NG>(a, grid, s);
    if (ks <= 16) return launch_grad<16, NG>(a, grid, s);
    if (ks <= 18) return launch_grad<18, NG>(a, grid, s);
    if constexpr (NG == 1) {
        if (ks <= 24) return launch_grad<24, NG>(a, grid, s);
        return launch_grad<32, NG>(a, grid, s);
    }
    return fail(GXG_ERR_UNSUPPORTED, "gxg: no two-gradient kernel for this width");   // gxg_gradient never asks for one
}

gxg_status launched(const char* who)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GXG_OK : fail(GXG_ERR_HIP, std::string(who) + " launch failed: " + hipGetErrorString(e));
}

} // namespace

extern "C" const char* gxg_last_error(void) { return g_err.c_str(); }

extern "C" const char* gxg_build_id(void) { return GXG_BUILD_ID; } // guardx_amd/build.py:GRAD_LIBRARIES["pgrad"].source_hash()

extern "C" int64_t gxg_param_count(int32_t D, int32_t A, int32_t hidden)
{
    return (D < 1 || A < 1 || hidden < 1) ? -1 : param_count(D, A, hidden);
}

extern "C" int32_t gxg_default_workgroups(int32_t B) { return B < 1 ? 0 : default_workgroups(B); }

extern "C" int64_t gxg_work_bytes(int32_t B, int32_t D, int32_t A, int32_t workgroups)
{
    if (check_shape("gxg_work_bytes", B, D, A, kH, workgroups) != GXG_OK) return -1;
    return work_bytes(param_count(D, A, kH), workgroups ? workgroups : default_workgroups(B));
}

extern "C" gxg_status gxg_gradient(int32_t B, int32_t D, int32_t A, int32_t hidden, const float* d_theta, const float* d_obs,
                                   const float* d_act, const float* d_adv, const float* d_logp, const float* d_adc,
                                   int32_t workgroups, void* d_work, float* d_g, float* d_b, void* d_info, void* stream)
{
    if (!d_theta || !d_obs || !d_act || !d_adv || !d_logp || !d_work || !d_g || !d_info) return fail(GXG_ERR_ARG, "gxg_gradient: null pointer");
    if ((d_adc == nullptr) != (d_b == nullptr)) return fail(GXG_ERR_ARG, "gxg_gradient: d_adc and d_b must be null together");
    const gxg_status sc = check_shape("gxg_gradient", B, D, A, hidden, workgroups);
    if (sc != GXG_OK) return sc;
    hipStream_t s = (hipStream_t)stream;
    const int grid = workgroups ? workgroups : default_workgroups(B);
    const int NG = d_adc ? 2 : 1;
    const bool fused = (D + 3) / 4 <= kFusedKS1;
    const int P = (int)param_count(D, A, kH);
    GradArgs a;
    a.B = B;
    a.D = D;
    a.A = A;
    a.tiles = tiles_of(B);
    a.theta = d_theta;
    a.obs = d_obs;
    a.act = d_act;
    a.adv = d_adv;
    a.logp_old = d_logp;
    a.adc = d_adc;
    a.cost = 0;
    a.vectors = NG;
    a.partial = static_cast<float*>(d_work);
    a.sums = reinterpret_cast<double*>(static_cast<char*>(d_work) + partial_bytes(P, grid));
    a.inv_b = 1.0 / (double)B;
    gxg_status sg = NG == 2 && fused ? gradient_at<2>(a, grid, s) : gradient_at<1>(a, grid, s);
    if (sg != GXG_OK) return sg;
    if (NG == 2 && !fused) {
        a.cost = 1;
        sg = gradient_at<1>(a, grid, s);
        if (sg != GXG_OK) return sg;
    }
    ReduceArgs r;
    r.P = P;
    r.A = A;
    r.NG = NG;
    r.grid = grid;
    r.B = B;
    r.partial = a.partial;
    r.sums = a.sums;
    r.theta = d_theta;
    r.g_out = d_g;
    r.b_out = d_b;
    r.info = static_cast<double*>(d_info);
    hipLaunchKernelGGL(reduce_kernel, dim3((P + kThreads - 1) / kThreads, NG), dim3(kThreads), 0, s, r);
    return launched("gxg_gradient");
}

extern "C" gxg_status gxg_cpo_direction(int32_t P, const float* d_b, const float* d_hinv_g, const float* d_hinv_b,
                                        const float* d_approx_g, const float* d_s, void* d_crit, float* d_x, int32_t* d_case,
                                        void* d_out, void* stream)
{
    if (!d_b || !d_hinv_g || !d_hinv_b || !d_approx_g || !d_s || !d_crit || !d_x || !d_case || !d_out)
        return fail(GXG_ERR_ARG, "gxg_cpo_direction: null pointer");
    if (P < 1) return fail(GXG_ERR_ARG, "gxg_cpo_direction: P must be at least 1");
    CpoArgs a;
    a.P = P;
    a.b = d_b;
    a.hinv_g = d_hinv_g;
    a.hinv_b = d_hinv_b;
    a.approx_g = d_approx_g;
    a.s = d_s;
    a.crit = static_cast<const double*>(d_crit);
    a.x = d_x;
    a.optim_case = d_case;
    a.out = static_cast<double*>(d_out);
    hipLaunchKernelGGL(cpo_kernel, dim3(1), dim3(kCpoThreads), 0, (hipStream_t)stream, a);
    return launched("gxg_cpo_direction");
}

extern "C" gxg_status gxg_trpo_direction(int32_t P, const float* d_x_hat, const float* d_s, void* d_target_kl, float* d_x, void* stream)
{
    if (!d_x_hat || !d_s || !d_target_kl || !d_x) return fail(GXG_ERR_ARG, "gxg_trpo_direction: null pointer");
    if (P < 1) return fail(GXG_ERR_ARG, "gxg_trpo_direction: P must be at least 1");
    hipLaunchKernelGGL(trpo_kernel, dim3((P + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, P, d_x_hat, d_s,
                       static_cast<const double*>(d_target_kl), d_x);
    return launched("gxg_trpo_direction");
}
