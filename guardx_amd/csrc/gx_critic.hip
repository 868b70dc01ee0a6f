// gx_critic.hip -- libguardx_critic.so (include/guardx_critic.h): the cost critic `ac.vc` of the CPO-family learners
// (safe_rl_libX/cpo/cpo_core.py) evaluated over rows of observations, e.g. everything a fused rollout_policy recorded
// (obs (T, N, D) and obs_last (N, D): M = T N + N rows), in one batched pass on the caller's stream.
//
// The arithmetic is the fused rollout's value head (gx_policy.h) and the checker's (oracle/gx_oracle.c:mlp_forward):
// every hidden unit is one v_mfma_f32_16x16x4_f32 chain over k ascending, started from its bias (that instruction
// accumulates exactly like a sequential fmaf chain, tools/probes/mfma_f32_probe.hip), then tanh_f; the output is 16 lane
// partials over the units 64 c + 4 l + j folded by the butterfly of head2_out.  So Vc(row) has the bits the in-kernel
// critic would give for the same weights, whichever hidden width.
//
// Organisation: a 256-thread workgroup (4 waves) takes tiles of 32 rows, grid-striding over them.  Waves 2 g and 2 g + 1
// own the 16 rows of group g and one half of the hidden units each (H / 32 output tiles of 16 units per wave: the
// streaming form of gx_policy.h, polS_chain / polS_store).  The B operands are the hidden layers transposed to
// [k][unit] (critic_transpose_kernel, into the caller's workspace): 27 KB at h = 64, 0.3 MB at h = 256, read by every
// workgroup and resident in L2; they are fetched eight k-steps ahead of the MFMAs that consume them.  The A operands
// (observation rows zero-padded to a multiple of four, then the first hidden layer) come from LDS.
#include "../../include/guardx_critic.h"
#include "gx_policy.h"
#include <hip/hip_runtime.h>
#include <string>

#ifndef GXC_BUILD_ID
#define GXC_BUILD_ID "unknown"
#endif

namespace {

using namespace gx;

thread_local std::string g_err;

gxc_status fail(gxc_status st, const std::string& msg)
{
    g_err = msg;
    return st;
}

constexpr int kRows = 32;     // rows per tile: two groups of 16, two waves each
constexpr int kThreads = 256;
constexpr size_t kLdsMax = 160 * 1024;

bool width_ok(int H) { return H == 64 || H == 128 || H == 192 || H == 256; }
int64_t critic_floats(int D, int H) { return (int64_t)H * D + H + (int64_t)H * H + H + H + 1; }
int64_t work_floats(int D, int H) { return (int64_t)pad4(D) * H + (int64_t)H * H; }
// LDS: head (b1 b2 W3 b3) | H1 [32][H + 4] | H2 [32][H + 4] | X [32][pad4 D + 1]
size_t lds_floats(int D, int H) { return (size_t)pad4(mlp2_head_floats(1, H)) + 2 * kRows * (H + 4) + (size_t)kRows * (pad4(D) + 1); }

// wt = Wt1 [pad4 D][H] (rows D .. pad4 D - 1 zero) | Wt2 [H][H], from the torch layout W1 [H][D] b1 W2 [H][H] ...
__global__ void critic_transpose_kernel(const float* __restrict__ params, float* __restrict__ wt, int D, int H)
{
    const int Dp = pad4(D);
    const long long n1 = (long long)Dp * H, n = n1 + (long long)H * H;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        if (i < n1) {
            const int k = (int)(i / H), j = (int)(i - (long long)k * H);
            wt[i] = k < D ? params[(size_t)j * D + k] : 0.0f;
        } else {
            const long long r = i - n1;
            const int k = (int)(r / H), j = (int)(r - (long long)k * H);
            wt[i] = params[(size_t)H * D + H + (size_t)j * H + k];
        }
    }
}

template <int H>
__global__ __launch_bounds__(kThreads) void critic_kernel(int M, int D, const float* __restrict__ params,
                                                          const float* __restrict__ wt, const float* __restrict__ x,
                                                          float* __restrict__ out)
{
    constexpr int TT = H / 32, HS = H + 4;
    extern __shared__ float4 cr_lds4[];
    float* head = reinterpret_cast<float*>(cr_lds4);
    float* H1 = head + pad4(mlp2_head_floats(1, H));
    float* H2 = H1 + kRows * HS;
    float* X = H2 + kRows * HS;
    const int Dp = pad4(D), XS = Dp + 1;
    const int tid = threadIdx.x, wave = tid >> 6, lw = tid & 63, c16 = lw & 15, kq = lw >> 4;
    const int grp = wave >> 1, col0 = 16 * TT * (wave & 1), l = tid & 15;
    mlp2_head_stage(head, params, D, 1, tid, kThreads, H);
    const Mlp2Head hd = mlp2_head_view(head, 1, H);
    const float* wt1 = wt;
    const float* wt2 = wt + (size_t)Dp * H;
    float* h1 = H1 + grp * 16 * HS;
    float* h2 = H2 + grp * 16 * HS;
    const long long ntiles = ((long long)M + kRows - 1) / kRows;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long r0 = tile * kRows;
        for (int i = tid; i < kRows * Dp; i += kThreads) {
            const int r = i / Dp, k = i - r * Dp;
            const long long row = r0 + r;
            X[r * XS + k] = (row < M && k < D) ? x[row * D + k] : 0.0f;
        }
        wg_sync_lds(); // (on the first tile this also publishes the head)
        mfma_f4 acc[TT];
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) { const float bb = hd.b1[col0 + TT * c16 + tt]; acc[tt] = mfma_f4{bb, bb, bb, bb}; }
        polS_chain<TT>(acc, wt1, H, col0, X + grp * 16 * XS, XS, Dp, c16, kq);
        polS_store<TT>(acc, h1 + col0, HS, c16, kq);
        wg_sync_lds();
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) { const float bb = hd.b2[col0 + TT * c16 + tt]; acc[tt] = mfma_f4{bb, bb, bb, bb}; }
        polS_chain<TT>(acc, wt2, H, col0, h1, HS, H, c16, kq);
        polS_store<TT>(acc, h2 + col0, HS, c16, kq);
        wg_sync_lds();
        // output layer: 16 lanes per row, 16 rows per pass.  The next tile writes X first (read by nobody past the
        // barrier above) and H1 / H2 only behind the next barriers, so no barrier closes the tile.
#pragma unroll
        for (int p = 0; p < kRows / 16; ++p) {
            const int r = 16 * p + (tid >> 4);
            const float v = head2_out<H>(hd, 0, l, H2 + r * HS);
            if (l == 0 && r0 + r < M) out[r0 + r] = v;
        }
    }
}

template <int H>
gxc_status launch(int M, int D, const float* params, const float* x, float* out, float* work, hipStream_t s)
{
    const long long n = work_floats(D, H);
    const unsigned tblocks = (unsigned)std::min<long long>((n + 255) / 256, 1024);
    hipLaunchKernelGGL(critic_transpose_kernel, dim3(tblocks), dim3(256), 0, s, params, work, D, H);
    const size_t lds = sizeof(float) * lds_floats(D, H);
    auto kern = critic_kernel<H>;
    if (lds > 64 * 1024) // more dynamic LDS than the default cap: raise it for this kernel
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    int dev = 0, cus = 0, per = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return fail(GXC_ERR_HIP, "gxc_critic_values: no HIP device");
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kern, kThreads, lds) != hipSuccess || per < 1) per = 1;
    const long long ntiles = ((long long)M + kRows - 1) / kRows;
    const unsigned grid = (unsigned)std::min<long long>(ntiles, (long long)cus * per);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), lds, s, M, D, params, work, x, out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GXC_OK : fail(GXC_ERR_HIP, std::string("gxc_critic_values launch failed: ") + hipGetErrorString(e));
}

} // namespace

extern "C" const char* gxc_last_error(void) { return g_err.c_str(); }

extern "C" const char* gxc_build_id(void) { return GXC_BUILD_ID; } // guardx_amd/build.py:LIBRARIES["critic"].source_hash()

extern "C" int64_t gxc_critic_floats(int32_t D, int32_t hidden)
{
    return (D >= 1 && width_ok(hidden)) ? critic_floats(D, hidden) : -1;
}

extern "C" int64_t gxc_critic_work_floats(int32_t D, int32_t hidden)
{
    return (D >= 1 && width_ok(hidden)) ? work_floats(D, hidden) : -1;
}

extern "C" gxc_status gxc_critic_values(int32_t M, int32_t D, int32_t hidden, const float* d_params, const float* d_x,
                                        float* d_out, float* d_work, void* stream)
{
    if (!d_params || !d_x || !d_out || !d_work) return fail(GXC_ERR_ARG, "gxc_critic_values: null pointer");
    if (M < 0 || D < 1) return fail(GXC_ERR_ARG, "gxc_critic_values: M must be >= 0 and D >= 1");
    if (!width_ok(hidden)) return fail(GXC_ERR_UNSUPPORTED, "gxc_critic_values: hidden width not in {64, 128, 192, 256}");
    if (sizeof(float) * lds_floats(D, hidden) > kLdsMax)
        return fail(GXC_ERR_UNSUPPORTED, "gxc_critic_values: D too wide for the LDS tile");
    if (M == 0) return GXC_OK;
    hipStream_t s = (hipStream_t)stream;
    switch (hidden) {
    case 64: return launch<64>(M, D, d_params, d_x, d_out, d_work, s);
    case 128: return launch<128>(M, D, d_params, d_x, d_out, d_work, s);
    case 192: return launch<192>(M, D, d_params, d_x, d_out, d_work, s);
    default: return launch<256>(M, D, d_params, d_x, d_out, d_work, s);
    }
}
