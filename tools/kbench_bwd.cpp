// kbench_bwd.cpp -- developer micro-benchmark of the scorer's backward kernels at the reference's training size
// (B = 12 per-sample rotation sets of N = 3000), kernel by kernel.  Not part of the product.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -I3dahv_amd/csrc -Iinclude tools/kbench_bwd.cpp -o tools/kbench_bwd
// (tools/build_kbench.sh; tests/test_tools_build_cpu.py compiles it with every suite run).  The kernels as the library launches
// them: every grid is backward_grid and the dW1 partials are sized by BackwardWs (ahv_launch.h), as in launch_score_backward.
// -DAHV_RMW_STAMPS adds the dV kernel's in-kernel phase times.
#include "../3dahv_amd/csrc/ahv_backward.hip"
#include "../3dahv_amd/csrc/ahv_bwd_volume.hip"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

// the library's launcher (never called here) refers to the zero-fill launcher of ahv_ops.hip
namespace ahv { hipError_t launch_zero_fill(void* const*, const size_t*, int, hipStream_t) { return hipErrorNotSupported; } }

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); return 1; } } while (0)

int main(int argc, char** argv)
{
    const int B = argc > 1 ? atoi(argv[1]) : 12;
    const long N = argc > 2 ? atol(argv[2]) : 3000;
    const int iters = argc > 3 ? atoi(argv[3]) : 10;
    std::mt19937 rng(0);
    std::normal_distribution<float> nd(0.f, 1.f);
    std::vector<float> vol((size_t)B * 8192), ft((size_t)B * 2048), R((size_t)B * N * 9), W1(32 * 384), W2(1024), b2(32), gs((size_t)B * N);
    for (auto& x : vol) x = 1.15f * nd(rng);
    for (auto& x : ft) x = nd(rng) / 5.6f;
    for (auto& x : W1) x = nd(rng) * 0.03f;
    for (auto& x : W2) x = nd(rng) * 0.1f;
    for (auto& x : b2) x = nd(rng) * 0.1f;
    for (auto& x : gs) x = nd(rng);
    for (long n = 0; n < B * N; ++n) {
        double q[4], s = 0;
        for (double& c : q) { c = nd(rng); s += c * c; }
        const double t = 2.0 / s, r = q[0], i = q[1], j = q[2], k = q[3];
        const double m[9] = {1 - t * (j * j + k * k), t * (i * j - k * r), t * (i * k + j * r), t * (i * j + k * r), 1 - t * (i * i + k * k),
                             t * (j * k - i * r), t * (i * k - j * r), t * (j * k + i * r), 1 - t * (i * i + j * j)};
        for (int e = 0; e < 9; ++e) R[n * 9 + e] = (float)m[e];
    }
    int cu = 0;
    CK(hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, 0));
    float *dvol, *dft, *dR, *dW1, *dW2, *db2, *dgs, *dws, *gvol, *gft, *gW1, *gW2, *gb2, *dpart;
    CK(hipMalloc(&dvol, vol.size() * 4)); CK(hipMalloc(&dft, ft.size() * 4)); CK(hipMalloc(&dR, R.size() * 4));
    CK(hipMalloc(&dW1, W1.size() * 4)); CK(hipMalloc(&dW2, W2.size() * 4)); CK(hipMalloc(&db2, b2.size() * 4));
    CK(hipMalloc(&dgs, gs.size() * 4)); CK(hipMalloc(&dws, (size_t)B * N * 2048 * 4));
    CK(hipMalloc(&dpart, ahv::BackwardWs(B, N, cu).partials * 32 * 384 * 4)); CK(hipMalloc(&gvol, vol.size() * 4)); CK(hipMalloc(&gft, ft.size() * 4)); CK(hipMalloc(&gW1, W1.size() * 4));
    CK(hipMalloc(&gW2, W2.size() * 4)); CK(hipMalloc(&gb2, b2.size() * 4));
    CK(hipMemcpy(dvol, vol.data(), vol.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(dft, ft.data(), ft.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dR, R.data(), R.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(dW1, W1.data(), W1.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dW2, W2.data(), W2.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(db2, b2.data(), b2.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dgs, gs.data(), gs.size() * 4, hipMemcpyHostToDevice));
    const dim3 grid_head = ahv::backward_grid(cu, B, N, ahv::kBwdHeadPerWg), grid_w1 = ahv::backward_grid(cu, B, N, ahv::kBwdW1PerWg);
    const dim3 grid_vol = ahv::backward_grid(cu, B, N, ahv::kBwdVolumePerWg), grid_saved = ahv::backward_grid(cu, B, N, ahv::kBwdHeadSavedPerWg);
    hipEvent_t e[5];
    for (auto& x : e) CK(hipEventCreate(&x));
    double t[4] = {0, 0, 0, 0};
    for (int it = -2; it < iters; ++it) {
        CK(hipMemsetAsync(gvol, 0, vol.size() * 4, 0)); CK(hipMemsetAsync(gft, 0, ft.size() * 4, 0));
        CK(hipMemsetAsync(gW1, 0, W1.size() * 4, 0)); CK(hipMemsetAsync(gW2, 0, 4096, 0)); CK(hipMemsetAsync(gb2, 0, 128, 0));
        CK(hipEventRecord(e[0], 0));
        hipLaunchKernelGGL(ahv::score_backward_head_kernel<true>, grid_head, dim3(ahv::kBwdThreads), 0, 0, dvol, dft, dR, (long)(N * 9), dW1, dW2, db2,
                           B, N, dgs, dws, gft, gW2, gb2);
        CK(hipEventRecord(e[1], 0));
        hipLaunchKernelGGL(ahv::score_backward_w1_kernel, grid_w1, dim3(ahv::kW1Threads), 0, 0, dvol, dR, (long)(N * 9), B, N, dws, dpart);
        hipLaunchKernelGGL(ahv::score_backward_w1_reduce_kernel, dim3(32 * 384 / 256, 16), dim3(256), 0, 0, dpart, (int)(grid_w1.x * grid_w1.y), gW1);
        CK(hipEventRecord(e[2], 0));
        hipLaunchKernelGGL(ahv::score_backward_volume_rmw_kernel, grid_vol, dim3(ahv::kRmwThreads), 0, 0, dR, (long)(N * 9), dW1, B, N, dws, gvol);
        CK(hipEventRecord(e[3], 0));
        // the training pair's head kernel (u from the workspace; for the clock any 8 KB per hypothesis will do: du stands in)
        hipLaunchKernelGGL(ahv::score_backward_head_saved_kernel, grid_saved, dim3(ahv::kSavedThreads), 0, 0, dft, dW2, db2,
                           B, N, dgs, dws, gft, gW2, gb2);
        CK(hipEventRecord(e[4], 0));
        CK(hipEventSynchronize(e[4]));
        CK(hipGetLastError());
        if (it >= 0)
            for (int k = 0; k < 4; ++k) { float ms; CK(hipEventElapsedTime(&ms, e[k], e[k + 1])); t[k] += ms; }
    }
    std::vector<float> hv(vol.size());
    CK(hipMemcpy(hv.data(), gvol, vol.size() * 4, hipMemcpyDeviceToHost));
    printf("B=%d N=%ld: head %.3f ms  dW1 %.3f ms   (grad_vol[0..2] = %g %g %g)\n", B, N, t[0] / iters, t[1] / iters, hv[0], hv[1], hv[2]);
#ifdef AHV_RMW_STAMPS
    {
        unsigned long long hs[64];
        CK(hipMemcpyFromSymbol(hs, HIP_SYMBOL(ahv::g_rmw_stamps), sizeof(hs)));
        static const char* nm[8] = {"loop head", "wait done", "corners", "dX half 0", "wait ready", "scatter 0", "dX half 1", "scatter 1"};
        const double nh = (double)N / (2.0 * grid_vol.x) * ((B + grid_vol.y - 1) / grid_vol.y);   // hypotheses per slot of workgroup (3, 5), roughly
        printf("   workgroup (3, 5): shader-clock cycles per hypothesis and phase (about %.0f hypotheses per slot)\n", nh);
        for (int w = 0; w < 8; ++w) {
            printf("   wave %d (slot %d member %d):", w, w >> 2, w & 3);
            double tot = 0;
            for (int i = 0; i < 8; ++i) { printf(" %s %.0f |", nm[i], hs[w * 8 + i] / nh); tot += hs[w * 8 + i] / nh; }
            printf(" total %.0f\n", tot);
        }
    }
#endif
    printf("           dV read-modify-write kernel %.3f ms  recomputing backward %.3f ms\n", t[2] / iters, (t[0] + t[1] + t[2]) / iters);
    printf("           head kernel of the training pair (u saved by the forward) %.3f ms  total with it %.3f ms\n", t[3] / iters,
           (t[3] + t[1] + t[2]) / iters);
    return 0;
}
