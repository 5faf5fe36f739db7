// tests/debug/rcas_lobe_probe.hip -- compiled and run by tests/test_gpu_rcas_identity.py (never shipped).
// The clamped RCAS lobe of the byte domain, twice per case on the device: the two-quotient form the kernels evaluated before
// rcas_lobe_bytes existed, restated here, and the shipped helper (openvr_fsr_amd/csrc/fsr_device.inc), under the flags and the
// contraction mode of the product kernels.  The test compares the two bit for bit.
//     rcas_lobe_probe CASES.bin OUT.bin     CASES: float32 [n][8] = mnR mxR mnG mxG mnB mxB sharp 0     OUT: uint32 [n][2] = old, new
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>
#include "fsr_params.h"
#include "fsr_launch.h"
#include "fsr_formats.h"
#include "fsr_bounds.h"

namespace ovrfsr_fast {
#define OVRFSR_STRICT 0
#pragma clang fp contract(fast)
#include "fsr_device.inc"

// the form of rcas_resolve_bytes<true> before the one-quotient helper: hitMin and hitMax per channel, PEAK = 255
__device__ __forceinline__ float lobe_two_quotients(float mnR, float mxR, float mnG, float mxG, float mnB, float mxB, float sharp)
{
    constexpr float PEAK = 255.0f;
    const float hitMinR = mnR * __builtin_amdgcn_rcpf(4.0f * mxR);
    const float hitMinG = mnG * __builtin_amdgcn_rcpf(4.0f * mxG);
    const float hitMinB = mnB * __builtin_amdgcn_rcpf(4.0f * mxB);
    const float hitMaxR = (PEAK - mxR) * __builtin_amdgcn_rcpf(4.0f * mnR + -4.0f * PEAK);
    const float hitMaxG = (PEAK - mxG) * __builtin_amdgcn_rcpf(4.0f * mnG + -4.0f * PEAK);
    const float hitMaxB = (PEAK - mxB) * __builtin_amdgcn_rcpf(4.0f * mnB + -4.0f * PEAK);
    const float lobeR = fmaxf(-hitMinR, hitMaxR), lobeG = fmaxf(-hitMinG, hitMaxG), lobeB = fmaxf(-hitMinB, hitMaxB);
    return __builtin_amdgcn_fmed3f(fmaxf(lobeR, fmaxf(lobeG, lobeB)), -OVRFSR_RCAS_LIMIT, 0.0f) * sharp;
}

__global__ __launch_bounds__(256) void lobe_probe_kernel(const float *__restrict__ cases, uint32_t *__restrict__ out, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float *c = cases + (size_t)i * 8u;
    out[2u * i] = __float_as_uint(lobe_two_quotients(c[0], c[1], c[2], c[3], c[4], c[5], c[6]));
    out[2u * i + 1u] = __float_as_uint(rcas_lobe_bytes(c[0], c[1], c[2], c[3], c[4], c[5], c[6]));
}
#undef OVRFSR_STRICT
} // namespace ovrfsr_fast

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s CASES.bin OUT.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (bytes <= 0 || bytes % 32 != 0) { fprintf(stderr, "%s: %ld bytes is not a whole number of 32-byte cases\n", argv[1], bytes); return 2; }
    const uint32_t n = (uint32_t)(bytes / 32);
    std::vector<float> cases((size_t)n * 8);
    if (fread(cases.data(), 32, n, f) != n) { fprintf(stderr, "%s: short read\n", argv[1]); return 2; }
    fclose(f);
    float *d_cases = nullptr;
    uint32_t *d_out = nullptr;
    CHECK(hipMalloc((void **)&d_cases, (size_t)n * 32));
    CHECK(hipMalloc((void **)&d_out, (size_t)n * 8));
    CHECK(hipMemcpy(d_cases, cases.data(), (size_t)n * 32, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(ovrfsr_fast::lobe_probe_kernel, dim3((n + 255u) / 256u), dim3(256), 0, 0, d_cases, d_out, n);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<uint32_t> out((size_t)n * 2);
    CHECK(hipMemcpy(out.data(), d_out, (size_t)n * 8, hipMemcpyDeviceToHost));
    CHECK(hipFree(d_cases));
    CHECK(hipFree(d_out));
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    if (fwrite(out.data(), 8, n, f) != n) { fprintf(stderr, "%s: short write\n", argv[2]); return 2; }
    fclose(f);
    printf("rcas_lobe_probe: %u cases\n", n);
    return 0;
}
