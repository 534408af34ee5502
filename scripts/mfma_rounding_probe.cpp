// How many fp32 roundings does one f16 MFMA make?  D = C + sum_k a_k b_k with every row and column alike, on operands whose
// exact sum and whose sum under each candidate order of rounding differ (tests/test_gpu_act_craft.py
// "Finding").  Stand-alone: hipcc -O2 --offload-arch=gfx950 scripts/mfma_rounding_probe.cpp -o mfma_rounding_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cmath>
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
__global__ void k32(const _Float16 *a, const _Float16 *b, float c, float *out)
{
    const int lane = threadIdx.x, g = lane >> 4;
    half8 A, B;
    for (int j = 0; j < 8; j++) { A[j] = a[g * 8 + j]; B[j] = b[g * 8 + j]; }
    f32x4 acc = {c, c, c, c};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(A, B, acc, 0, 0, 0);
    if (lane == 0) out[0] = acc[0];
}
__global__ void k16(const _Float16 *a, const _Float16 *b, float c, float *out)
{
    const int lane = threadIdx.x, g = lane >> 4;
    half4 A, B;
    for (int j = 0; j < 4; j++) { A[j] = a[g * 4 + j]; B[j] = b[g * 4 + j]; }
    f32x4 acc = {c, c, c, c};
    acc = __builtin_amdgcn_mfma_f32_16x16x16f16(A, B, acc, 0, 0, 0);
    if (lane == 0) out[0] = acc[0];
}
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)
int main()
{
    _Float16 *da, *db; float *dout;
    CK(hipMalloc(&da, 64)); CK(hipMalloc(&db, 64)); CK(hipMalloc(&dout, 4));
    const float big = 16777216.f;
    auto run = [&](int K, const float *pa, const float *pb, float c, const char *what) -> int {
        _Float16 ha[32], hb[32];
        for (int i = 0; i < 32; i++) { ha[i] = (_Float16)(i < K ? pa[i] : 0.f); hb[i] = (_Float16)(i < K ? pb[i] : 0.f); }
        CK(hipMemcpy(da, ha, 64, hipMemcpyHostToDevice)); CK(hipMemcpy(db, hb, 64, hipMemcpyHostToDevice));
        if (K == 32) hipLaunchKernelGGL(k32, dim3(1), dim3(64), 0, 0, da, db, c, dout);
        else hipLaunchKernelGGL(k16, dim3(1), dim3(64), 0, 0, da, db, c, dout);
        CK(hipDeviceSynchronize());
        float r; CK(hipMemcpy(&r, dout, 4, hipMemcpyDeviceToHost));
        double exact = c; for (int i = 0; i < K; i++) exact += (double)(float)ha[i] * (double)(float)hb[i];
        printf("K=%d %-44s result - 2^24 = %.4f   exact - 2^24 = %.4f\n", K, what, (double)r - big, exact - big);
        return 0;
    };
    for (int K : {32, 16}) {
        float a[32], b[32];
        for (float p : {1.f, 0.75f, 0.375f, 0.1875f, 0.09375f, 0.046875f}) {
            for (int i = 0; i < 32; i++) { a[i] = p; b[i] = 1.f; }
            char w[64]; snprintf(w, sizeof w, "C = 2^24, every product %g", p);
            if (run(K, a, b, big, w)) return 1;
        }
        for (int at : {0, K / 2, K - 1}) {
            for (float p : {0.75f, 0.375f, 0.1875f}) {
                for (int i = 0; i < 32; i++) { a[i] = p; b[i] = 1.f; }
                a[at] = 4096.f; b[at] = 4096.f;
                char w[64]; snprintf(w, sizeof w, "C = 0, product %d = 2^24, the others %g", at, p);
                if (run(K, a, b, 0.f, w)) return 1;
            }
        }
        // cancellation: +2^24 and -2^24 among the products, small ones between them
        for (int i = 0; i < 32; i++) { a[i] = 0.75f; b[i] = 1.f; }
        a[0] = 4096.f; b[0] = 4096.f; a[K - 1] = -4096.f; b[K - 1] = 4096.f;
        if (run(K, a, b, big, "C = 2^24, p0 = 2^24, p_last = -2^24, others .75")) return 1;
    }
    return 0;
}
