// Plate numbers (include/irmv_hip.h, "plate numbers"): a small MLP on each armor's plate patch, one 64-lane wavefront per
// detection, on the grid of k_patch.hip.  A module of its own, compiled with -ffp-contract=off: every fp32 operation below is
// the one written, in the written order -- four chains a unit, chain q the inputs k = q (mod 4), combined as
// (a0 + a1) + (a2 + a3) --, and irmv_detection_amd/number_net.py follows it operation for operation.
//
// A lane is an output unit (two a lane past 64); the weights lie k-major, [in][out padded], so the wave's load of one k is
// contiguous.  A lane owns the patch's words as the patch kernel writes them -- three a lane -- and the wave takes x_k from
// the lane that holds it with v_readlane, in k order; later layers take the previous layer's activations the same way.  No
// LDS, NO workgroup barrier: waves leave early (past num_dets, enable = 0) and the others must not wait.  No address is formed
// from data: otsu and the gray values are compared and converted, the label is computed; the table, the weights and the
// biases are what the host checked and uploaded.
#include <hip/hip_runtime.h>

#include "irmv_common.hpp"

namespace irmv {

// lane `from` (wave-uniform) of v, on every lane
__device__ inline float num_lane(float v, int from)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), from));
}

struct NumUnit { float c[4]; };   // the four chains of one unit
__device__ inline void num_start(NumUnit &u, const float *b, int unit, int pad) { u.c[0] = unit < pad ? b[unit] : 0.0f; u.c[1] = u.c[2] = u.c[3] = 0.0f; }
__device__ inline float num_weight(const half_t *w, int k, int unit, int pad) { return unit < pad ? (float)w[(size_t)k * pad + unit] : 0.0f; }
__device__ inline float num_sum(const NumUnit &u) { return (u.c[0] + u.c[1]) + (u.c[2] + u.c[3]); }
__device__ inline float num_relu(float a) { return a > 0.0f ? a : 0.0f; }

// the smallest index of the largest value, on every lane
__device__ inline void num_argmax(float &v, int &i)
{
    for (int m = 1; m < 64; m <<= 1) {
        const float ov = __shfl_xor(v, m);
        const int oi = __shfl_xor(i, m);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
}

// One patch record on the whole wave: p and o are wave-uniform.
__device__ inline void number_wave(const DevPatch *p, const NumberTable &tb, const half_t *W, const float *B, DevNumber *o)
{
    const int lane = threadIdx.x & 63;
    uint32_t *words = reinterpret_cast<uint32_t *>(o);
    const uint32_t *pw = reinterpret_cast<const uint32_t *>(p);
    const int state = p->state, otsu = p->otsu;              // (uniform)
    if (state != 1) {                                        // no answer: all 96 bytes zero
        if (lane < kNumRecWords) words[lane] = 0u;
        return;
    }
    // the inputs a lane holds: x[4 r + q] is x_k of k = 4 (lane + 64 r) + q
    const bool gray = tb.input == 1;
    float x[12];
    int ones = 0;
    for (int r = 0; r < 3; r++) {
        const int wi = lane + 64 * r;
        const bool have = wi < kPatchWords;
        const uint32_t word = have ? pw[wi] : 0u;
        for (int q = 0; q < 4; q++) {
            const int g = (int)((word >> (8 * q)) & 255u);
            if (gray) {
                x[4 * r + q] = (float)g / 255.0f;
                ones += g;
            } else {
                const bool one = have && g > otsu;
                x[4 * r + q] = one ? 1.0f : 0.0f;
                ones += one ? 1 : 0;
            }
        }
    }
    for (int m = 1; m < 64; m <<= 1) ones += __shfl_xor(ones, m);
    // the first layer: k = 4 wi + q in ascending order, word wi from lane wi % 64, round wi / 64
    const int u0 = lane, u1 = lane + 64;
    NumUnit c0, c1;
    {
        const int pad = tb.pad[0];
        const bool two = tb.dims[1] > 64;
        const half_t *w = W + tb.w_off[0];
        const float *b = B + tb.b_off[0];
        num_start(c0, b, u0, pad);
        num_start(c1, b, u1, pad);
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const int nl = kPatchWords - 64 * r < 64 ? kPatchWords - 64 * r : 64;
#pragma unroll 4
            for (int l = 0; l < nl; l++) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int k = 4 * (l + 64 * r) + q;
                    const float xk = num_lane(x[4 * r + q], l);
                    c0.c[q] = c0.c[q] + num_weight(w, k, u0, pad) * xk;
                    if (two) c1.c[q] = c1.c[q] + num_weight(w, k, u1, pad) * xk;
                }
            }
        }
    }
    float a0 = num_sum(c0), a1 = num_sum(c1);
    // the later layers: input k is the ReLU output of unit k, on lane k % 64
    for (int layer = 1; layer < tb.n_layers; layer++) {
        const float h0 = num_relu(a0), h1 = num_relu(a1);
        const int n_in = tb.dims[layer], pad = tb.pad[layer];
        const bool two = tb.dims[layer + 1] > 64;
        const half_t *w = W + tb.w_off[layer];
        const float *b = B + tb.b_off[layer];
        num_start(c0, b, u0, pad);
        num_start(c1, b, u1, pad);
        for (int k0 = 0; k0 < n_in; k0 += 4) {
            const float h = k0 < 64 ? h0 : h1;               // (uniform: four neighbouring k lie on one side)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int k = k0 + q;
                if (k < n_in) {
                    const float xk = num_lane(h, k & 63);
                    c0.c[q] = c0.c[q] + num_weight(w, k, u0, pad) * xk;
                    if (two) c1.c[q] = c1.c[q] + num_weight(w, k, u1, pad) * xk;
                }
            }
        }
        a0 = num_sum(c0);
        a1 = num_sum(c1);
    }
    // label and runner-up: logits are finite (the header's bound), -inf stands for "no unit"
    const int C = tb.dims[tb.n_layers];
    const float none = -__builtin_inff();
    const float logit = lane < C ? a0 : none;
    float bv = logit;
    int label = lane;
    num_argmax(bv, label);
    float sv = lane == label ? none : logit;
    int second = lane;
    num_argmax(sv, second);
    float margin = bv - sv;
    if (C < 2) { second = -1; margin = 0.0f; }
    // the record's 24 dwords, one a lane
    const uint32_t lbits = lane < C ? __float_as_uint(a0) : 0u;
    const uint32_t moved = (uint32_t)__shfl((int)lbits, (lane - 8) & 63);
    if (lane < kNumRecWords) {
        const uint32_t head[8] = {1u, (uint32_t)label, (uint32_t)second, (uint32_t)ones, __float_as_uint(margin), 0u, 0u, 0u};
        uint32_t v = moved;
        for (int q = 0; q < 8; q++) v = lane == q ? head[q] : v;
        words[lane] = v;
    }
}

// kPatchPerBlock detections per workgroup, one per wave; grid (ceil(max_det / kPatchPerBlock), batch)
__global__ __launch_bounds__(kPatchThreads) void number_step_kernel(NumberArgs a)
{
    const NumberTable &tb = *a.table;
    if (!tb.enable) return;
    const int b = blockIdx.y, wave = threadIdx.x >> 6, j = blockIdx.x * kPatchPerBlock + wave;
    const int ndet = min(a.num_dets[b * a.num_dets_stride], a.max_det);
    if (j >= ndet) return;
    number_wave(a.patches + (size_t)b * a.max_det + j, tb, a.weights, a.bias, a.out + (size_t)b * a.max_det + j);
}

__global__ __launch_bounds__(kPatchThreads) void number_points_kernel(NumberArgs a, int n)
{
    const int wave = threadIdx.x >> 6, j = blockIdx.x * kPatchPerBlock + wave;
    if (j >= n) return;
    number_wave(a.patches + j, *a.table, a.weights, a.bias, a.out + j);
}

void launch_number_step(const NumberArgs &a, int batch, hipStream_t s)
{
    if (a.max_det <= 0 || batch <= 0) return;
    hipLaunchKernelGGL(number_step_kernel, dim3((a.max_det + kPatchPerBlock - 1) / kPatchPerBlock, batch), dim3(kPatchThreads), 0, s, a);
}

void launch_number_points(const NumberArgs &a, int n, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(number_points_kernel, dim3((n + kPatchPerBlock - 1) / kPatchPerBlock), dim3(kPatchThreads), 0, s, a, n);
}

}  // namespace irmv
