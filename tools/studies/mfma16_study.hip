// Diagnostic micro-study (not part of the library): can a v_mfma_f32_16x16x4_f32 stream keep up with the weight stream that 16-row
// fused FFN tiles need?  A 16-row block reuses each weight fragment half as often as a 32-row block: 1 KB of weights per wave feeds
// four 16x16x4 MFMAs (128 cycles per SIMD) instead of four 32x32x2 MFMAs (256 cycles), so a CU pulls twice the bytes per FLOP.
// Every mode streams the weights with raw buffer loads (SGPR descriptor, constant per-lane offset, ring of RING fragments refilled
// right behind the last MFMA that reads them), as ffn_pc.hip does, and reads its A operand from an LDS tile.  Same FLOPs per launch in
// every mode (256 x 8 waves x 4096 32x32x2 MFMAs = 512 x 8 waves x 4096 16x16x4 MFMAs at half the FLOPs each).
//   32x32x2: 8-wave workgroups, 256 of them (2 waves / SIMD) -- today's fused FFN main loop (tools/studies/mfma_study.hip, run_buf)
//   16x16x4: 8-wave workgroups, 512 of them (2 per CU: 4 waves / SIMD), NT accumulator chains (n tiles) sharing each A value --
//            NT = 2 is the producer of a 16-row block (h[16, 32]), NT = 4 the consumer ([16, 64]); A values read as single dwords in
//            the lane-to-k order of the 32x32x2 chain (tests/test_gpu_mfma_order.py)
//   hipcc --offload-arch=gfx950 -O3 tools/studies/mfma16_study.hip -o mfma16_study && ./mfma16_study
#include <hip/hip_runtime.h>
#include <stdio.h>
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

static constexpr unsigned kMask = 256 * 1024 - 1;       // 1 MB weight stream (L2-resident), in floats

template <int RING, int LOADS>
__global__ __launch_bounds__(512) void study32(float* out, const float* __restrict__ wts, int iters) {
    __shared__ __align__(16) float tile[32 * 260];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 32 * 260; i += 512) tile[i] = (float)(i & 7) * 0.01f;
    __syncthreads();
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float* xa = tile + (lane & 31) * 260 + 4 * (lane >> 5);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)wts, 0, 8 << 20, 0x00020000);
    const unsigned wofs = (unsigned)(blockIdx.x & 7) * 16384 + (unsigned)wave * 4096 + lane * 4;
    f32x4 ring[RING];
#pragma unroll
    for (int k = 0; k < RING; ++k)
        ring[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, ((wofs + k * 256) & kMask) * 4, 0, 0));
    f32x4 a = *reinterpret_cast<const f32x4*>(xa);
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int g = 0; g < RING; ++g) {
            const f32x4 an = *reinterpret_cast<const f32x4*>(xa + ((it * RING + g + 1) & 31) * 8);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], ring[g][q], acc, 0, 0, 0);
                if (LOADS && q == 3)
                    ring[g] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                            rs, ((wofs + (unsigned)((it * RING + g + RING) * 256)) & kMask) * 4, 0, 0));
                __builtin_amdgcn_sched_barrier(0);
            }
            a = an;
        }
    }
    float s = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) s += acc[r];
    out[(size_t)blockIdx.x * blockDim.x + tid] = s;
}

// 16 rows: lane l holds A[l & 15][k(l >> 4)]; per group of four MFMAs one 16-byte weight fragment per lane; the NT chains of one k
// step share the A value, so a group covers 4 / NT k steps
template <int RING, int NT, int LOADS>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) void study16(float* out, const float* __restrict__ wts,
                                                                                        int iters) {
    __shared__ __align__(16) float tile[16 * 260];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 16 * 260; i += 512) tile[i] = (float)(i & 7) * 0.01f;
    __syncthreads();
    f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int kk = lane >> 4;
    const int o0 = (kk & 1) * 4 + (kk >> 1), o1 = o0 + 2;          // k order of the 32x32x2 chain: 8g + {0,4,1,5} then 8g + {2,6,3,7}
    const float* xa = tile + (lane & 15) * 260;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)wts, 0, 8 << 20, 0x00020000);
    const unsigned wofs = (unsigned)(blockIdx.x & 7) * 16384 + (unsigned)wave * 4096 + lane * 4;
    f32x4 ring[RING];
#pragma unroll
    for (int k = 0; k < RING; ++k)
        ring[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, ((wofs + k * 256) & kMask) * 4, 0, 0));
    constexpr int KS = 4 / NT;                                     // k steps per group
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int g = 0; g < RING; ++g) {
            float av[KS];
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const int step = (it * RING + g) * KS + s;         // k step: group 8 (step >> 1), half (step & 1)
                av[s] = xa[((step >> 1) & 31) * 8 + ((step & 1) ? o1 : o0)];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc[q % NT] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q / NT], ring[g][q], acc[q % NT], 0, 0, 0);
                if (LOADS && q == 3)
                    ring[g] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                            rs, ((wofs + (unsigned)((it * RING + g + RING) * 256)) & kMask) * 4, 0, 0));
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    float s = 0;
#pragma unroll
    for (int n = 0; n < NT; ++n) s += acc[n][0] + acc[n][1] + acc[n][2] + acc[n][3];
    out[(size_t)blockIdx.x * blockDim.x + tid] = s;
}

template <typename K>
static double time_launch(K launch) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    for (int k = 0; k < 3; ++k) launch();
    hipDeviceSynchronize();
    hipEventRecord(e0);
    const int reps = 40;
    for (int k = 0; k < reps; ++k) launch();
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms;
    hipEventElapsedTime(&ms, e0, e1);
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    return ms / reps;
}

static const double kFlop = 256.0 * 8 * 4096 * 4096.0;          // per launch, every mode

static double report(const char* name, double ms) {
    const double tf = kFlop / (ms * 1e-3) / 1e12;
    printf("%-72s %7.1f us/launch  %6.1f TF\n", name, ms * 1e3, tf);
    return tf;
}

int main() {
    float *out, *wts;
    hipMalloc(&out, sizeof(float) * 512 * 512);
    hipMalloc(&wts, 8 << 20);
    hipMemset(wts, 0, 8 << 20);
    double ref = 0, best16 = 0;
    for (int rep = 0; rep < 2; ++rep) {
        printf("-- pass %d\n", rep);
        ref = report("32x32x2, 2 waves/SIMD, 1 KB / 4 MFMAs, ring 8 (today's main loop)",
                     time_launch([&] { study32<8, 1><<<256, 512>>>(out, wts, 4096 / (4 * 8)); }));
        report("32x32x2, 2 waves/SIMD, no weight loads", time_launch([&] { study32<8, 0><<<256, 512>>>(out, wts, 4096 / (4 * 8)); }));
        report("16x16x4, 4 waves/SIMD, no weight loads, 2 chains",
               time_launch([&] { study16<8, 2, 0><<<512, 512>>>(out, wts, 4096 / (4 * 8)); }));
        double t;
        t = report("16x16x4, 4 waves/SIMD, 1 KB / 4 MFMAs, 2 chains (producer), ring 4",
                   time_launch([&] { study16<4, 2, 1><<<512, 512>>>(out, wts, 4096 / (4 * 4)); }));
        best16 = t > best16 ? t : best16;
        t = report("16x16x4, 4 waves/SIMD, 1 KB / 4 MFMAs, 2 chains (producer), ring 8",
                   time_launch([&] { study16<8, 2, 1><<<512, 512>>>(out, wts, 4096 / (4 * 8)); }));
        best16 = t > best16 ? t : best16;
        t = report("16x16x4, 4 waves/SIMD, 1 KB / 4 MFMAs, 4 chains (consumer), ring 4",
                   time_launch([&] { study16<4, 4, 1><<<512, 512>>>(out, wts, 4096 / (4 * 4)); }));
        best16 = t > best16 ? t : best16;
        t = report("16x16x4, 4 waves/SIMD, 1 KB / 4 MFMAs, 4 chains (consumer), ring 8",
                   time_launch([&] { study16<8, 4, 1><<<512, 512>>>(out, wts, 4096 / (4 * 8)); }));
        best16 = t > best16 ? t : best16;
        t = report("16x16x4, 4 waves/SIMD, 1 KB / 4 MFMAs, 2 chains, ring 4, 496 workgroups",
                   time_launch([&] { study16<4, 2, 1><<<496, 512>>>(out, wts, 4096 / (4 * 4)); }) * 512.0 / 496.0);
    }
    printf("gate G2: best 16x16x4 stream / 32x32x2 stream = %.3f (needs >= 0.94)\n", best16 / ref);
    hipError_t err = hipDeviceSynchronize();
    if (err != hipSuccess) {
        printf("error: %s\n", hipGetErrorString(err));
        return 1;
    }
    return 0;
}
