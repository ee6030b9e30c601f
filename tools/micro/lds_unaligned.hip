// What a byte-misaligned ds_read_b32 costs on gfx950, against the aligned reads it replaces in the `.count()` kernel's `derive` (gram4_kernels.hip):
// every lane takes the eight bytes from a random byte address e - 3 of a 32 KB LDS buffer (the hit's text) and folds them into a sum, either
//   aligned:   ds_read2_b32 + ds_read_b32 of the three dwords around the bytes, two v_alignbyte_b32 and the address split (the old derive),
//   unaligned: two ds_read_b32 at e - 3 and e + 1 (the new one),
//   rounded:   the same two reads at e - 3 rounded down to a dword (aligned, same pattern of banks: the LDS cost without the misalignment).
// 256 workgroups x 1024 threads, 4096 reads per lane; time by events over the whole grid, best of five.
//   hipcc --offload-arch=gfx950 -O3 -o /tmp/lds_unaligned tools/micro/lds_unaligned.hip && /tmp/lds_unaligned
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>

typedef __attribute__((address_space(3))) const uint32_t lds_a32;
typedef __attribute__((address_space(3), aligned(1))) const uint32_t lds_u32;

constexpr uint32_t kBuf = 32768, kIters = 4096, kTpb = 1024, kBlocks = 256;

template <int MODE>
__global__ __launch_bounds__(kTpb) void probe(uint32_t *out, uint32_t seed) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint32_t *w = reinterpret_cast<uint32_t *>(smem);
    for (uint32_t i = threadIdx.x; i < kBuf / 4; i += blockDim.x) w[i] = i * 0x9E3779B9u + seed;
    __syncthreads();
    uint32_t x = (blockIdx.x * blockDim.x + threadIdx.x) * 0x2545F491u + seed, acc = 0;
    for (uint32_t it = 0; it < kIters; ++it) {
        x = x * 1664525u + 1013904223u;
        const uint32_t e3 = 16u + ((x >> 8) & (kBuf / 2u - 1u));   // byte address of e - 3: [16, kBuf / 2 + 16), the reads stay inside the buffer
        uint32_t lo, t0;
        if (MODE == 0) {
            const uint32_t a0 = e3 & ~3u, sh = e3 & 3u;
            const uint32_t d0 = *reinterpret_cast<lds_a32 *>(static_cast<uintptr_t>(a0));
            const uint32_t d1 = *reinterpret_cast<lds_a32 *>(static_cast<uintptr_t>(a0 + 4u));
            const uint32_t d2 = *reinterpret_cast<lds_a32 *>(static_cast<uintptr_t>(a0 + 8u));
            lo = __builtin_amdgcn_alignbyte(d1, d0, sh);
            t0 = __builtin_amdgcn_alignbyte(d2, d1, sh);
        } else {
            const uint32_t a = MODE == 1 ? e3 : (e3 & ~3u);
            lo = *reinterpret_cast<lds_u32 *>(static_cast<uintptr_t>(a));
            t0 = *reinterpret_cast<lds_u32 *>(static_cast<uintptr_t>(a + 4u));
        }
        acc += lo ^ t0;
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = acc;
}

template <int MODE>
static float run(uint32_t *out, uint32_t seed) {
    hipEvent_t a, b;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    float best = 1e30f;
    for (int rep = 0; rep < 6; ++rep) {
        (void)hipEventRecord(a);
        hipLaunchKernelGGL(probe<MODE>, dim3(kBlocks), dim3(kTpb), kBuf, 0, out, seed);
        (void)hipEventRecord(b);
        (void)hipEventSynchronize(b);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, a, b);
        if (rep) best = ms < best ? ms : best;   // (the first launch warms up)
    }
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return best;
}

int main() {
    uint32_t *out = nullptr;
    if (hipMalloc(&out, sizeof(uint32_t) * kBlocks * kTpb) != hipSuccess) { std::printf("hipMalloc failed\n"); return 1; }
    // the same bytes from every variant: the sums of modes 0 and 1 must agree
    uint32_t *h0 = new uint32_t[kBlocks * kTpb], *h1 = new uint32_t[kBlocks * kTpb];
    const char *name[3] = {"aligned x3 + 2 alignbyte", "unaligned b32 x2", "rounded (aligned) b32 x2"};
    float t[3];
    t[0] = run<0>(out, 7u);
    (void)hipMemcpy(h0, out, sizeof(uint32_t) * kBlocks * kTpb, hipMemcpyDeviceToHost);
    t[1] = run<1>(out, 7u);
    (void)hipMemcpy(h1, out, sizeof(uint32_t) * kBlocks * kTpb, hipMemcpyDeviceToHost);
    t[2] = run<2>(out, 7u);
    if (hipDeviceSynchronize() != hipSuccess) { std::printf("kernel failed\n"); return 1; }
    size_t bad = 0;
    for (uint32_t i = 0; i < kBlocks * kTpb; ++i) bad += h0[i] != h1[i];
    const double lanes = static_cast<double>(kBlocks) * kTpb * kIters;
    for (int m = 0; m < 3; ++m)
        std::printf("%-26s %8.3f ms  %6.2f G lane-reads of 8 bytes/s\n", name[m], t[m], lanes / (t[m] * 1e-3) / 1e9);
    std::printf("aligned vs unaligned sums: %zu mismatches\n", bad);
    delete[] h0;
    delete[] h1;
    (void)hipFree(out);
    return bad != 0;
}
