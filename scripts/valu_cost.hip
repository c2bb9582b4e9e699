// valu_cost.hip -- diagnostic microbenchmark (not part of the product library): what does ONE wave-instruction of the
// stealing trip's instruction mix cost a SIMD of gfx950, and how does that depend on the waves that share the SIMD?
// DESIGN.md section 5 argues from it: "pipes N % busy" charges every VALU instruction a fixed number of cycles, and
// whether that number is 4 or 2 decides whether the headline kernel is bound by its vector pipes or by each wave's own
// issue chain.
//
// Every CU runs W waves per SIMD (W = 1, 2, 4, 6, forced by the block size and by an LDS request that lets exactly the
// wanted number of blocks onto a CU); each wave issues N copies of one instruction with no dependence between neighbours
// (eight live destination registers in turn: a copy depends only on the copy eight instructions earlier) and stamps the
// shader clock before and after.  Reported per
// instruction and W:
//   wave  = cycles between two instructions of the SAME wave (median over the waves),
//   simd  = wave / W = cycles of the SIMD per wave-instruction.
// A pipe-bound instruction keeps `simd` constant as W grows; an issue-bound one keeps `wave` constant.
//
// build: hipcc -O2 --offload-arch=gfx950 scripts/valu_cost.hip -o valu_cost      run: ./valu_cost > table.md
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

typedef float f2 __attribute__((ext_vector_type(2)));

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

enum { OP_FMA, OP_PK_FMA, OP_CVT_SDWA, OP_PERM, OP_CNDMASK, OP_MAX3, OP_MUL_LO, OP_LSHL_ADD, OP_AND_OR, OP_SAVEEXEC, OP_COUNT };
static const char* const kNames[OP_COUNT] = {
    "v_fma_f32", "v_pk_fma_f32", "v_cvt_f32_u32 (SDWA word select)", "v_perm_b32", "v_cndmask_b32 (SGPR-pair mask)",
    "v_max3_f32", "v_mul_lo_u32", "v_lshl_add_u32", "v_and_or_b32", "s_and_saveexec_b64 + s_or_b64 exec (per pair)"};

constexpr int UNROLL = 128;     // instructions (pairs for OP_SAVEEXEC) per loop iteration
constexpr int ITERS = 128;      // loop iterations: 16 384 instructions per wave

// UNROLL copies of one instruction, sixteen rounds over eight destination registers, as ONE asm statement: every destination is an in-out
// operand ("+v": all eight stay live, no copy is dead) and the compiler cannot put anything between the copies -- between
// separate asm statements it pads with s_nop, and it lets dead "=v" outputs share one register, which turns the stream
// into a write-after-write chain on one register with a filler per instruction.  A copy depends only on the copy eight
// instructions earlier.  The timed loops hold nothing but these instructions and the loop's own three scalar ones (check
// with -S: no s_nop inside them).
#define R8_(INS) INS(0) INS(1) INS(2) INS(3) INS(4) INS(5) INS(6) INS(7)
#define R8(INS) R8_(INS) R8_(INS) R8_(INS) R8_(INS) R8_(INS) R8_(INS) R8_(INS) R8_(INS) R8_(INS) R8_(INS) R8_(INS) R8_(INS) R8_(INS) R8_(INS) R8_(INS) R8_(INS)
static_assert(UNROLL == 128, "R8 is sixteen rounds over the eight destinations");
#define OUT8(r) "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7])
#define I_FMA(k) "v_fma_f32 %" #k ", %8, %9, %" #k "\n\t"
#define I_PK_FMA(k) "v_pk_fma_f32 %" #k ", %8, %9, %" #k "\n\t"
#define I_CVT(k) "v_cvt_f32_u32_sdwa %" #k ", %" #k " dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t"
#define I_PERM(k) "v_perm_b32 %" #k ", %" #k ", %8, %9\n\t"
#define I_CNDMASK(k) "v_cndmask_b32_e64 %" #k ", %" #k ", %8, %9\n\t"
#define I_MAX3(k) "v_max3_f32 %" #k ", %8, %9, %" #k "\n\t"
#define I_MUL_LO(k) "v_mul_lo_u32 %" #k ", %" #k ", %8\n\t"
#define I_LSHL_ADD(k) "v_lshl_add_u32 %" #k ", %" #k ", 4, %8\n\t"
#define I_AND_OR(k) "v_and_or_b32 %" #k ", %" #k ", %8, %9\n\t"
#define I_SAVEEXEC(k) "s_and_saveexec_b64 %0, %1\n\ts_or_b64 exec, exec, %0\n\t"
template <int OP>
__device__ __forceinline__ void eight(float (&a)[8], f2 (&p)[8], uint32_t (&u)[8], float x, float y, f2 px, f2 py,
                                      uint32_t i1, uint32_t i2, unsigned long long m) {
    if constexpr (OP == OP_FMA) asm volatile(R8(I_FMA) : OUT8(a) : "v"(x), "v"(y));
    if constexpr (OP == OP_PK_FMA) asm volatile(R8(I_PK_FMA) : OUT8(p) : "v"(px), "v"(py));
    if constexpr (OP == OP_CVT_SDWA) asm volatile(R8(I_CVT) : OUT8(u));
    if constexpr (OP == OP_PERM) asm volatile(R8(I_PERM) : OUT8(u) : "v"(i1), "v"(i2));
    if constexpr (OP == OP_CNDMASK) asm volatile(R8(I_CNDMASK) : OUT8(u) : "v"(i1), "s"(m));
    if constexpr (OP == OP_MAX3) asm volatile(R8(I_MAX3) : OUT8(a) : "v"(x), "v"(y));
    if constexpr (OP == OP_MUL_LO) asm volatile(R8(I_MUL_LO) : OUT8(u) : "v"(i1));
    if constexpr (OP == OP_LSHL_ADD) asm volatile(R8(I_LSHL_ADD) : OUT8(u) : "v"(i1));
    if constexpr (OP == OP_AND_OR) asm volatile(R8(I_AND_OR) : OUT8(u) : "v"(i1), "v"(i2));
    if constexpr (OP == OP_SAVEEXEC) {
        unsigned long long saved;
        // (the mask is all ones: no lane is ever switched off)
        asm volatile(R8(I_SAVEEXEC) : "=&s"(saved) : "s"(m) : "scc");
    }
}

template <int OP>
__global__ void k_cost(long long* __restrict__ cycles, float* __restrict__ sink, int nwaves, float seed) {
    extern __shared__ int32_t pad_lds[];      // only requested: it sets how many blocks fit on a CU
    float a[8];
    f2 p[8];
    uint32_t u[8];
    for (int k = 0; k < 8; k++) {
        a[k] = seed + (float)k;
        p[k] = f2{seed, seed + (float)k};
        u[k] = (uint32_t)k + threadIdx.x * 2654435761u;
    }
    const float x = 1.0f + seed * 1e-7f, y = seed * 1e-9f;
    const f2 px = {x, x}, py = {y, y};
    const uint32_t i1 = 0x01234567u + threadIdx.x, i2 = 0x07060100u;
    const unsigned long long m = ~0ull;
    __syncthreads();                           // the waves of a block start together
    const long long t0 = clock64();
#pragma unroll 1
    for (int it = 0; it < ITERS; it++) {
        eight<OP>(a, p, u, x, y, px, py, i1, i2, m);      // UNROLL instructions
    }
    const long long t1 = clock64();
    float s = 0.f;
    for (int k = 0; k < 8; k++) s += a[k] + p[k].x + p[k].y + (float)u[k];
    const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (wave < nwaves) {
        if ((threadIdx.x & 63) == 0) cycles[wave] = t1 - t0;
        if (s == 12345.678f) sink[wave] = s;  // (never true: keeps the results alive)
    }
}

struct Shape { int waves_per_simd, block, blocks_per_cu; size_t lds; };

template <int OP>
static int run(int ncu, long long* d_cycles, float* d_sink, int cap_waves, double (&wave_cyc)[4]) {
    // 160 KiB of LDS per CU: 96 KiB lets one block on, 64 KiB two
    const Shape shapes[4] = {{1, 256, 1, 96 * 1024}, {2, 512, 1, 96 * 1024}, {4, 1024, 1, 96 * 1024}, {6, 768, 2, 64 * 1024}};
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cost<OP>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    for (int s = 0; s < 4; s++) {
        const Shape& sh = shapes[s];
        const int grid = ncu * sh.blocks_per_cu, nwaves = grid * (sh.block / 64);
        if (nwaves > cap_waves) { fprintf(stderr, "wave buffer too small\n"); return 1; }
        std::vector<long long> h(nwaves);
        double best = 0.0;
        for (int rep = 0; rep < 3; rep++) {   // the first launch warms the clocks up; the last one is reported
            hipLaunchKernelGGL(k_cost<OP>, dim3(grid), dim3(sh.block), sh.lds, 0, d_cycles, d_sink, nwaves, 1.0f);
            CHECK(hipGetLastError());
            CHECK(hipDeviceSynchronize());
            CHECK(hipMemcpy(h.data(), d_cycles, sizeof(long long) * nwaves, hipMemcpyDeviceToHost));
            std::nth_element(h.begin(), h.begin() + nwaves / 2, h.end());
            best = (double)h[nwaves / 2] / ((double)UNROLL * ITERS);
        }
        wave_cyc[s] = best;
    }
    return 0;
}

int main() {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int ncu = prop.multiProcessorCount;
    const int cap_waves = ncu * 2 * 16;
    long long* d_cycles = nullptr;
    float* d_sink = nullptr;
    CHECK(hipMalloc(&d_cycles, sizeof(long long) * cap_waves));
    CHECK(hipMalloc(&d_sink, sizeof(float) * cap_waves));
    printf("# Cycles per wave-instruction on %s (%d CUs), %d independent instructions per wave, every CU loaded\n\n", prop.gcnArchName, ncu, UNROLL * ITERS);
    printf("`wave` = shader-clock cycles between two instructions of one wave (median over the waves); `simd` = wave / W =\n");
    printf("cycles of the SIMD per wave-instruction, at W waves per SIMD.\n\n");
    printf("| instruction | wave W=1 | W=2 | W=4 | W=6 | simd W=1 | W=2 | W=4 | W=6 |\n|---|---|---|---|---|---|---|---|---|\n");
    const int W[4] = {1, 2, 4, 6};
    double c[4];
    int rc = 0;
#define ROW(OP) if (!rc) { rc = run<OP>(ncu, d_cycles, d_sink, cap_waves, c); if (!rc) { printf("| `%s` |", kNames[OP]); \
        for (int s = 0; s < 4; s++) printf(" %.2f |", c[s]); for (int s = 0; s < 4; s++) printf(" %.2f |", c[s] / W[s]); printf("\n"); fflush(stdout); } }
    ROW(OP_FMA) ROW(OP_PK_FMA) ROW(OP_CVT_SDWA) ROW(OP_PERM) ROW(OP_CNDMASK) ROW(OP_MAX3) ROW(OP_MUL_LO) ROW(OP_LSHL_ADD) ROW(OP_AND_OR) ROW(OP_SAVEEXEC)
    (void)hipFree(d_cycles);
    (void)hipFree(d_sink);
    return rc;
}
