// Micro-benchmark: what does a ds_read_b32 table look-up cost the LDS array of a CU when its lanes conflict?
//   a. the replicated table of the earlier Buzhash scans: address = byte * 256 + lane * 4 (64 KiB, conflict-free by construction);
//   b. the single-copy table of rotations R[r][v] at r * 1024 + v * 4 (32 KiB, bank = v mod 32), random bytes;
//   c. the same on bytes drawn from the eight values of ONE bank (the worst pattern: up to 8 distinct addresses on a bank).
// Every lane holds 16 look-up addresses (its own random bytes, drawn once) and reads them again and again, 16 loads in flight per wave;
// one workgroup per CU (96 KiB of LDS asked for, so that two cannot share a CU) of 4 or of 16 waves.  The workgroup's shader-clock
// cycles (s_memtime, wave 0) over its look-ups give CU cycles per wave64 look-up; a look-up is served in two groups of 32 lanes.
// Build: hipcc --offload-arch=gfx950 -O3 tools/ubench/lds_table_lookup.hip -o tools/ubench/lds_table_lookup ; run on the GPU box.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <vector>
#define LDS_BYTES (96 * 1024)
#define RD(d, a, o) "ds_read_b32 %" #d ", %" #a " offset:" #o "\n\t"
template <int CASE>
__global__ __launch_bounds__(1024) void k(uint32_t* out, unsigned long long* clk, uint32_t seed, int iters)
{
    extern __shared__ uint32_t smem[];
    for (uint32_t i = threadIdx.x; i < LDS_BYTES / 4; i += blockDim.x)
        smem[i] = i * 2654435761u;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t x = (seed * 0x9e3779b9u) ^ ((blockIdx.x * blockDim.x + threadIdx.x + 1u) * 0x85ebca6bu);
    uint32_t a[16];
#pragma unroll
    for (int i = 0; i < 16; ++i)
    {
        x ^= x << 13, x ^= x >> 17, x ^= x << 5;
        const uint32_t b = CASE == 2 ? ((x >> 9) & 7u) * 32u + 5u : (x >> 9) & 255u;
        a[i] = CASE == 0 ? b * 256u + lane * 4u : b * 4u; // (b, c: the row is the instruction's offset, rows 0, 2, .. 30)
    }
    __syncthreads();
    const unsigned long long c0 = clock64(), w0 = wall_clock64();
    uint32_t acc = 0;
    for (int it = 0; it < iters; ++it)
    {
        uint32_t r0, r1, r2, r3, r4, r5, r6, r7, r8, r9, r10, r11, r12, r13, r14, r15;
#define LO_OUT "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(r4), "=&v"(r5), "=&v"(r6), "=&v"(r7)
#define LO_IN "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7])
#define HI_OUT "=&v"(r8), "=&v"(r9), "=&v"(r10), "=&v"(r11), "=&v"(r12), "=&v"(r13), "=&v"(r14), "=&v"(r15)
#define HI_IN "v"(a[8]), "v"(a[9]), "v"(a[10]), "v"(a[11]), "v"(a[12]), "v"(a[13]), "v"(a[14]), "v"(a[15])
#define TIE "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3), "+v"(r4), "+v"(r5), "+v"(r6), "+v"(r7)
        if (CASE == 0)
        {
            asm volatile(RD(0, 8, 0) RD(1, 9, 0) RD(2, 10, 0) RD(3, 11, 0) RD(4, 12, 0) RD(5, 13, 0) RD(6, 14, 0) RD(7, 15, 0) : LO_OUT : LO_IN : "memory");
            asm volatile(RD(0, 8, 0) RD(1, 9, 0) RD(2, 10, 0) RD(3, 11, 0) RD(4, 12, 0) RD(5, 13, 0) RD(6, 14, 0) RD(7, 15, 0) : HI_OUT : HI_IN : "memory");
        }
        else
        {
            asm volatile(RD(0, 8, 0) RD(1, 9, 2048) RD(2, 10, 4096) RD(3, 11, 6144) RD(4, 12, 8192) RD(5, 13, 10240) RD(6, 14, 12288) RD(7, 15, 14336) : LO_OUT : LO_IN : "memory");
            asm volatile(RD(0, 8, 16384) RD(1, 9, 18432) RD(2, 10, 20480) RD(3, 11, 22528) RD(4, 12, 24576) RD(5, 13, 26624) RD(6, 14, 28672) RD(7, 15, 30720) : HI_OUT : HI_IN : "memory");
        }
        asm volatile("s_waitcnt lgkmcnt(0)" : TIE, "+v"(r8), "+v"(r9), "+v"(r10), "+v"(r11), "+v"(r12), "+v"(r13), "+v"(r14), "+v"(r15)); // all sixteen landed
        acc ^= r0 ^ r1 ^ r2 ^ r3 ^ r4 ^ r5 ^ r6 ^ r7 ^ r8 ^ r9 ^ r10 ^ r11 ^ r12 ^ r13 ^ r14 ^ r15;
    }
    __syncthreads(); // every wave of the workgroup is done
    const unsigned long long c1 = clock64(), w1 = wall_clock64();
    out[blockIdx.x * blockDim.x + threadIdx.x] = acc;
    if (threadIdx.x == 0)
    {
        clk[2 * blockIdx.x] = c1 - c0;
        clk[2 * blockIdx.x + 1] = w1 - w0;
    }
}
template <int CASE> void run(const char* name, int waves, int cus, uint32_t* d, unsigned long long* c)
{
    const int iters = 20000;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k<CASE>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
    k<CASE><<<cus, 64 * waves, LDS_BYTES>>>(d, c, 1, 200); // warm-up
    k<CASE><<<cus, 64 * waves, LDS_BYTES>>>(d, c, 2, iters);
    if (hipDeviceSynchronize() != hipSuccess)
    {
        printf("%s: launch failed\n", name);
        return;
    }
    std::vector<unsigned long long> h(2 * cus);
    (void)hipMemcpy(h.data(), c, sizeof(unsigned long long) * 2 * cus, hipMemcpyDeviceToHost);
    double cyc = 0, wall = 0;
    for (int i = 0; i < cus; ++i)
        cyc += (double)h[2 * i], wall += (double)h[2 * i + 1];
    cyc /= cus, wall /= cus;
    const double lookups = (double)waves * iters * 16; // wave64 look-ups per CU
    printf("%-52s %2d waves/CU: %6.2f CU cycles per wave64 look-up = %5.2f per 32-lane group, %5.3f look-ups per CU cycle (clock %4.0f MHz)\n", name, waves,
           cyc / lookups, cyc / lookups / 2, lookups / cyc, cyc / (wall / 1e8) / 1e6);
}
int main()
{
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0);
    uint32_t* d;
    unsigned long long* c;
    if (hipMalloc(&d, (size_t)cus * 1024 * 4) != hipSuccess || hipMalloc(&c, (size_t)cus * 16) != hipSuccess)
        return 1;
    for (int waves : {4, 16})
    {
        run<0>("a. replicated table (byte, lane): no conflicts", waves, cus, d, c);
        run<1>("b. one copy of R[32][256], random bytes", waves, cus, d, c);
        run<2>("c. one copy of R[32][256], the 8 bytes of one bank", waves, cus, d, c);
    }
    return 0;
}
