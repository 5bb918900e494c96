// Where do the workgroups of a launch land, and when do they end?  A stand-in kernel with the launch shape of k_match_lds (grid (4, 255),
// 256 threads, 8320 B of static LDS) or k_tv_hyp (grid (16, 255), 256 threads) does a FIXED amount of vector work per workgroup (the
// matcher's mix: 8 v_xor + 8 v_bcnt + 3 key instructions per trip and query, two queries per lane), so a CU that holds more workgroups than
// its neighbours takes longer, as the real kernel would.  Every workgroup records the XCD, shader engine and CU it ran on (hardware-id
// registers) and the 100 MHz wall clock at entry and exit.  Printed per configuration: the launch's duration, the histogram of workgroups
// per CU, the totals per shader engine and per XCD, and the spread of the end times.  The same total work is then cut into S = 2, 4, 8
// slices (grid.z = S, 1/S of the trips each), repeated with the LDS raised above 32 KB (at most 4 workgroups per CU), and repeated with
// the wavefronts lowering their priority (s_setprio 3 .. 0) from quarter to quarter of their trips, as k_match_lds does per tile.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

struct Rec { uint32_t xcc, hwid; unsigned long long t0, t1; };

template <int LDS, bool PRIO> __global__ __launch_bounds__(256) void k_probe(Rec* rec, uint32_t* sink, int trips) {
    __shared__ uint32_t s[LDS / 4];
    const int wg = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    const unsigned long long t0 = wall_clock64();
    s[threadIdx.x % (LDS / 4)] = threadIdx.x;
    __syncthreads();
    uint32_t a[2][8], k0[2] = {~0u, ~0u}, k1[2] = {~0u, ~0u};
    for (int m = 0; m < 2; m++)
        for (int k = 0; k < 8; k++) a[m][k] = (threadIdx.x + 1) * 2654435761u + k * 40503u + m + s[(threadIdx.x + k) % (LDS / 4)];
    for (int j = 0; j < trips; j++) {
        if (PRIO && (j & 7) == 0) {  // the priority falls with the quarter of its trips a wavefront is in: whoever is ahead yields
            if (j * 4 < trips) __builtin_amdgcn_s_setprio(3);
            else if (j * 4 < 2 * trips) __builtin_amdgcn_s_setprio(2);
            else if (j * 4 < 3 * trips) __builtin_amdgcn_s_setprio(1);
            else __builtin_amdgcn_s_setprio(0);
        }
        uint32_t b[8];
        for (int k = 0; k < 8; k++) b[k] = __builtin_amdgcn_readfirstlane(a[0][k]) + j * (2 * k + 1);  // wave-uniform, like a broadcast LDS read
#pragma unroll
        for (int m = 0; m < 2; m++) {
            uint32_t d = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) asm volatile("v_bcnt_u32_b32 %0, %1, %2" : "=v"(d) : "v"(a[m][k] ^ b[k]), "v"(d));
            const uint32_t key = (d << 20) | (uint32_t)j;
            uint32_t med;
            asm volatile("v_med3_u32 %0, %1, %2, %3" : "=v"(med) : "v"(k0[m]), "v"(k1[m]), "v"(key));
            k1[m] = med;
            k0[m] = min(k0[m], key);
        }
    }
    if (k0[0] + k1[0] + k0[1] + k1[1] == 0x12345678u) sink[threadIdx.x] = k0[0];  // keeps the work alive; never true in practice
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t xcc, hwid;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
        Rec r;
        r.xcc = xcc & 15u; r.hwid = hwid; r.t0 = t0; r.t1 = wall_clock64();
        rec[wg] = r;
    }
}

template <int LDS, bool PRIO = false> static void run(const char* what, dim3 grid, int trips, Rec* d_rec, uint32_t* d_sink) {
    const int n = grid.x * grid.y * grid.z;
    std::vector<Rec> h(n);
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    hipLaunchKernelGGL((k_probe<LDS, PRIO>), grid, dim3(256), 0, 0, d_rec, d_sink, trips);  // loads the code object, warms the clocks
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(a, 0));
    hipLaunchKernelGGL((k_probe<LDS, PRIO>), grid, dim3(256), 0, 0, d_rec, d_sink, trips);
    CK(hipEventRecord(b, 0)); CK(hipEventSynchronize(b));
    float ms; CK(hipEventElapsedTime(&ms, a, b));
    CK(hipMemcpy(h.data(), d_rec, n * sizeof(Rec), hipMemcpyDeviceToHost));
    // HW_ID (gfx9): cu_id [11:8], sh_id [12], se_id [15:13]; a CU is named by (xcc, se, sh, cu)
    std::map<uint32_t, int> per_cu, per_se, per_xcc;
    std::map<uint32_t, unsigned long long> cu_end;
    unsigned long long first = ~0ull, last = 0;
    for (const Rec& r : h) first = std::min(first, r.t0), last = std::max(last, r.t1);
    std::vector<double> end_us, len_us;
    for (const Rec& r : h) {
        const uint32_t cu = (r.xcc << 8) | ((r.hwid >> 8) & 0xFFu), se = (r.xcc << 4) | ((r.hwid >> 13) & 7u);
        per_cu[cu]++; per_se[se]++; per_xcc[r.xcc]++;
        cu_end[cu] = std::max(cu_end[cu], r.t1 - first);
        end_us.push_back((r.t1 - first) * 0.01); len_us.push_back((r.t1 - r.t0) * 0.01);
    }
    std::sort(end_us.begin(), end_us.end()); std::sort(len_us.begin(), len_us.end());
    std::map<int, int> hist;
    for (auto& kv : per_cu) hist[kv.second]++;
    std::vector<double> ce;
    for (auto& kv : cu_end) ce.push_back(kv.second * 0.01);
    std::sort(ce.begin(), ce.end());
    printf("== %s: grid (%u, %u, %u) lds %d trips %d: %d workgroups, launch %.1f us, first entry to last exit %.1f us\n", what, grid.x, grid.y,
           grid.z, LDS, trips, n, ms * 1e3, (last - first) * 0.01);
    printf("   CUs seen %zu; workgroups per CU -> number of CUs:", per_cu.size());
    for (auto& kv : hist) printf("  %d: %d", kv.first, kv.second);
    printf("\n   per XCD:");
    for (auto& kv : per_xcc) printf(" %d", kv.second);
    printf("\n   per shader engine (xcd.se):");
    for (auto& kv : per_se) printf(" %u.%u=%d", kv.first >> 4, kv.first & 15u, kv.second);
    printf("\n   CUs per shader engine:");
    std::map<uint32_t, int> cus_in_se;
    for (auto& kv : per_cu) cus_in_se[((kv.first >> 8) << 4) | ((kv.first >> 5) & 7u)]++;
    for (auto& kv : cus_in_se) printf(" %u.%u=%d", kv.first >> 4, kv.first & 15u, kv.second);
    printf("\n   workgroup length us: min %.1f median %.1f max %.1f;  workgroup end us: min %.1f median %.1f max %.1f\n", len_us.front(),
           len_us[n / 2], len_us.back(), end_us.front(), end_us[n / 2], end_us.back());
    printf("   last exit per CU us: min %.1f p10 %.1f median %.1f p90 %.1f max %.1f  (max / median %.3f)\n", ce.front(), ce[ce.size() / 10],
           ce[ce.size() / 2], ce[ce.size() * 9 / 10], ce.back(), ce.back() / ce[ce.size() / 2]);
    CK(hipEventDestroy(a)); CK(hipEventDestroy(b));
}

int main(int argc, char** argv) {
    const int trips = argc > 1 ? atoi(argv[1]) : 400;  // 400 trips x 38 vector instructions: about 0.1 ms at 4 wavefronts per SIMD
    const int max_wg = 16 * 255 * 8;
    Rec* d_rec; uint32_t* d_sink;
    CK(hipMalloc(&d_rec, max_wg * sizeof(Rec))); CK(hipMalloc(&d_sink, 256 * sizeof(uint32_t)));
    for (int s : {1, 2, 4, 8}) run<8320>("matcher shape", dim3(4, 255, s), trips / s, d_rec, d_sink);
    for (int s : {1, 2, 4, 8}) run<33792>("matcher shape, at most 4 workgroups per CU", dim3(4, 255, s), trips / s, d_rec, d_sink);
    for (int s : {1, 2, 4}) run<8320, true>("matcher shape, priority falling with progress", dim3(4, 255, s), trips / s, d_rec, d_sink);
    run<64>("k_tv_hyp shape", dim3(16, 255, 1), trips / 2, d_rec, d_sink);
    run<64>("k_tv_hyp shape, blocks half as long", dim3(32, 255, 1), trips / 4, d_rec, d_sink);
    CK(hipFree(d_rec)); CK(hipFree(d_sink));
    return 0;
}
