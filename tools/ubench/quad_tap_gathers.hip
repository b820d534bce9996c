// Micro-benchmark (development aid): what does the texture path charge per wavefront instruction for the tap loads of a dense quad when
// two adjacent pixels SHARE one unaligned 32-bit gather per row (fused_stage_b, G = 4), and what does the fall-back cost?
//   (a) unaligned 32-bit gathers with the address pattern of a warped quad row (lane l around x = 4 l (1 + 1/64) + phase, two rows), next to
//       today's 16-bit gathers at the same addresses;
//   (b) the same 32-bit gather with only 1, 2, 4 or 8 of the 64 lanes active (the lanes whose pair crosses a row of the current image):
//       is a gather under a thin EXEC mask cheaper?  -> decides between a wavefront-level branch and an unconditional second gather;
//   (c) an unaligned 64-bit gather (one load per row for the whole quad).
// Image: one 640 x 480 level (L2-resident), like tap_loads.hip; 8 wavefronts per SIMD; CU-cycles per wavefront instruction at 2.4 GHz.
// One short run (< 1 s of kernels); the process ends itself after 60 s whatever happens.
//   hipcc --offload-arch=gfx950 -O3 tools/ubench/quad_tap_gathers.hip -o tools/ubench/quad_tap_gathers
#include <hip/hip_runtime.h>
#include <unistd.h>
#include <cstdint>
#include <cstdio>
#define ITERS 2048
#define COLS 640
#define ROWS 480

// FORM 0: 16-bit gathers, 1: 32-bit unaligned, 2: 64-bit unaligned; `n_active` lanes of each wavefront execute the loads
template <int FORM>
__global__ __launch_bounds__(256) void k(const uint8_t* __restrict__ img, uint32_t* out, int n_active) {
    const int lane = threadIdx.x & 63, wave = (blockIdx.x * 4 + (threadIdx.x >> 6));
    uint32_t s = 0;
    const bool active = lane % (64 / n_active) == 0;  // n_active (a power of two) lanes, evenly spread
    for (int it = 0; it < ITERS; ++it) {
        const int row = (it * 7 + wave * 3) % (ROWS - 3);
        // a warped quad row: 4 pixels per lane, scale 1 + 1/64, a phase that changes with the iteration; the row drifts by one over 64 lanes
        const int x = (lane * 4 + lane / 16 + (it & 3) + ((wave & 1) ? 256 : 0)) % (COLS - 16);
        const unsigned base = (unsigned)((row + (lane >> 5)) * COLS + x);
        if (active) {
#pragma unroll
            for (int g = 0; g < 4; g += 2) {  // four instructions per iteration in every form
                if (FORM == 0) {
                    uint16_t a, b;
                    __builtin_memcpy(&a, img + base + g, 2);
                    __builtin_memcpy(&b, img + base + COLS + g, 2);
                    s += a + b;
                } else if (FORM == 1) {
                    uint32_t a, b;
                    __builtin_memcpy(&a, img + base + g, 4);
                    __builtin_memcpy(&b, img + base + COLS + g, 4);
                    s += a + b;
                } else {
                    uint64_t a, b;
                    __builtin_memcpy(&a, img + base + 2 * g, 8);
                    __builtin_memcpy(&b, img + base + COLS + 2 * g, 8);
                    s += (uint32_t)a + (uint32_t)(a >> 32) + (uint32_t)b + (uint32_t)(b >> 32);
                }
            }
        }
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <int FORM>
static double run(const char* name, const uint8_t* img, uint32_t* out, int n_active) {
    const int waves_per_simd = 8, blocks = 256 * waves_per_simd;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    hipLaunchKernelGGL(k<FORM>, dim3(blocks), dim3(256), 0, 0, img, out, n_active);
    (void)hipEventRecord(e0);
    hipLaunchKernelGGL(k<FORM>, dim3(blocks), dim3(256), 0, 0, img, out, n_active);
    (void)hipEventRecord(e1);
    if (hipEventSynchronize(e1) != hipSuccess) { printf("%s: launch failed\n", name); _exit(1); }
    float ms;
    (void)hipEventElapsedTime(&ms, e0, e1);
    const double instr_per_cu = (double)waves_per_simd * 4 * ITERS * 4;  // wavefronts per CU x iterations x 4 load instructions
    const double cyc = ms * 1e-3 * 2.4e9 / instr_per_cu;
    printf("%-34s %2d of 64 lanes active: %7.3f ms  %5.1f CU-cycles per load instruction\n", name, n_active, ms, cyc);
    return cyc;
}

int main() {
    alarm(60);
    uint8_t* img;
    uint32_t* out;
    if (hipMalloc(&img, COLS * ROWS + 64) != hipSuccess || hipMalloc(&out, 256 * 8 * 256 * 4) != hipSuccess) return 1;
    (void)hipMemset(img, 7, COLS * ROWS + 64);
    run<0>("16-bit gather (today)", img, out, 64);
    const double c32 = run<1>("(a) 32-bit unaligned gather", img, out, 64);
    for (int n : {8, 4, 2, 1}) run<1>("(b) 32-bit unaligned gather", img, out, n);
    for (int n : {8, 4, 2, 1}) run<0>("(b) 16-bit gather", img, out, n);
    const double c64 = run<2>("(c) 64-bit unaligned gather", img, out, 64);
    printf("64-bit / 32-bit = %.2f\n", c64 / c32);
    return 0;
}
