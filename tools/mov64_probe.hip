// What a 64-bit register copy costs the issue pipe on gfx950: a stream of 64 independent v_mov_b64 against the same number of v_mov_b32 (and, for scale, of
// v_mov_b32 PAIRS: what copying a double costs 32 bits at a time), one wave alone on its SIMD and two waves per SIMD, five repeats each.  The row swaps of the one-wave
// kernel (pk_even_rows, srbdqp_mfma.hpp; row_chunks(double), srbdqp_admm.hpp) copy doubles before every v_permlane*_swap: one v_mov_b64 replaces two v_mov_b32 only if
// it issues like ONE of them.
//   hipcc -O3 --offload-arch=gfx950 -Wno-unused-value -o tools/mov64_probe tools/mov64_probe.hip && tools/mov64_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#define M64(D, E, S, T) "v_mov_b64 v[" #D ":" #E "], v[" #S ":" #T "]\n\t"
#define M32(D, E, S, T) "v_mov_b32 v" #D ", v" #S "\n\t"
#define M32P(D, E, S, T) "v_mov_b32 v" #D ", v" #S "\n\tv_mov_b32 v" #E ", v" #T "\n\t"
#define ROW8(M) M(16, 17, 0, 1) M(18, 19, 2, 3) M(20, 21, 4, 5) M(22, 23, 6, 7) M(24, 25, 8, 9) M(26, 27, 10, 11) M(28, 29, 12, 13) M(30, 31, 14, 15)
#define ROW64(M) ROW8(M) ROW8(M) ROW8(M) ROW8(M) ROW8(M) ROW8(M) ROW8(M) ROW8(M)
#define CLOB "v0", "v1", "v2", "v3", "v4", "v5", "v6", "v7", "v8", "v9", "v10", "v11", "v12", "v13", "v14", "v15", "v16", "v17", "v18", "v19", "v20", "v21", "v22", "v23", "v24", \
             "v25", "v26", "v27", "v28", "v29", "v30", "v31"
// VAR 0: 64 v_mov_b64; 1: 64 v_mov_b32; 2: 64 pairs of v_mov_b32 -- per trip of the loop, sources v0 .. v15 never written: every move is independent
template <int VAR>
__global__ __launch_bounds__(64, 2) void k(long long* cyc, int reps) {
    const long long t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < reps; ++i) {
        if constexpr (VAR == 0) asm volatile(ROW64(M64) ::: CLOB);
        else if constexpr (VAR == 1) asm volatile(ROW64(M32) ::: CLOB);
        else asm volatile(ROW64(M32P) ::: CLOB);
    }
    const long long t1 = __builtin_amdgcn_s_memtime();
    if (threadIdx.x == 0 && blockIdx.x == 0) cyc[0] = t1 - t0;
}
int main() {
    long long* c; hipMalloc(&c, 8);
    const int reps = 2000;
    const char* names[3] = {"v_mov_b64          ", "v_mov_b32          ", "two v_mov_b32      "};
    for (int grid : {1, 2048}) {
        for (int var = 0; var < 3; ++var) {
            printf("%s, %s:", names[var], grid == 1 ? "one wave alone      " : "two waves per SIMD  ");
            for (int rep = 0; rep < 6; ++rep) {       // (the first launch of each is the warm-up: not printed)
                if (var == 0) hipLaunchKernelGGL(k<0>, dim3(grid), dim3(64), 0, 0, c, reps);
                else if (var == 1) hipLaunchKernelGGL(k<1>, dim3(grid), dim3(64), 0, 0, c, reps);
                else hipLaunchKernelGGL(k<2>, dim3(grid), dim3(64), 0, 0, c, reps);
                hipDeviceSynchronize();
                long long h; hipMemcpy(&h, c, 8, hipMemcpyDeviceToHost);
                if (rep) printf(" %.3f", (double)h / reps / 64);
            }
            printf("   cycles of the s_memtime clock per copy\n");
        }
    }
    return 0;
}
