// 16 x 16 diagonal-tile inversion (S SPD -> W = L^-1, S = L L'): the blocked matrix-core routine the kernels use (diag16_invert_mfma) against the
// column-per-lane DPP elimination (diag16_invert_dpp) and its packed form (diag16_invert_dpp_packed: S and R in alternate DPP rows of the same registers, the
// one-wave kernel's routine), one wave alone and eight waves per CU (two per SIMD); then max |W L - I| of the three over 64 random SPD tiles, L from a host Cholesky.
// Fourth row: the packed form with 12 pivots (diag16_invert_dpp_packed<12>: the last diagonal tile of a 60-variable QP), on the same tiles with rows and columns
// 12 .. 15 replaced by the identity's -- the padding that routine is promised.  Fifth row: the packed form with a riding panel tile (diag16_invert_dpp_packed<16, true>:
// U = L^-1 B out of the same elimination, in the DPP row that held an unread copy of R): its W against the plain packed routine's bit for bit, its U against a
// host forward substitution in long double.
//   hipcc -O3 --offload-arch=gfx950 -Iinclude -Ig1_locomotion_amd/csrc -o tools/diag_probe tools/diag_probe.hip && tools/diag_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include <cmath>
#include <cstring>
#include "srbdqp.h"
#include "srbdqp_common.hpp"
#include "srbdqp_mfma.hpp"
using namespace srbdqp;
template <int VAR>
__global__ __launch_bounds__(64, 2) void k(const double* A, double* W, long long* cyc, int reps) {
    __shared__ __attribute__((aligned(16))) double tile[PkTile::kDoubles];    // (diag16_invert_dpp uses the first 256; the packed form the S / W and identity tiles of PkTile, the riding form its panel area too: srbdqp_mfma.hpp)
    if constexpr (VAR >= 2) pk_ident_store(tile, threadIdx.x);                // the identity the packed form starts from: once, as the kernel stores it once per pass
    const int lane = threadIdx.x, col = lane & 15, g = lane >> 4;
    v4d s;
    for (int r = 0; r < 4; ++r) s[r] = A[(g + 4 * r) * 16 + col];
    bool ok = true;
    v4d w = s;
    [[maybe_unused]] v4d u = s;
    const long long t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < reps; ++i) {
        v4d in = s;
        in[0] += 1e-30 * w[0];      // dependency between repetitions
        if constexpr (VAR == 4) {   // the riding form: the tile itself as the panel (U = L'), and U feeds the next repetition as W does
            in[0] += 1e-30 * u[0];
            u = s;
            w = diag16_invert_dpp_packed<16, true>(in, lane, ok, tile, &u);
        } else
        if constexpr (VAR == 0) w = diag16_invert_mfma(in, lane, ok);
        else if constexpr (VAR == 1) w = diag16_invert_dpp(in, lane, ok, tile);
        else if constexpr (VAR == 2) w = diag16_invert_dpp_packed(in, lane, ok, tile);
        else w = diag16_invert_dpp_packed<12>(in, lane, ok, tile);
    }
    const long long t1 = __builtin_amdgcn_s_memtime();
    if (blockIdx.x == 0) for (int r = 0; r < 4; ++r) W[(g + 4 * r) * 16 + col] = w[r];
    if constexpr (VAR == 4) { if (blockIdx.x == 0 && u[0] == 12345.678) W[0] = u[0]; }
    if (lane == 0 && blockIdx.x == 0) { cyc[0] = t1 - t0; cyc[1] = ok; }
}
// accuracy: workgroup t inverts tile t
template <int VAR>
__global__ __launch_bounds__(64, 2) void acc(const double* A, double* W, int* okout, [[maybe_unused]] double* U = nullptr) {
    __shared__ __attribute__((aligned(16))) double tile[PkTile::kDoubles];    // (diag16_invert_dpp uses the first 256; the packed form the S / W and identity tiles of PkTile, the riding form its panel area too: srbdqp_mfma.hpp)
    if constexpr (VAR >= 2) pk_ident_store(tile, threadIdx.x);                // the identity the packed form starts from: once, as the kernel stores it once per pass
    const int lane = threadIdx.x, col = lane & 15, g = lane >> 4;
    const double* At = A + 256 * blockIdx.x;
    v4d s;
    for (int r = 0; r < 4; ++r) s[r] = At[(g + 4 * r) * 16 + col];
    bool ok = true;
    v4d w;
    if constexpr (VAR == 0) w = diag16_invert_mfma(s, lane, ok);
    else if constexpr (VAR == 1) w = diag16_invert_dpp(s, lane, ok, tile);
    else if constexpr (VAR == 2) w = diag16_invert_dpp_packed(s, lane, ok, tile);
    else if constexpr (VAR == 4) {                                            // the panel: the next workgroup's tile (the first one's for the last)
        const double* Bt = A + 256 * ((blockIdx.x + 1) % gridDim.x);
        v4d b;
        for (int r = 0; r < 4; ++r) b[r] = Bt[(g + 4 * r) * 16 + col];
        w = diag16_invert_dpp_packed<16, true>(s, lane, ok, tile, &b);
        for (int r = 0; r < 4; ++r) U[256 * blockIdx.x + (g + 4 * r) * 16 + col] = b[r];
    }
    else w = diag16_invert_dpp_packed<12>(s, lane, ok, tile);
    for (int r = 0; r < 4; ++r) W[256 * blockIdx.x + (g + 4 * r) * 16 + col] = w[r];
    if (lane == 0) okout[blockIdx.x] = ok;
}
int main() {
    std::vector<double> A(256), W(256);
    unsigned s = 7; auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xffff) / 65536.0 - 0.5; };
    std::vector<double> G(256); for (auto& v : G) v = rnd();
    for (int i = 0; i < 16; ++i) for (int j = 0; j < 16; ++j) { double a = (i == j) ? 4.0 : 0.0; for (int k2 = 0; k2 < 16; ++k2) a += G[i * 16 + k2] * G[j * 16 + k2]; A[i * 16 + j] = a; }
    auto pad12 = [](double* a) { for (int i = 0; i < 16; ++i) for (int j = 0; j < 16; ++j) if (i >= 12 || j >= 12) a[i * 16 + j] = (i == j) ? 1.0 : 0.0; };
    std::vector<double> Ap(A); pad12(Ap.data());
    double *dA, *dAp, *dW; long long* dc;
    hipMalloc(&dA, 2048); hipMalloc(&dAp, 2048); hipMalloc(&dW, 2048); hipMalloc(&dc, 16);
    hipMemcpy(dA, A.data(), 2048, hipMemcpyHostToDevice);
    hipMemcpy(dAp, Ap.data(), 2048, hipMemcpyHostToDevice);
    const int reps = 1000;
    const char* names[5] = {"diag16_invert_mfma      ", "diag16_invert_dpp       ", "diag16_invert_dpp_packed", "  ... _packed<12 pivots>", "  ... _packed<16, ride> "};
    for (int var = 0; var < 5; ++var) for (int grid : {1, 2048}) {
        const std::vector<double>& Av = var == 3 ? Ap : A;
        for (int it = 0; it < 2; ++it) {
            if (var == 0) hipLaunchKernelGGL(k<0>, dim3(grid), dim3(64), 0, 0, dA, dW, dc, reps);
            else if (var == 1) hipLaunchKernelGGL(k<1>, dim3(grid), dim3(64), 0, 0, dA, dW, dc, reps);
            else if (var == 2) hipLaunchKernelGGL(k<2>, dim3(grid), dim3(64), 0, 0, dA, dW, dc, reps);
            else if (var == 3) hipLaunchKernelGGL(k<3>, dim3(grid), dim3(64), 0, 0, dAp, dW, dc, reps);
            else hipLaunchKernelGGL(k<4>, dim3(grid), dim3(64), 0, 0, dA, dW, dc, reps);
        }
        hipDeviceSynchronize();
        long long c[2]; hipMemcpy(c, dc, 16, hipMemcpyDeviceToHost); hipMemcpy(W.data(), dW, 2048, hipMemcpyDeviceToHost);
        // check W = L^-1: W A W' = I
        double err = 0, up = 0;
        for (int i = 0; i < 16; ++i) for (int j = 0; j < 16; ++j) {
            double v = 0;
            for (int p = 0; p <= i; ++p) for (int q = 0; q <= j; ++q) v += W[i * 16 + p] * Av[p * 16 + q] * W[j * 16 + q];
            err = fmax(err, fabs(v - (i == j ? 1.0 : 0.0)));
            if (j > i) up = fmax(up, fabs(W[i * 16 + j]));
        }
        printf("%s, %4d workgroups (%s): %.0f cycles per 16x16 inversion, ok=%lld, |W A W' - I| = %.2e, max above the diagonal %.1e\n", names[var], grid,
               grid == 1 ? "one wave alone" : "8 waves per CU", (double)c[0] / reps, c[1], err, up);
    }
    // accuracy on NT random SPD tiles (G G' + shift I, the shift from 4 down to 1e-3: condition numbers up to ~1e4)
    const int NT = 64;
    std::vector<double> As(256 * NT), Ls(256 * NT, 0.0), Ws(256 * NT), Aps(256 * NT), Lps(256 * NT, 0.0);
    auto chol = [](const double* a, double* l) {
        for (int j = 0; j < 16; ++j) {
            long double d = a[j * 16 + j]; for (int p = 0; p < j; ++p) d -= (long double)l[j * 16 + p] * l[j * 16 + p];
            l[j * 16 + j] = (double)sqrtl(d);
            for (int i = j + 1; i < 16; ++i) { long double v = a[i * 16 + j]; for (int p = 0; p < j; ++p) v -= (long double)l[i * 16 + p] * l[j * 16 + p]; l[i * 16 + j] = (double)(v / l[j * 16 + j]); }
        }
    };
    for (int t = 0; t < NT; ++t) {
        const double shift = 4.0 * pow(10.0, -3.6 * t / (NT - 1));
        for (auto& v : G) v = rnd();
        double* a = &As[256 * t]; double* l = &Ls[256 * t];
        for (int i = 0; i < 16; ++i) for (int j = 0; j < 16; ++j) { double v = (i == j) ? shift : 0.0; for (int k2 = 0; k2 < 16; ++k2) v += G[i * 16 + k2] * G[j * 16 + k2]; a[i * 16 + j] = v; }
        chol(a, l);
        for (int e = 0; e < 256; ++e) Aps[256 * t + e] = a[e];
        pad12(&Aps[256 * t]);
        chol(&Aps[256 * t], &Lps[256 * t]);
    }
    double *dAs, *dAps, *dWs; int* dok;
    hipMalloc(&dAs, 2048 * NT); hipMalloc(&dAps, 2048 * NT); hipMalloc(&dWs, 2048 * NT); hipMalloc(&dok, 4 * NT);
    hipMemcpy(dAs, As.data(), 2048 * NT, hipMemcpyHostToDevice);
    hipMemcpy(dAps, Aps.data(), 2048 * NT, hipMemcpyHostToDevice);
    std::vector<double> Wfull(256 * NT);                      // W of the full packed routine on the PADDED tiles: the 12-pivot routine must return its bits
    for (int var = 0; var < 5; ++var) {
        const std::vector<double>& Lv = var >= 3 ? Lps : Ls;
        if (var == 0) hipLaunchKernelGGL(acc<0>, dim3(NT), dim3(64), 0, 0, dAs, dWs, dok);
        else if (var == 1) hipLaunchKernelGGL(acc<1>, dim3(NT), dim3(64), 0, 0, dAs, dWs, dok);
        else if (var == 2) hipLaunchKernelGGL(acc<2>, dim3(NT), dim3(64), 0, 0, dAs, dWs, dok);
        else if (var == 3) hipLaunchKernelGGL(acc<2>, dim3(NT), dim3(64), 0, 0, dAps, dWs, dok);
        else hipLaunchKernelGGL(acc<3>, dim3(NT), dim3(64), 0, 0, dAps, dWs, dok);
        hipDeviceSynchronize();
        std::vector<int> oks(NT);
        hipMemcpy(Ws.data(), dWs, 2048 * NT, hipMemcpyDeviceToHost); hipMemcpy(oks.data(), dok, 4 * NT, hipMemcpyDeviceToHost);
        double err = 0; int nok = 0;
        for (int t = 0; t < NT; ++t) {
            nok += oks[t];
            for (int i = 0; i < 16; ++i) for (int j = 0; j <= i; ++j) {   // (W L is lower triangular: the routines' entries above the diagonal are not part of W)
                long double v = 0;
                for (int p = j; p <= i; ++p) v += (long double)Ws[256 * t + i * 16 + p] * Lv[256 * t + p * 16 + j];
                err = fmax(err, fabs((double)v - (i == j ? 1.0 : 0.0)));
            }
        }
        if (var == 3) { Wfull = Ws; continue; }
        printf("%s: max |W L - I| over %d random SPD tiles = %.3e, ok on %d", names[var == 4 ? 3 : var], NT, err, nok);
        if (var == 4) {
            int diff = 0;
            for (int e = 0; e < 256 * NT; ++e) diff += memcmp(&Ws[e], &Wfull[e], 8) != 0;
            printf("  (padded tiles; entries whose bits differ from the 16-pivot routine's on the same tiles: %d of %d)", diff, 256 * NT);
        }
        printf("\n");
    }
    // the riding form: W against the plain packed routine's on the same tiles, U = L^-1 B (B: the next tile) against forward substitution in long double
    {
        std::vector<double> Wp(256 * NT), Us(256 * NT);
        double* dUs; hipMalloc(&dUs, 2048 * NT);
        hipLaunchKernelGGL(acc<2>, dim3(NT), dim3(64), 0, 0, dAs, dWs, dok, (double*)nullptr);
        hipDeviceSynchronize();
        hipMemcpy(Wp.data(), dWs, 2048 * NT, hipMemcpyDeviceToHost);
        hipLaunchKernelGGL(acc<4>, dim3(NT), dim3(64), 0, 0, dAs, dWs, dok, dUs);
        hipDeviceSynchronize();
        std::vector<int> oks(NT);
        hipMemcpy(Ws.data(), dWs, 2048 * NT, hipMemcpyDeviceToHost); hipMemcpy(Us.data(), dUs, 2048 * NT, hipMemcpyDeviceToHost); hipMemcpy(oks.data(), dok, 4 * NT, hipMemcpyDeviceToHost);
        int diff = 0, nok = 0;
        for (int e = 0; e < 256 * NT; ++e) diff += memcmp(&Ws[e], &Wp[e], 8) != 0;
        double err = 0;
        for (int t = 0; t < NT; ++t) {
            nok += oks[t];
            const double* l = &Ls[256 * t]; const double* b = &As[256 * ((t + 1) % NT)];
            long double u[256]; double top = 0;
            for (int i = 0; i < 16; ++i) for (int c = 0; c < 16; ++c) {
                long double v = b[i * 16 + c];
                for (int p = 0; p < i; ++p) v -= (long double)l[i * 16 + p] * u[p * 16 + c];
                u[i * 16 + c] = v / l[i * 16 + i];
                top = fmax(top, fabs((double)u[i * 16 + c]));
            }
            for (int e = 0; e < 256; ++e) err = fmax(err, fabs((double)(Us[256 * t + e] - u[e])) / top);
        }
        printf("%s: W entries whose bits differ from the plain packed routine's: %d of %d; max |U - L^-1 B| / max |U| over %d tiles = %.3e, ok on %d\n", names[4], diff, 256 * NT, NT, err, nok);
    }
    return 0;
}
