// srbdqp_mfma.hpp -- the fp64 matrix-core building blocks shared by every kernel of the engine (the round-1 kernel "v1"
// that introduced them -- all 12N variables, packed G + GᵀG on the matrix cores -- is retired; its phases live on in
// srbdqp_compact.hpp / srbdqp_setup1.hpp / srbdqp_wrench.hpp on the presolved problems).
//
// All dense n x n work is 16x16 tiles on v_mfma_f64_16x16x4_f64:
//
//   H  : K = G'G (+ R s^2 + sigma + A' rho A on the diagonal), G = Q^1/2 s B_qp packed block-lower in LDS; the 36
//        upper tiles (n = 120 -> 8x8 tiles) accumulate in registers, 9 tiles per wave.          [a7, MFMA contraction]
//   F  : right-looking Cholesky K = U'U with the trailing tiles resident in registers; per block column one wave
//        factors and inverts the 16x16 diagonal tile (diag16_invert_mfma: blocked 4x4, on the matrix cores), the
//        panel is L_jj^-1 K_jb and the trailing update K_ab -= U_ja' U_jb.                          [a9 factor]
//   W  : W = L^-1 row by row, in place over U (W_ij = -W_ii sum_k L_ik W_kj).
//   I  : K^-1 = W'W, tiles swizzled into LDS, then every thread pulls its row fragment of K^-1 into registers.
//   ADMM: shared admm_loop() -- the two triangular solves of each iteration are applied as one mat-vec with the
//        explicit inverse (depth-1 instead of depth-n substitution).                              [a9 iterations]
//
// Register tiles are in the MFMA C/D layout (lane l: column l&15, rows (l>>4)+4r, r = 0..3).  Register r of a
// C-layout tile is exactly the B operand of K-step r of a product that contracts over the tile's ROW index, so
// chains of tile products (panel, W rows) never leave the register file.  LDS tiles are row-major 16x16; tiles that
// are read both along rows and along columns (the diagonal inverses, the final K^-1) are XOR-swizzled
// (col ^ row), which makes both access directions bank-conflict free.
#pragma once
#include "srbdqp_common.hpp"
#include "srbdqp_admm.hpp"

namespace srbdqp {

constexpr bool kMfmaReady = true;

#ifdef SRBDQP_PROFILE_F
#define F_T(var) do { unsigned long long t_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); var = (long long)t_; } while (0)
#else
#define F_T(var) do { } while (0)
#endif

typedef double v4d __attribute__((ext_vector_type(4)));

__device__ __forceinline__ v4d mfma_f64(double a, double b, v4d c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ double readlane_f64(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// index of upper tile (a, b), a <= b
__device__ __forceinline__ int tile_id(int a, int b) { return (b * (b + 1)) / 2 + a; }

// C-layout register tile -> LDS tile (row-major; swizzled: col ^ row)
template <bool SWZ>
__device__ __forceinline__ void store_tile(double* tile, const v4d& v, int lane) {
    const int col = lane & 15, g = lane >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = g + 4 * r;
        tile[row * 16 + (SWZ ? (col ^ row) : col)] = v[r];
    }
}

// the same two for either tile type (the general kernel, srbdqp_wrench.hpp: fp64 tiles on v_mfma_f64_16x16x4_f64, fp32 tiles on v_mfma_f32_16x16x4_f32)
typedef float v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ v4d mma16(double a, double b, v4d c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
__device__ __forceinline__ v4f mma16(float a, float b, v4f c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
// row of accumulator register q in the MFMA C/D layout: fp64 16x16x4: (lane >> 4) + 4 q; fp32 16x16x4: 4 (lane >> 4) + q
template <typename TT> __device__ __forceinline__ int crow(int kq, int q) { return (sizeof(TT) == 8) ? kq + 4 * q : 4 * kq + q; }
template <typename TT, bool SWZ, typename V4>
__device__ __forceinline__ void store_tile_t(TT* tile, const V4& v, int lane) {
    const int col = lane & 15, g = lane >> 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = crow<TT>(g, q);
        tile[row * 16 + (SWZ ? (col ^ row) : col)] = v[q];
    }
}

// 1/sqrt(d) of a positive, normal pivot: v_rsq_f64 seed + ONE Newton step.  Measured on gfx950 (tools/rsq_probe.hip, 4 M random
// doubles over 40 binades): seed 5.2e-8 relative, one step 4.1e-15, two steps 1.4e-16 -- the second step (four more dependent
// fp64 instructions per pivot, 16 pivots per diagonal tile, on the critical path of every factorisation) bought nothing the
// ADMM can see: K^-1 is applied to right-hand sides that are themselves only converged to 1e-6.
__device__ __forceinline__ double fast_rsqrt(double d) {
    const double r = __builtin_amdgcn_rsq(d);
    const double h = 0.5 * d * r;
    return fma(r, fma(-h, r, 0.5), r);
}

// ... with the second Newton step (1.4e-16 relative): the 6 x 6 wrench blocks E of the general kernel, whose inverse enters T and
// V at full weight (the assembly parity tests hold both to 1e-11).  Still a fifth of the instructions of 1.0 / sqrt(d).
__device__ __forceinline__ double fast_rsqrt2(double d) {
    double r = __builtin_amdgcn_rsq(d);
    double h = 0.5 * d * r;
    r = fma(r, fma(-h, r, 0.5), r);
    h = 0.5 * d * r;
    return fma(r, fma(-h, r, 0.5), r);
}

// ---------------------------------------------------------------------------------------------------------
// 16x16 diagonal tile, blocked on the matrix cores: S (SPD, C-layout register tile) -> W = L^-1 (C layout), S = L L'.
// One wave, nothing leaves the register file.  Row block kb (4 rows) of a C-layout tile is register kb; kept as the
// UPPER factor U = L', register kb is at once the A operand (A[i][k] = L[i][4kb+k]) and the B operand
// (B[k][j] = U[4kb+k][j]) of the rank-4 products, so per block the work is
//   - 10 v_readlane pairs broadcast the 4x4 diagonal block; every lane factors it and inverts the factor (4 rsqrt),
//   - U_kb = L_kk^-1 S_kb              one MFMA (L_kk^-1 repeated in every row block of the A operand; accumulator register kb is the result),
//   - S   -= U_kb' U_kb                one MFMA (trailing update of the whole tile),
//   - W_kb = L_kk^-1 R_kb, R -= L[:,kb] W_kb   two MFMAs (block forward substitution L W = I riding along),
// 14 MFMAs and ~350 other instructions per tile (a row-by-row LDL' elimination with v_readlane broadcasts, the first
// version of this routine, took ~1000 and twice the time).
// ---------------------------------------------------------------------------------------------------------
template <int KB>
__device__ __forceinline__ void diag16_block(v4d& s, v4d& rr, v4d& w, double& pmin, int lane) {
    const int col = lane & 15, k = lane >> 4, li = col & 3;
    const double sk = s[KB];
    // diagonal block D[g][c] = S[4KB+g][4KB+c] sits in lane 16 g + 4KB + c of register KB
    const double d00 = readlane_f64(sk, 4 * KB), d01 = readlane_f64(sk, 4 * KB + 1), d02 = readlane_f64(sk, 4 * KB + 2), d03 = readlane_f64(sk, 4 * KB + 3);
    const double d11 = readlane_f64(sk, 16 + 4 * KB + 1), d12 = readlane_f64(sk, 16 + 4 * KB + 2), d13 = readlane_f64(sk, 16 + 4 * KB + 3);
    const double d22 = readlane_f64(sk, 32 + 4 * KB + 2), d23 = readlane_f64(sk, 32 + 4 * KB + 3);
    const double d33 = readlane_f64(sk, 48 + 4 * KB + 3);
    // D = R'R (R upper), X = R^-1
    const double x00 = fast_rsqrt(d00);
    const double r01 = d01 * x00, r02 = d02 * x00, r03 = d03 * x00;
    const double p1 = fma(-r01, r01, d11);
    const double x11 = fast_rsqrt(p1);
    const double r12 = fma(-r01, r02, d12) * x11, r13 = fma(-r01, r03, d13) * x11;
    const double p2 = fma(-r12, r12, fma(-r02, r02, d22));
    const double x22 = fast_rsqrt(p2);
    const double r23 = fma(-r12, r13, fma(-r02, r03, d23)) * x22;
    const double p3 = fma(-r23, r23, fma(-r13, r13, fma(-r03, r03, d33)));
    const double x33 = fast_rsqrt(p3);
    pmin = (d00 > 0.0 && p1 > 0.0 && p2 > 0.0 && p3 > 0.0) ? pmin : -1.0;   // (a NaN pivot fails the comparison too)
    const double x01 = -x00 * r01 * x11;
    const double x12 = -x11 * r12 * x22;
    const double x23 = -x22 * r23 * x33;
    const double x02 = -fma(x00, r02, x01 * r12) * x22;
    const double x13 = -fma(x11, r13, x12 * r23) * x33;
    const double x03 = -fma(x00, r03, fma(x01, r13, x02 * r23)) * x33;
    // A operand: lane (i = col, k): L_kk^-1[i - 4KB][k] = X[k][i - 4KB] for rows i of this block, k <= i - 4KB; else 0
    const double c0 = x00;                                              // li = 0: k = 0
    const double c1 = (k == 0) ? x01 : x11;                             // li = 1: k = 0, 1
    const double c2 = (k == 0) ? x02 : (k == 1) ? x12 : x22;            // li = 2
    const double c3 = (k == 0) ? x03 : (k == 1) ? x13 : (k == 2) ? x23 : x33;
    double a = (li == 0) ? c0 : (li == 1) ? c1 : (li == 2) ? c2 : c3;
    a = (k <= li) ? a : 0.0;   // (the same 4 x 4 block in every row block of the operand: only accumulator register KB -- rows 4 KB .. 4 KB + 3 -- of the two products is read)
    const v4d zero = (v4d){0.0, 0.0, 0.0, 0.0};
    double u = mfma_f64(a, sk, zero)[KB];                               // U_kb = L_kk^-1 S_kb
    u = (col >= 4 * KB) ? u : 0.0;                                      // columns left of the block: exact zeros
    const double wk = mfma_f64(a, rr[KB], zero)[KB];                    // W_kb = L_kk^-1 R_kb
    w[KB] = wk;
    if constexpr (KB < 3) {
        s = mfma_f64(-u, u, s);                                         // S -= U_kb' U_kb
        const double am = (col >= 4 * (KB + 1)) ? u : 0.0;              // L[i][4KB + k] for the rows below the block
        rr = mfma_f64(-am, wk, rr);                                     // R -= L[:, kb] W_kb
        diag16_block<KB + 1>(s, rr, w, pmin, lane);
    }
}

// returns W = L^-1 in C layout (entries above the diagonal are rounding-level garbage: consumers mask them);
// ok = every pivot positive
__device__ __forceinline__ v4d diag16_invert_mfma(v4d s, int lane, bool& ok) {
    const int col = lane & 15, g = lane >> 4;
    v4d rr, w;
#pragma unroll
    for (int r = 0; r < 4; ++r) { rr[r] = (g + 4 * r == col) ? 1.0 : 0.0; w[r] = 0.0; }
    double pmin = 1.0e300;
    diag16_block<0>(s, rr, w, pmin, lane);
    ok = pmin > 0.0;
    return w;
}


// ---------------------------------------------------------------------------------------------------------
// The same inversion without the matrix cores and without v_readlane: one COLUMN per lane.  Lane c of every 16-lane DPP row holds column c of S
// (16 registers S_i = S[i][c]) and of R (R_i, the identity at the start).  Pivot k: d = S[k][k] is a row_newbcast of register S_k, u = S_k / sqrt(d)
// is row k of L' (own lane: L[c][k]), W_k = R_k / sqrt(d) is row k of L^-1, and every row below takes ONE DPP multiply-add per matrix,
//     S_i -= L[i][k] u,   R_i -= L[i][k] W_k     with L[i][k] = u in lane i = the instruction's row_newbcast:i source operand,
// 240 v_fmac_f64_dpp + 16 x 9 instructions of pivot chain (the next pivot's chain depends on the first multiply-add of a pivot only: the
// scheduler runs it beside the rest).  The blocked routine above is as many instructions but spends half its time waiting on dependent MFMAs and
// on v_readlane hazards: 3309 cycles a tile alone on its SIMD against 2888 here, 3571 against 2961 with two waves per SIMD (tools/diag_probe.hip; a DPP
// multiply-add of doubles issues every 8 cycles from one wave alone).  In and out through a 16 x 16 LDS tile of the caller's (C layout -> columns; W back
// row-major, XOR-swizzled as the consumers read it); the four DPP rows work redundantly.  Used by the general kernel and by the 4-wave kernel's batch-1
// instantiation (N = 10 double support 14.75 -> 14.99 M QP/s, configs[4] 2.83 -> 2.88 M, the batch-1 call -0.8 us); NOT by the one-wave kernel: its 64 live
// registers beside that kernel's ten register tiles end in scratch memory (256 VGPRs + 88 bytes; configs[1] at 35 fixed iterations 1.775 -> 1.852 ms per 65,536 QPs).
// (The one-wave kernel runs the PACKED form further down, diag16_invert_dpp_packed: half the registers.)
// ---------------------------------------------------------------------------------------------------------
template <int I>
__device__ __forceinline__ void fmac_newbcast(double& acc, double nu, double m) {   // acc += nu[lane I of the row] * m
    asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(nu), "v"(m), "n"(I));
}
template <int K>
__device__ __forceinline__ double mov_newbcast(double v) {   // (the source may come out of one of the asm statements above, which the hazard recognizer does not see into: the two wait states by hand)
    double d;
    asm("s_nop 1\n\tv_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(d) : "v"(v), "n"(K));
    return d;
}
template <int K, int I>
struct Diag16Rows {
    static __device__ __forceinline__ void run(double (&S)[16], double (&R)[16], double nu, double u, double wk) {
        if constexpr (I < 16) {
            fmac_newbcast<I>(S[I], nu, u);
            fmac_newbcast<I>(R[I], nu, wk);
            Diag16Rows<K, I + 1>::run(S, R, nu, u, wk);
        }
    }
};
// pivots K .. KEND - 1 (KEND = 16: the whole tile; the low-latency general kernel runs the tile in two halves around a workgroup barrier)
template <int K, int KEND = 16>
__device__ __forceinline__ void diag16_pivot(double (&S)[16], double (&R)[16], bool& ok) {
    const double d = mov_newbcast<K>(S[K]);
    ok = ok && (d > 0.0);                         // (a NaN pivot fails the comparison too)
    const double r = fast_rsqrt(d);
    const double u = S[K] * r;
    const double wk = R[K] * r;
    R[K] = wk;
    if constexpr (K < 15) {
        double nu;
        asm("v_mul_f64 %0, %1, %2\n\ts_nop 1" : "=v"(nu) : "v"(S[K]), "v"(-r));       // -u, two wait states before its first DPP read
        Diag16Rows<K, K + 1>::run(S, R, nu, u, wk);
    }
    if constexpr (K + 1 < KEND) diag16_pivot<K + 1, KEND>(S, R, ok);
}
// tile: 256 doubles of LDS owned by this wave; on return it holds W = L^-1 row-major with the column XOR-swizzled (tile[row * 16 + (col ^ row)]), exact zeros
// above the diagonal; the return value is the same W in C layout.
__device__ __forceinline__ v4d diag16_invert_dpp(v4d s, int lane, bool& ok, double* tile) {
    const int col = lane & 15, g = lane >> 4;
    asm volatile("" ::: "memory");
#pragma unroll
    for (int r = 0; r < 4; ++r) tile[(g + 4 * r) * 16 + col] = s[r];
    asm volatile("" ::: "memory");
    double S[16], R[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { S[i] = tile[i * 16 + col]; R[i] = (i == col) ? 1.0 : 0.0; }     // (row i of the upper triangle; below the diagonal the lanes carry values nobody reads)
    asm volatile("" ::: "memory");
    ok = true;
    diag16_pivot<0>(S, R, ok);
    if (g == 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) tile[i * 16 + (col ^ i)] = R[i];
    }
    asm volatile("" ::: "memory");
    v4d w;
#pragma unroll
    for (int q = 0; q < 4; ++q) { const int row = g + 4 * q; w[q] = tile[row * 16 + (col ^ row)]; }
    asm volatile("" ::: "memory");
    return w;
}
// ---------------------------------------------------------------------------------------------------------
// The DPP elimination with S and R PACKED into the same 16 registers: the EVEN 16-lane DPP rows of register X_i hold row i of S (lane c: S[i][c]), the ODD
// rows hold row i of R.  A row_newbcast operand is broadcast inside each DPP row on its own, so with nu = -L[:, k] in EVERY row and Y = X_k / sqrt(d) (u in
// the even rows, W_k in the odd ones: one multiply) the ONE instruction  X_i += nu[lane i] * Y  is S_i -= L[i][k] u in the even rows and R_i -= L[i][k] W_k in the odd
// ones: 120 DPP multiply-adds a tile instead of 240, 16 live register pairs instead of 32 -- which is what lets the one-wave kernel use it (the unpacked routine
// spills there, see above).  Every entry goes through the arithmetic of diag16_pivot, operation by operation: the two return the same bits.  The price is one row
// exchange per pivot: S_k has to reach the odd rows for nu (v_permlane16_swap of two copies: [S R S R] x 2 -> [S S S S], [R R R R]).
// Wait states (the hazard recogniser does not see into the asm statements, and pads one state behind them): a VGPR written by a vector instruction needs two
// before a DPP operand or a v_permlane*_swap reads it -- the s_nop 1 in front of every such read below; the multiply-adds of a pivot are at most three statements
// (first row | rows up to 7 | rows 8 .. 15), each with its operands pinned and its own s_nop, as fmac_row_bcast_block (srbdqp_admm.hpp).
// ---------------------------------------------------------------------------------------------------------
// (Round 35: the two copies are two v_mov_b64 where they were four v_mov_b32 -- tools/mov64_probe.hip: one issues like one.  The assembler's operand syntax has no
// name for the halves of a 64-bit operand, so the swaps cannot stand in the statement that makes the copies: they are the compiler's builtins, which swap the halves in
// place in the copies' registers, and whose hazards the recogniser knows -- should the allocator ever put a move between a copy and its swap, the wait states come with
// it.  The copies' own two wait states are the s_nop 1 that ends their statement, as before.)
__device__ __forceinline__ double pk_even_rows(double x) {   // the even DPP rows of x (rows 0, 2), each also in the odd row behind it
    double a, b;                                              // (b: the swap's second operand, a register pair the swaps need and nobody reads afterwards -- it ends as [R R R R])
    asm("v_mov_b64 %0, %2\n\tv_mov_b64 %1, %2\n\ts_nop 1" : "=&v"(a), "=&v"(b) : "v"(x));
    const v2u_t lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
    const v2u_t hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
    return __hiloint2double((int)hi[0], (int)lo[0]);
}
#define SRBDQP_PK(P, I) "v_fmac_f64_dpp %" #P ", %8, %9 row_newbcast:" #I " row_mask:0xf bank_mask:0xf\n\t"
#define SRBDQP_PK_LO7 SRBDQP_PK(7, 7)
#define SRBDQP_PK_LO6 SRBDQP_PK(6, 6) SRBDQP_PK_LO7
#define SRBDQP_PK_LO5 SRBDQP_PK(5, 5) SRBDQP_PK_LO6
#define SRBDQP_PK_LO4 SRBDQP_PK(4, 4) SRBDQP_PK_LO5
#define SRBDQP_PK_LO3 SRBDQP_PK(3, 3) SRBDQP_PK_LO4
#define SRBDQP_PK_LO2 SRBDQP_PK(2, 2) SRBDQP_PK_LO3
#define SRBDQP_PK_HI15 SRBDQP_PK(7, 15)
#define SRBDQP_PK_HI14 SRBDQP_PK(6, 14) SRBDQP_PK_HI15
#define SRBDQP_PK_HI13 SRBDQP_PK(5, 13) SRBDQP_PK_HI14
#define SRBDQP_PK_HI12 SRBDQP_PK(4, 12) SRBDQP_PK_HI13
#define SRBDQP_PK_HI11 SRBDQP_PK(3, 11) SRBDQP_PK_HI12
#define SRBDQP_PK_HI10 SRBDQP_PK(2, 10) SRBDQP_PK_HI11
#define SRBDQP_PK_HI9 SRBDQP_PK(1, 9) SRBDQP_PK_HI10
#define SRBDQP_PK_HI8 SRBDQP_PK(0, 8) SRBDQP_PK_HI9
#define SRBDQP_PK_MID11 SRBDQP_PK(3, 11)
#define SRBDQP_PK_MID10 SRBDQP_PK(2, 10) SRBDQP_PK_MID11
#define SRBDQP_PK_MID9 SRBDQP_PK(1, 9) SRBDQP_PK_MID10
#define SRBDQP_PK_MID8 SRBDQP_PK(0, 8) SRBDQP_PK_MID9
#define SRBDQP_PK_ASM(TAIL, B) asm("s_nop 1\n\t" TAIL : "+v"(X[B]), "+v"(X[B + 1]), "+v"(X[B + 2]), "+v"(X[B + 3]), "+v"(X[B + 4]), "+v"(X[B + 5]), "+v"(X[B + 6]), "+v"(X[B + 7]) : "v"(nu), "v"(y))
// X_i += nu[lane i of the row] * y for the rows FROM .. END - 1 (all 8 registers of a half are operands of its statement: the finished ones are simply not named in
// it).  END = 16, or 12 / 8 for a tile whose last rows are padding (diag16_invert_dpp_packed<NP>): those rows are not touched at all.
template <int FROM, int END = 16>
__device__ __forceinline__ void pk_rows(double (&X)[16], double nu, double y) {
    static_assert(END == 16 || END == 12 || END == 8, "whole k-steps of four rows");
    if constexpr (FROM == 2) SRBDQP_PK_ASM(SRBDQP_PK_LO2, 0);
    else if constexpr (FROM == 3) SRBDQP_PK_ASM(SRBDQP_PK_LO3, 0);
    else if constexpr (FROM == 4) SRBDQP_PK_ASM(SRBDQP_PK_LO4, 0);
    else if constexpr (FROM == 5) SRBDQP_PK_ASM(SRBDQP_PK_LO5, 0);
    else if constexpr (FROM == 6) SRBDQP_PK_ASM(SRBDQP_PK_LO6, 0);
    else if constexpr (FROM == 7) SRBDQP_PK_ASM(SRBDQP_PK_LO7, 0);
    if constexpr (END == 8) return;
    else if constexpr (END == 12) {
        if constexpr (FROM <= 8) SRBDQP_PK_ASM(SRBDQP_PK_MID8, 8);
        else if constexpr (FROM == 9) SRBDQP_PK_ASM(SRBDQP_PK_MID9, 8);
        else if constexpr (FROM == 10) SRBDQP_PK_ASM(SRBDQP_PK_MID10, 8);
        else if constexpr (FROM == 11) SRBDQP_PK_ASM(SRBDQP_PK_MID11, 8);
    }
    else if constexpr (FROM <= 8) SRBDQP_PK_ASM(SRBDQP_PK_HI8, 8);
    else if constexpr (FROM == 9) SRBDQP_PK_ASM(SRBDQP_PK_HI9, 8);
    else if constexpr (FROM == 10) SRBDQP_PK_ASM(SRBDQP_PK_HI10, 8);
    else if constexpr (FROM == 11) SRBDQP_PK_ASM(SRBDQP_PK_HI11, 8);
    else if constexpr (FROM == 12) SRBDQP_PK_ASM(SRBDQP_PK_HI12, 8);
    else if constexpr (FROM == 13) SRBDQP_PK_ASM(SRBDQP_PK_HI13, 8);
    else if constexpr (FROM == 14) SRBDQP_PK_ASM(SRBDQP_PK_HI14, 8);
    else if constexpr (FROM == 15) SRBDQP_PK_ASM(SRBDQP_PK_HI15, 8);
}
#undef SRBDQP_PK_ASM
#undef SRBDQP_PK_HI8
#undef SRBDQP_PK_HI9
#undef SRBDQP_PK_HI10
#undef SRBDQP_PK_HI11
#undef SRBDQP_PK_HI12
#undef SRBDQP_PK_HI13
#undef SRBDQP_PK_HI14
#undef SRBDQP_PK_HI15
#undef SRBDQP_PK_MID8
#undef SRBDQP_PK_MID9
#undef SRBDQP_PK_MID10
#undef SRBDQP_PK_MID11
#undef SRBDQP_PK_LO2
#undef SRBDQP_PK_LO3
#undef SRBDQP_PK_LO4
#undef SRBDQP_PK_LO5
#undef SRBDQP_PK_LO6
#undef SRBDQP_PK_LO7
#undef SRBDQP_PK
// The wave-private LDS of the packed inversion, in doubles from its base: three tiles and the riding panel's area, every access of which is ONE lane base plus
// immediate offsets.
//   [0, 256)          S, row-major, rows 16 apart: stored from C layout (lane l, register r: l + 64 r), read back a row per register.
//   [0, 271)          W = L^-1 in its place once S is in registers: row i at wrow(i) = 17 i.  With immediate offsets the compiler pairs the accesses of a lane into
//                     ds_read2_b64 / ds_write2_b64, which the LDS serves in groups of 16 consecutive lanes over 32 banks (16 doubles): the store of row i and the
//                     C-layout read of rows g + 4 q (68 q behind the lane base 17 g + col) are the 16 lanes of one DPP row on 16 consecutive doubles, and the
//                     A-operand read of lane (k', i) at 17 i + k' + 4 r has the lanes i = 0 .. 15 of a group on 17 i mod 16 = i: all three free of conflicts.
//                     (Unpaired, as ds_read_b64 -- two 32-lane halves over 64 banks -- stride 17 has one two-way collision in each of the two reads, stride 18 two
//                     in the second; stride 16 + 2 per row PAIR is free of conflicts there, and two-way in the paired A-operand read that is actually emitted:
//                     measured, SQ_LDS_BANK_CONFLICT + 48 cycles a pass.  profiles/r23_wave_setup_diet.txt.)  (Until round 22: rows 16 apart with the column
//                     XOR-swizzled, tile[i * 16 + (col ^ i)] -- sixteen store and eight read addresses formed in registers per tile.)
//   [kIdent, +256)    the 16 x 16 identity, row-major, rows 16 apart: written once per pass (pk_ident_store), read by the odd DPP rows beside the even rows' S --
//                     kIdent = 16 (mod 32), so that also unpaired reads, in which a DPP row's S shares a 32-lane half with the next row's identity, sit 32 banks apart.
//   [kPanel, +271)    the riding panel tile (diag16_invert_dpp_packed<16, true>): B stored and read as S is (row-major, rows 16 apart: DPP row 3 reads it beside row 2's
//                     S, and kPanel = 16 (mod 32) as kIdent is, for the same reason), then U = L^-1 B in its place with row i at kPanel + wrow(i), stored by DPP row 3
//                     in the instructions that store row 1's W (two DPP rows of one store: two groups of 16 consecutive doubles, served one after the other) and
//                     read back in C layout as W is -- the three access kinds of S / W at another base, with their reasoning.
struct PkTile {
    static constexpr int kIdent = 272;
    static constexpr int kPanel = kIdent + 256;
    static constexpr int kDoubles = kPanel + 272;
    static constexpr __host__ __device__ int wrow(int row) { return 17 * row; }
};
static_assert(PkTile::kIdent % 32 == 16 && PkTile::kPanel % 32 == 16 && PkTile::kIdent >= PkTile::wrow(15) + 16 && PkTile::kDoubles >= PkTile::kPanel + PkTile::wrow(15) + 16, "PkTile");
// lane (g, col) stores its four entries of the identity, (g + 4 r, col): the C-layout store of the S tile
__device__ __forceinline__ void pk_ident_store(double* tile, int lane) {
    const int col = lane & 15, g = lane >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) tile[PkTile::kIdent + lane + 64 * r] = (g + 4 * r == col) ? 1.0 : 0.0;
}
// pivot K of NP: rows K + 1 .. NP - 1 take the multiply-adds, the recursion ends behind pivot NP - 1 (NP < 16: see diag16_invert_dpp_packed)
template <int K, int NP = 16>
__device__ __forceinline__ void diag16_pivot_packed(double (&X)[16], unsigned& worst) {
    const double sk = pk_even_rows(X[K]);         // row k of S in every DPP row
    const double d = mov_newbcast<K>(sk);
    // a pivot is good when it is positive and finite, its high word in [1, 0x7ff00000): what d > 0.0 accepts in the other routines, less the subnormals below
    // 2^-1042 and +infinity (a NaN fails here as there) -- one unsigned maximum per pivot, decided once per tile (as sixteen fp64 comparisons the compiler gathers
    // them behind the elimination and keeps every pivot in registers until then)
    const unsigned dh = (unsigned)__double2hiint(d) - 1u;
    worst = dh > worst ? dh : worst;
    const double r = fast_rsqrt(d);
    const double y = X[K] * r;                    // even rows: u = row k of L'; odd rows: W_k
    if constexpr (K + 1 < NP) {
        double nu;                                // -u in every row; the first row below the pivot in the same statement: the next pivot's chain hangs on it alone
        asm("v_mul_f64 %1, %3, -%4\n\ts_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:%5 row_mask:0xf bank_mask:0xf"
            : "+v"(X[K + 1]), "=&v"(nu) : "v"(y), "v"(sk), "v"(r), "n"(K + 1));
        if constexpr (K + 2 < NP) pk_rows<K + 2, NP>(X, nu, y);
        X[K] = y;                                 // (behind the statements that name y as an input: assigned ahead of them, X[K] is a second register and a copy)
        diag16_pivot_packed<K + 1, NP>(X, worst);
    } else {
        X[K] = y;
    }
}
// tile: PkTile::kDoubles doubles of LDS owned by this wave, the identity in place (pk_ident_store).  In: S in C layout.  On return the tile holds W = L^-1 with
// row i at PkTile::wrow(i), exact zeros above the diagonal -- the A operand of W is read straight from it (a_operand_read, srbdqp_setup1.hpp) --; the return value
// is the same W in C layout.
// NP < 16 (12 or 8): the caller's promise that rows and columns NP .. 15 of S are padding -- exact zeros off the diagonal, 1.0 on it (the last diagonal tile of a K
// whose size is no multiple of 16: kasm_rows / dcol, srbdqp_setup1.hpp).  Then the elimination stops behind pivot NP - 1 and leaves rows NP .. 15 alone.  The full routine
// computes nothing there: a padded row i has nu[lane i] = -(+-0 * r) = -+0 at every real pivot, so its multiply-adds put +-0 on the +0 / 1.0 of the identity row
// (+0 + -0 = +0: not even a sign moves), and its own pivot is 1.0 with fast_rsqrt(1.0) = 1.0 exactly and a row of +-0 to pass down.  So register X_i, i >= NP, holds
// after the full routine what the packed load put there -- row i of the identity on the odd DPP rows, which is what the store below writes as row i of W (the even
// rows hold S's row i, 0 / 1 as well, and are not stored) -- and the rows below NP never see the padded ones (nu of a real row is its own S entry).  W, the returned
// C-layout tile and `ok` (a padded pivot's high word, 0x3ff00000, never decides the maximum's comparison) are the full routine's bit for bit whenever S is finite;
// where it is not, a real pivot fails in both and the padded rows here stay the finite identity where the full routine spreads NaNs into them.
// RIDE (NP = 16 only): DPP row 3, whose copy of R nobody reads, carries a second tile instead.  *panel holds B (C layout: the tile to the right of S in its block
// row of K) on entry and U = L^-1 B on return.  Row 3 of register X_i starts as row i of B where it started as row i of the identity, and the pivots do to it what
// they do to every row, not one instruction more: y = X_k r is row k of U (B_k less its sum, over the diagonal entry of L), X_i += nu[lane i] y is
// B_i -= L[i][k] U_k -- forward substitution on [S | I | B], operation by operation, each column of B in its own lane.  Rows 0 and 2 hold S as before
// (pk_even_rows reads nothing else), row 1 holds R: W and `ok` are the routine's without RIDE bit for bit, whatever B holds -- `worst` is formed from the
// even rows' S alone, so a NaN or an infinity in B ends in U and nowhere else here (the caller's trailing update carries it to a later pivot).
template <int NP = 16, bool RIDE = false>
__device__ __forceinline__ v4d diag16_invert_dpp_packed(v4d s, int lane, bool& ok, double* tile, [[maybe_unused]] v4d* panel = nullptr) {
    static_assert(NP == 16 || NP == 12 || NP == 8, "padding in whole k-steps of four rows");
    static_assert(!RIDE || NP == 16, "the riding panel goes through every pivot");
    const int col = lane & 15, g = lane >> 4;
    asm volatile("" ::: "memory");
#pragma unroll
    for (int r = 0; r < 4; ++r) tile[lane + 64 * r] = s[r];
    if constexpr (RIDE) {
#pragma unroll
        for (int r = 0; r < 4; ++r) tile[PkTile::kPanel + lane + 64 * r] = (*panel)[r];
    }
    asm volatile("" ::: "memory");
    // register i: row i of S on the even DPP rows (of the upper triangle; below the diagonal the lanes carry values nobody reads), row i of the identity on the odd
    // ones (RIDE: on row 1, and row i of B on row 3) -- sixteen reads off one lane base.  (Until round 22 every lane read S and the odd rows took the identity
    // through two DPP moves a register.)
    const double* rowp = tile + col + (RIDE ? (g == 1 ? PkTile::kIdent : g == 3 ? PkTile::kPanel : 0) : ((g & 1) ? PkTile::kIdent : 0));
    double X[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) X[i] = rowp[i * 16];
    asm volatile("" ::: "memory");
    unsigned worst = 0u;
    diag16_pivot_packed<0, NP>(X, worst);
    ok = worst < 0x7fefffffu;                     // (zero, negative, NaN and infinite pivots fail, and subnormal ones with a zero high word)
    if constexpr (RIDE) {
        if (g & 1) {                              // row 1: W; row 3: U, the same offsets off its own base
            double* const outp = tile + col + (g == 3 ? PkTile::kPanel : 0);
#pragma unroll
            for (int i = 0; i < 16; ++i) outp[PkTile::wrow(i)] = X[i];
        }
    } else {
        if (g == 1) {
#pragma unroll
            for (int i = 0; i < 16; ++i) tile[PkTile::wrow(i) + col] = X[i];
        }
    }
    asm volatile("" ::: "memory");
    const double* cp = tile + lane + g;                 // wrow(g) + col = 17 g + col; row g + 4 q is wrow(4) q behind it
    v4d w;
#pragma unroll
    for (int q = 0; q < 4; ++q) w[q] = cp[PkTile::wrow(4) * q];
    if constexpr (RIDE) {
#pragma unroll
        for (int q = 0; q < 4; ++q) (*panel)[q] = cp[PkTile::kPanel + PkTile::wrow(4) * q];
    }
    asm volatile("" ::: "memory");
    return w;
}

// ... from a row-major 16 x 16 tile `in` (float or double, not swizzled; this wave's own writes, complete) into the swizzled tile `out` (may be the same memory when
// the types agree): the form the tile phases use -- the inverse of a diagonal tile is only ever read back from LDS.
template <typename TI, typename TO>
__device__ __forceinline__ void diag16_invert_dpp_tiles(const TI* in, TO* out, int lane, bool& ok) {
    const int col = lane & 15, g = lane >> 4;
    double S[16], R[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { S[i] = (double)in[i * 16 + col]; R[i] = (i == col) ? 1.0 : 0.0; }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // (the reads are done before `out` -- possibly the same tile -- is written)
    ok = true;
    diag16_pivot<0>(S, R, ok);
    if (g == 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) out[i * 16 + (col ^ i)] = (TO)R[i];
    }
    asm volatile("" ::: "memory");
}

}  // namespace srbdqp
