// srbdqp_setup1.hpp -- set-up kernel of the split pipeline with ONE WAVE PER QP (first kernel; srbdqp_admm_kernel is
// the second).
//
// The 4-wave set-up kernel is latency-bound (61 % of its wave time parked on s_waitcnt / barriers) and holds only 4 QPs
// per CU, because a QP owns 4 waves x 118 registers and 38 KB of LDS (mostly the tile store).  Since the assembly is
// closed form (srbdqp_compact.hpp) nothing needs 256 threads: here the 10 upper 16x16 tiles of K are 80 registers of one
// wave in MFMA C layout and the whole factorisation stays in that wave's registers --
//   F  right-looking Cholesky K = U'U: diagonal tile inverted by the packed DPP elimination (diag16_invert_dpp_packed: no matrix-core
//      instruction, no v_readlane; since round 35 the panel's first tile U_j,j+1 = L_jj^-1 K_j,j+1 rides it as forward substitution in a spare DPP row), panel
//      U_jb = L_jj^-1 K_jb for b > j + 1 (the A operand L_jj^-1 is read from the wave-private LDS tile the inversion leaves it in: PkTile, srbdqp_mfma.hpp),
//      trailing update K_ab -= U_ja' U_jb with both operands straight from registers (register r of a C-layout tile is
//      the A operand of K-step r of a product that contracts over the tile's row index, and the B operand as well); on the way out of block row j
//      P_j = W_jj' W_jj (W_jj = L_jj^-1) takes the slot of the diagonal tile and -V_lj = -U_jl' W_jj the slot of U_jl, both such products;
//   I  X = K^-1 by block recurrence from the factor, U X = L^-1: X_jb = delta_jb P_j - sum_{l>j} V_lj' X_lb, block column by block column from the last and
//      each from its diagonal block upwards (X_lb = X_bl' for l > b comes back transposed through the staging tiles), stored to the hand-over workspace as
//      it is produced.  (Until round 19: W = L^-1 block row by block row, then K^-1 = W'W -- 208 matrix-core instructions a pass at NT = 4 where this takes 184; since round 33
//      174 at KS = 60: the k-steps over the padded rows 60 .. 63 of the last block are left out, and the last inversion runs its twelve real pivots -- PAD below.) --
// with no barrier anywhere (a workgroup is one wave) and 3x the QPs in flight per CU.  Produces exactly the workspace
// (persistent strip + dense K^-1) the 4-wave set-up kernel produces; everything else is shared with it.
#pragma once
#include "srbdqp_split.hpp"

namespace srbdqp {

// phase stamps of the wave kernel only in diagnostic builds (tools/build_variant.sh -DSRBDQP_WAVE_STAMPS): the stamp
// code costs registers even when the stamp buffer is null
#ifdef SRBDQP_WAVE_STAMPS
#define WSTAMP(a, b, idx) SRBDQP_STAMP(a, b, idx)
#define WSTAMP_RT(a, b, idx) do { if ((a).stamps && threadIdx.x == 0) (a).stamps[(size_t)(b) * 16 + (idx)] = (long long)__builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define WSTAMP(a, b, idx) do { } while (0)
#define WSTAMP_RT(a, b, idx) do { } while (0)
#endif

// LDS of one wave: [0, S::o_R) the persistent strip with the offsets of CompactSmem (the ADMM kernel reads it back from
// the workspace), then the phase-A arrays with their lifetimes shared: inputs, prefix sums and tables -> error vector / warm-start vectors -> the table rows of
// the K assembly -> the tiles of the packed inversion (over the prefix sums and tables) -> the K^-1 staging tiles.
template <int N, int MAXS>
struct Setup1Smem {
    using S = CompactSmem<N, MAXS>;
    static constexpr int n = Dims<N>::n;
    static constexpr int up2(int v) { return (v + 1) & ~1; }
    static constexpr int o_x0 = S::o_x0, o_tm = S::o_tm, o_J = S::o_J;   // strip offsets used by the shared helpers
    static constexpr int o_cp = S::o_R;                    // 9N   prefix sums C_k
    static constexpr int o_mt = o_cp + up2(9 * N);         // 18N  D_m, E_m of the rank-6 assembly (srbdqp_common.hpp, de_tables; until round 4: the 9 NPAIR doubles of M(j, m))
    static constexpr int o_ab = o_mt + 18 * N;             // the assembly's table rows, one per presolved variable: over everything below, which is dead by then
    static constexpr int o_gv = o_mt + up2(9 * S::NPAIR);  // 9N   G'v tables
    static constexpr int o_t1 = o_gv + up2(9 * N);         // 9N   T1(m)          | later: x0c (nmax + 16), tf (6N)
    static constexpr int o_t2 = o_t1 + up2(9 * N);         // 9N   T2(m)
    static constexpr int o_x0c = o_t1;
    static constexpr int o_tf = o_x0c + up2(S::nmax) + 16;
    static constexpr int endT = (o_t2 + up2(9 * N) > o_tf + 6 * N) ? o_t2 + up2(9 * N) : o_tf + 6 * N;
    static constexpr int o_xref = up2(endT);               // 13N  inputs
    static constexpr int o_foot = o_xref + up2(N * 13);    // 12N                  | later: eh (n), then G x^0 (n)
    static constexpr int o_pcom = o_foot + N * 12;         // 3N
    static constexpr int o_eh = o_foot;
    static constexpr int o_gx = o_foot;
    // the tiles of the packed inversion (PkTile, srbdqp_mfma.hpp: S / W, the constant identity and since round 35 the riding panel tile, 6.3 KB) during the
    // factorisation, when nothing behind the strip is alive: over the prefix sums and tables, which are dead with the K assembly, and under the K^-1 staging, which
    // begins behind the factorisation.  (Until round 22 one 2 KB tile over the inputs.)  NT >= 3 does not grow by it (three staging tiles, 864 doubles, cover its
    // 800): N = 10, MAXS = 2 stays at 16,672 bytes (18,208 with the parked (x, y)); a two-tile instantiation's end is the inversion's tiles or its table rows,
    // whichever lie further, inside the assert on kCuShareBytes below.
    static constexpr int o_scr = o_cp;
    static constexpr int endIn = o_pcom + up2(N * 3);
    static constexpr int kStgRow = 18;                    // row stride of the K^-1 staging tiles (16 + 2: the 16-byte row reads of 16 lanes hit 64 different banks)
    static constexpr int kStgTile = 16 * kStgRow;
    static constexpr int endStg = (endIn > o_cp + S::NT * kStgTile) ? endIn : o_cp + S::NT * kStgTile;   // K^-1 block-column staging (wave kernel)
    static constexpr int endAb = o_ab + 16 * S::NT * kAbStride;
    static constexpr int endPk = o_scr + PkTile::kDoubles;
    static constexpr int o_end = (endStg > endAb ? endStg : endAb) > endPk ? (endStg > endAb ? endStg : endAb) : endPk;
    static constexpr size_t bytes = (size_t)o_end * sizeof(double);
    static constexpr size_t kCuShareBytes = 20480;        // an eighth of the CU's 160 KB: eight workgroups (two waves per SIMD) fit, the parked (x, y) of the restart kernels included
    // The step pairs (m, i >= m) of the T1 / T2 and G'v tables, a lane each (setup1_pass): pair p = r (N + 1) + c, r < N / 2, is (m, i) = (r, r + c) for c < N - r and
    // (N - 1 - r, N - 1 - r + c - (N - r)) behind that -- row r of the rectangle holds the N - r pairs of step r and the r + 1 pairs of step N - 1 - r --, so that
    // the pairs of one m are neighbours in ascending i, from slot pair_base(m) on, and a lane finds its (m, i) without a table.  Slots up to pair_base(m) + N - 1
    // are addressed (never summed) by lane m: kPairSlots of them.
    static constexpr int kPairs = S::NPAIR;
    static constexpr int kPairSlots = (N / 2) * N + N;
    static constexpr int o_pd = o_t1;                      // 2 per slot: the entries a, b of C_i - C_m     (T1 / T2 sums only: x0c / tf come later)
    static constexpr int o_pq = up2(endIn);                // 4 per slot: the T2 terms of the pair | later: its three torque terms of the G'v tables
    static constexpr bool pairs_fit = N % 2 == 0 && kPairs <= 64 && 2 * kPairSlots <= 2 * up2(9 * N) && o_pq + 4 * kPairSlots <= o_end;   // (in LDS that is free while the tables are formed)
    static constexpr bool supported = SplitWs<N, MAXS>::supported && S::NT <= 4;
    static_assert(!supported || pairs_fit, "a lane and an LDS slot for every step pair of a horizon the one-wave kernel takes");
    static_assert(!supported || bytes + 3 * 64 * sizeof(double) <= kCuShareBytes, "eight workgroups of the one-wave kernel per CU");
    static_assert(n + 6 * N <= o_end - o_eh || true, "");
};

// FUSED = false: first kernel of the split pipeline (stores the persistent strip + K^-1 to the hand-over workspace).
// FUSED = true : the whole solve on this wave ("wave" kernel): the K^-1 tiles are turned into one row per lane through
//                the 2 KB transpose tile, then the ADMM iterations and the roll-out of srbdqp_split.hpp follow in place --
//                nothing but the inputs and the outputs touches HBM.
// PHI (split only): also store dq/dx0 for the two-phase call (srbdqp_prepare_staged_f64): q is affine in x0, so 13 more
//                passes of the gradient tables with x0 = e_k and x_ref = 0 give its 13 columns.
// RST (fused only): the rho restart IN PLACE.  A QP that has not converged after a.restart_every iterations re-balances its rho (OSQP's rule from the maxima of its
//                last check, each time from the rho of the pass that ended), repeats the part of the set-up that depends on rho -- the tables of the K assembly,
//                K, its factorisation and inverse, P x of the point it continues from; the inputs, J and the gradient stay -- and continues from its own (x, y), at most a.restart_max times; the
//                cap a.max_iter is on the total.  What a second launch over the capped QPs does for the other kernels (srbdqp.hip), without the launches: 4 % of
//                the configs[1] QPs pass the first mark, 1 % the second.  The body is compiled TWICE for this: the first pass as straight-line code (RP = 1: the
//                code of the kernel without restart), the continued passes as a loop behind it (RP = 2) -- ONE copy inside a loop has hipcc hoist the body's
//                lane-index arithmetic, fp64 constants and literal materialisations in front of the loop and keep them in registers through the whole body
//                (256 VGPRs + 228 bytes of scratch against 224 + 0, -7 % on every QP); this way only the restarted QPs run the loop's code.
//                The (x, y) of a pass wait in 1.5 KB of LDS behind the kernel's own.  oracle: SrbdParams.rho_restart_iter / rho_restart_count.
// One pass of the body.  RP: 0 = the whole solve of a kernel without restart; 1 = first pass of a restart kernel; 2 = a continued pass in the SAME workgroup (the
// strip is in place); 3 = a continued pass in ANOTHER workgroup (deferred tails, srbdqp_wave_defer_kernel: the strip is rebuilt from the inputs, (x, y) of the
// pass before were put into park[] by the caller).  io: the QP's own pointers (RP = 3: those of the launch it came from).  Returns true if another pass follows
// (rho_b, rs_pass, rs_done updated; (x, y) in park[]).
template <int N, int MAXS, bool FUSED, bool DUMP, bool PHI, int RP>
__device__ __forceinline__ bool setup1_pass(const KArgs& a, const QpIo& io, const int b, double* sm, double& rho_b, int& rs_pass, int& rs_done) {
    using S = CompactSmem<N, MAXS>;
    using W = SplitWs<N, MAXS>;
    using L1 = Setup1Smem<N, MAXS>;
    constexpr int n = Dims<N>::n, m = Dims<N>::m, NT = S::NT;
    int lane = threadIdx.x;
    if constexpr (RP == 2) asm volatile("" : "+v"(lane));   // (inside the loop of the continued passes: an opaque value in every trip, or its arithmetic is hoisted too)
    [[maybe_unused]] double* const park = sm + L1::o_end;   // RP > 0: [3][64] behind the kernel's own LDS
    int mcol = lane & 15, kq = lane >> 4;
    double* ws = FUSED ? nullptr : a.ws + (size_t)b * W::doubles;
    int* icnt = reinterpret_cast<int*>(sm + S::o_int);
    int* imisc = icnt + 2 * N;
    uint8_t* act = reinterpret_cast<uint8_t*>(imisc + 8);
    uint8_t* sct = reinterpret_cast<uint8_t*>(sm + S::o_ct);
    const double* SQ = sm + S::o_sq;
    const double* CP = sm + L1::o_cp;

    // ================= load + linearise (a5) =================
    // Round 6: on the whole wave, from registers, behind ONE barrier.  Every global load is issued first (each lane also fetches the foot / CoM operands of its
    // own J entries and the x_ref entries of its own error-vector rows, so that neither goes through LDS); lane k < N forms cos / sin of yaw_k, the J loop reads
    // them from lane k (a shuffle) and C_k = sum_{l<=k} T_l -- only two of its nine entries are not constant: C_k = [[cc_k, cs_k, 0], [-cs_k, cc_k, 0],
    // [0, 0, k + 1]] -- is summed in registers, lane to lane, in the order of the serial loop it replaces (the chain below).  (Until round 6: inputs -> LDS, three barriers, a 9-lane prefix loop
    // of ten dependent LDS round trips and a J loop reading its operands back from LDS.)
    WSTAMP(a, b, 0);
    WSTAMP_RT(a, b, 12);
    constexpr int JT = (12 * N + 63) / 64;                   // trips of the wave over the 12 N entries of J (and of the error vector: n = 12 N as well)
    double yc, ys;                                           // lane k < N: cos / sin of yaw_k
    [[maybe_unused]] double v_xr[JT];                        // x_ref entry of error-vector row lane + 64 t
    if constexpr (RP == 2) {   // the strip (contact lists, T, J, x0, q) is in place; the prefix sums were overwritten by the K^-1 staging
        const int k = lane < N ? lane : 0;
        yc = sm[S::o_tm + k * 9 + 0];
        ys = sm[S::o_tm + k * 9 + 1];
    } else {
        const double* gx0 = io.x0 + (size_t)b * 13;
        const double* gxr = io.xref + (size_t)b * N * 13;
        const double* gft = io.foot + (size_t)b * N * 12;
        const uint8_t* gct = io.contact + (size_t)b * N * 4;
        const double* gpc = io.pcom ? io.pcom + (size_t)b * N * 3 : nullptr;
        // (clamped indices, no branch: the loads of every lane travel together)
        const double v_x0 = gx0[lane < 13 ? lane : 0];
        const uint8_t v_ct = gct[lane < 4 * N ? lane : 0];
        const double v_yaw = gxr[(lane < N ? lane : 0) * 13 + 2];
        double v_f[JT][3], v_p[JT][3];
#pragma unroll
        for (int t = 0; t < JT; ++t) {
            const int tt = (lane + 64 * t < 12 * N) ? lane + 64 * t : 0;
            const int t3 = (int)((unsigned)tt / 3u), k = t3 >> 2;       // entry tt = 12 k + 3 ci + ax: the contact's three coordinates start at 3 (tt / 3)
            const double* pc = gpc ? gpc + k * 3 : gxr + k * 13 + 3;     // no CoM path: the CoM of x_ref
#pragma unroll
            for (int c = 0; c < 3; ++c) { v_f[t][c] = gft[3 * t3 + c]; v_p[t][c] = pc[c]; }
            v_xr[t] = gxr[tt + k];                                       // (k * 13 + tt - 12 k)
        }
        sincos(v_yaw, &ys, &yc);
        if (lane < 13) sm[S::o_x0 + lane] = v_x0;
        if (lane >= 32 && lane < 44) sm[S::o_sq + lane - 32] = a.sqrtq[lane - 32];
        if (lane < N * 4) sct[lane] = v_ct ? 1 : 0;
        if (lane < N) {   // Rz(yaw_k)'
            double* T = sm + S::o_tm + lane * 9;
            T[0] = yc;  T[1] = ys;  T[2] = 0.0;
            T[3] = -ys; T[4] = yc;  T[5] = 0.0;
            T[6] = 0.0; T[7] = 0.0; T[8] = 1.0;
        }
        {   // presolve: compact the stance contacts; per-step bound check from the same ballot
            const bool flag = (lane < 4 * N) && v_ct != 0;
            const unsigned long long bal = __ballot(flag);
            if (flag) act[__popcll(bal & ((1ull << lane) - 1ull))] = (uint8_t)lane;
            if (lane < N) icnt[lane] = __popcll(bal & ((4 * (lane + 1) >= 64) ? ~0ull : ((1ull << (4 * (lane + 1))) - 1ull)));
            const bool over = lane < N && __popcll((bal >> (4 * (lane < N ? lane : 0))) & 0xFull) > MAXS;
            const unsigned long long viol = __ballot(over);
            if (lane == 0) {
                imisc[0] = __popcll(bal);
                imisc[1] = viol != 0ull;
                sm[S::o_misc] = 0.0;
                sm[S::o_misc + 1] = 0.0;
            }
        }
#pragma unroll
        for (int t = 0; t < JT; ++t) {   // J_k[:, 3 ci + ax] = Iw^-1 * skew(r)[:, ax]
            const int tt = lane + 64 * t;
            const int tc = tt < 12 * N ? tt : 0, t3 = (int)((unsigned)tc / 3u), k = t3 >> 2, cc = tt - 12 * k, ax = tc - 3 * t3;   // (one division: tt / 12 = (tt / 3) / 4)
            const double cs = __shfl(yc, k), sn = __shfl(ys, k);    // (every lane takes part: the shuffles sit outside the store's condition)
            const double i0 = a.iinv[0], i1 = a.iinv[1], i2 = a.iinv[2];
            const double w00 = cs * cs * i0 + sn * sn * i1, w01 = cs * sn * (i0 - i1), w11 = sn * sn * i0 + cs * cs * i1;
            const double rx = v_f[t][0] - v_p[t][0];
            const double ry = v_f[t][1] - v_p[t][1];
            const double rz = v_f[t][2] - v_p[t][2];
            // column ax of skew(r) as selects (a three-way if chain on this value was miscompiled in srbdqp_wrench.hpp)
            const double s0 = (ax == 0) ? 0.0 : ((ax == 1) ? -rz : ry);
            const double s1 = (ax == 0) ? rz : ((ax == 1) ? 0.0 : -rx);
            const double s2 = (ax == 0) ? -ry : ((ax == 1) ? rx : 0.0);
            if (tt < 12 * N) {
                double* J = sm + S::o_J + k * 36;
                J[0 * 12 + cc] = w00 * s0 + w01 * s1;
                J[1 * 12 + cc] = w01 * s0 + w11 * s1;
                J[2 * 12 + cc] = i2 * s2;
            }
        }
    }
    // prefix sums C_k (cc_k = sum_{l<=k} cos yaw_l, cs_k = sum_{l<=k} sin yaw_l: the serial loop's order) on lane k, and from there to LDS: a chain over
    // neighbouring lanes, acc = (acc of the lane before) + own term, N - 1 times behind acc = 0 + own term (row_prev: lanes 0 .. N - 1 sit in one 16-lane DPP row, and
    // lane 0 reads +0.0 in every step).  Lane m is final after step m -- ((0 + c_0) + c_1) + ... + c_m, the loop's association, its +0 for c_0 = -0.0 included --
    // and every later step forms the same value from the same operands again, so no step needs a select; lanes past N - 1 hold values nobody reads.  (Until round
    // 22: lane m summed the wave-uniform cos / sin of all N steps, 2 N v_readlane pairs, the steps past m selected to exact zeros.  Until round 13 the prefix
    // sums were ALSO kept as twenty wave-uniform doubles for the T1 / T2 loop of lane m; the step pairs below read C_i and C_m back from LDS instead.)
    static_assert(N <= 16, "the prefix chain stays inside one 16-lane DPP row");
    double ccm = 0.0 + yc, csm = 0.0 + ys;
#pragma unroll
    for (int k = 1; k < N; ++k) {
        ccm = row_prev(ccm) + yc;
        csm = row_prev(csm) + ys;
    }
    if (lane < N) {
        double* C = sm + L1::o_cp + lane * 9;
        C[0] = ccm;  C[1] = csm; C[2] = 0.0;
        C[3] = -csm; C[4] = ccm; C[5] = 0.0;
        C[6] = 0.0;  C[7] = 0.0; C[8] = (double)(lane + 1);
    }
    __syncthreads();
    const int na = imisc[0];
    const int n_eff = 3 * na;
    double* xs0 = sm + L1::o_mt;                             // scratch vectors of the early exit (n + 12N doubles; M is not built)
    static_assert(L1::o_end - L1::o_mt >= n + 12 * N, "early-exit scratch");
    if (RP != 2 && (imisc[1] != 0 || na == 0)) {   // bound violated (status -2) or nothing to solve (all forces 0): finished here
        if constexpr (DUMP) { if (lane == 0) a.ub_out[(size_t)b * m] = (imisc[1] != 0) ? -1.0 : 0.0; return false; }   // assembly dump: nothing to show
        for (int c = lane; c < n; c += 64) xs0[c] = 0.0;
        if (io.y_out) for (int i = lane; i < m; i += 64) io.y_out[(size_t)b * m + i] = 0.0;
        if (lane == 0) {
            if (io.status) io.status[b] = (imisc[1] != 0) ? kStatusContactBound : 1;
            if (io.iters) io.iters[b] = a.iters_base;
            if constexpr (!FUSED) ws[S::o_misc + 1] = 1.0;
        }
        __syncthreads();
        rollout_and_store_to<N, S, 64>(a, io.u_out, io.x_out, b, sm, xs0, xs0 + n);
        return false;
    }

    WSTAMP(a, b, 1);
    // ================= closed-form tables, gradient, warm-start P x^0 (see srbdqp_compact.hpp, phase A) =================
    const double dt = a.dt, dt2 = a.dt * a.dt, dtm = a.dt * a.inv_mass, dt2m = dt2 * a.inv_mass;
    double* DE = sm + L1::o_mt;
    double* GV = sm + L1::o_gv;
    if constexpr (RP != 2) {
#pragma unroll
        for (int t = 0; t < JT; ++t) {   // error vector: one row per lane and trip, every kind of row in the same instructions (free_response_sel)
            const int k = lane + 64 * t;
            const int kc = k < n ? k : 0, i = kc / 12, kk = kc - 12 * i;
            const double v = SQ[kk] * (free_response_sel<N, L1>(a, sm, i, kk) - v_xr[t]);
            if (k < n) sm[L1::o_eh + k] = v;
        }
    }
    // T1(m) = sum_{i>=m} (C_i - C_m), T2(m) = sum_{i>=m} (C_i - C_m)' W (C_i - C_m) (W = diag(q_0..2)) and from them D_m, E_m of the rank-6 assembly, on lane m
    // (de_step).  C has two non-constant entries, so T1 has two (t1a, t1b: [[t1a, t1b, 0], [-t1b, t1a, 0], [0, 0, t1z]]) and T2
    // three ([[t2aa, t2ab, 0], [t2ab, t2bb, 0], [0, 0, t2zz]]).  The sums stay in the differences-first form (every term formed from C_i - C_m, as the loop over LDS
    // it replaces did): the suffix-sum form S(m) - (N - m) C_m, Q(m) - C_m'W S(m) - ... is O(1) per entry but cancels -- C_i grows like i, and T2 near the end
    // of the horizon comes out ~250 ulps off at N = 10 against a few for this form (tests/test_suffix_tables_cpu.py).  (Until round 6: 6 N lanes with 8 LDS reads per step each, a barrier,
    // de_tables over LDS.  Rounds 6 - 12: lane m alone, an N-step loop over wave-uniform prefix sums held in 4 N registers.)
    // Round 13: the terms on the step PAIRS (m, i >= m), a lane each (N (N + 1) / 2 <= 64; Setup1Smem, kPairs) -- the differences and the six terms of a pair are
    // formed once, by one instruction for all pairs, where lane m formed them in N unrolled steps of ~36 instructions with 54 lanes idle -- and lane m adds up the
    // slots of its pairs in ascending i, which is the loop's order.  One term stays on lane m: the loop's LAST step (i = N - 1, which every m takes) went into t2zz as
    // ONE multiply-add, fma(w2 dz, dz, t2zz) -- its select was provably true and the compiler fused the product with the accumulator --, so the pairs (m, N - 1) store
    // +0 there and lane m ends with that multiply-add; a term rounded first gives another D_m[2][2] wherever w2 dz^2 is not exact (it is exact with the default weight).
    // The pair lane keeps its two differences for the torque entries of gt_tables.
    const int pair_c = lane < L1::kPairs ? lane : L1::kPairs - 1;                    // (lanes past the last pair repeat it and store nothing)
    const int pair_r = pair_c / (N + 1), pair_k = pair_c - pair_r * (N + 1);
    const bool pair_lo = pair_k < N - pair_r;
    const int pair_m = pair_lo ? pair_r : N - 1 - pair_r, pair_i = pair_m + (pair_lo ? pair_k : pair_k - (N - pair_r));
    const double pair_da = CP[9 * pair_i] - CP[9 * pair_m], pair_db = CP[9 * pair_i + 1] - CP[9 * pair_m + 1];
    double* PD = sm + L1::o_pd;
    double* PQ = sm + L1::o_pq;
    {
        const double w0 = SQ[0] * SQ[0], w1 = SQ[1] * SQ[1], w2 = SQ[2] * SQ[2];
        const double da = pair_da, db = pair_db, dz = (double)(pair_i - pair_m);
        if (lane < L1::kPairs) {
            PD[2 * lane] = da;
            PD[2 * lane + 1] = db;
            // (w0 da) da + (w1 db) db, (w0 da) db - (w1 db) da, (w0 db) db + (w1 da) da with the multiply-adds written out, so that the rounding is chosen here and
            // not by the compiler's contraction of the day: the first product fused, the second rounded (what lane m's loop computed until round 12)
            PQ[4 * lane] = fma(w0 * da, da, (w1 * db) * db);
            PQ[4 * lane + 1] = fma(w0 * da, db, -((w1 * db) * da));
            PQ[4 * lane + 2] = fma(w0 * db, db, (w1 * da) * da);
            PQ[4 * lane + 3] = (pair_i == N - 1) ? 0.0 : (w2 * dz) * dz;                // (the last step's term: lane m, below)
        }
    }
    __syncthreads();
    const int pair_base = (2 * lane < N) ? lane * (N + 1) : (N - lane) * N;          // lane m < N: the slot of its pair (m, m)
    if (lane < N) {
        const int mm = lane;
        double t1a = 0.0, t1b = 0.0, t2aa = 0.0, t2ab = 0.0, t2bb = 0.0, t2zz = 0.0;
#pragma unroll
        // (The guard of these sums, and of the two in gt_tables, compiles to an EXEC save + skip branch per step: 60 -> 123 s_cbranch_exec* in the front end, which is
        //  why 5 % fewer vector instructions return 2 %.  Branch-free -- the term loaded unconditionally and selected against +0 -- costs 104 v_cndmask_b32 and measured
        //  0.5 % slower, inside the noise: profiles/r13_wave_front_end.txt, `bf`.  Zero-padded rows of N slots would need neither; they do not fit this LDS.)
        for (int s = 0; s < N; ++s) {   // i = m + s
            if (s < N - mm) {
                const double* pd = PD + 2 * (pair_base + s);
                const double* pq = PQ + 4 * (pair_base + s);
                t1a += pd[0];
                t1b += pd[1];
                t2aa += pq[0];
                t2ab += pq[1];
                t2bb += pq[2];
                t2zz += pq[3];
            }
        }
        const double dzl = (double)(N - 1 - mm);
        t2zz = fma((SQ[2] * SQ[2]) * dzl, dzl, t2zz);
        const double t1z = (double)(((N - mm) * (N - mm - 1)) / 2);
        const double Cm[9] = {ccm, csm, 0.0, -csm, ccm, 0.0, 0.0, 0.0, (double)(mm + 1)};
        const double t1[9] = {t1a, t1b, 0.0, -t1b, t1a, 0.0, 0.0, 0.0, t1z};
        const double t2[9] = {t2aa, t2ab, 0.0, t2ab, t2bb, 0.0, 0.0, 0.0, t2zz};
        de_step<N>(Cm, t1, t2, SQ, dt2, mm, DE + 18 * mm);
    }
    auto gt_tables = [&](const double* vec) {
        // The 3 torque entries of step j are sums over i >= j of dt^2 (C_i - C_j)' (SQ v_i) + dt SQ v_i: the three terms of a pair on ITS lane, from the differences
        // it holds (C_i - C_j = [[a, b, 0], [-b, a, 0], [0, 0, i - j]]: the products with its exact zeros are left out), then 3 N lanes add up their pairs in
        // ascending i.  (Until round 13: 3 N lanes, each an N-step loop of 7 LDS reads, 4 subtractions and 8 multiply-adds.)
        {
            const double* v = vec + 12 * pair_i;
            const double p0 = SQ[0] * v[0], p1 = SQ[1] * v[1], p2 = SQ[2] * v[2], dz = (double)(pair_i - pair_m);
            if (lane < L1::kPairs) {
                // (the multiply-adds written out, the rounding chosen here: inside, the first product fused and the second rounded; outside, dt^2 (...) rounded and
                //  dt (SQ v) fused -- what the N-step loop computed until round 12)
                PQ[4 * lane] = fma(dt, SQ[6] * v[6], dt2 * fma(pair_da, p0, (-pair_db) * p1));
                PQ[4 * lane + 1] = fma(dt, SQ[7] * v[7], dt2 * fma(pair_db, p0, pair_da * p1));
                PQ[4 * lane + 2] = fma(dt, SQ[8] * v[8], dt2 * (dz * p2));
            }
        }
        __syncthreads();
        if (lane < 3 * N) {
            const int j = lane / 3, comp = lane - 3 * j;
            const double* pq = PQ + 4 * ((2 * j < N) ? j * (N + 1) : (N - j) * N) + comp;
            double acc = 0.0;
#pragma unroll
            for (int s = 0; s < N; ++s)   // i = j + s
                if (s < N - j) acc += pq[4 * s];
            GV[9 * j + comp] = acc;
        }
        // The 6 force entries of step j: the plain and the (i - j)-weighted sums over i >= j of one entry of v_i, one lane each, i = j + s ascending
        static_assert(6 * N <= 64, "the force entries of the G'v tables are one trip of the wave");
        if (lane < 6 * N) {
            const int j = lane / 6, comp = 3 + (lane - 6 * j);
            const double* v = vec + 12 * j + ((comp < 6) ? comp : 3 + comp);
            const double winc = (comp < 6) ? 1.0 : 0.0;
            double acc = 0.0, w = (comp < 6) ? 0.0 : 1.0;                            // (double)(i - j), or 1
#pragma unroll
            for (int s = 0; s < N; ++s) {
                if (s < N - j) {
                    double term = w * v[12 * s];
                    asm volatile("" : "+v"(term));                                  // (rounded before it is added, as the loop's select had it: not one multiply-add)
                    acc += term;
                }
                w += winc;
            }
            GV[9 * j + comp] = acc;
        }
    };
    auto gt_eval = [&](int c) -> double {
        const int e = c / 3, ax = c - 3 * e, gc = act[e], j = gc >> 2;
        const double* J = sm + S::o_J + j * 36 + 3 * (gc & 3) + ax;
        const double* g = GV + 9 * j;
        return a.s * (J[0] * g[0] + J[12] * g[1] + J[24] * g[2] + SQ[3 + ax] * dt2m * g[3 + ax] + SQ[9 + ax] * dtm * g[6 + ax]);
    };
    __syncthreads();
    if constexpr (RP != 2) gt_tables(sm + L1::o_eh);
    __syncthreads();
    WSTAMP(a, b, 2);
    if constexpr (RP != 2) for (int c = lane; c < n_eff; c += 64) sm[S::o_q + c] = gt_eval(c);      // (a continued pass: q stays)
    if (RP >= 2 || a.warm_u) {   // P x^0 through the tables; a continued pass: of the x the pass before left (in newtons, one per lane), as a second launch would
        double* TF = sm + L1::o_tf;
        for (int c = lane; c < n_eff; c += 64)
            sm[L1::o_x0c + c] = (RP >= 2 ? park[c] : a.warm_u[(size_t)b * n + 3 * act[c / 3] + (c % 3)]) / a.s;
        __syncthreads();
        for (int tt = lane; tt < 6 * N; tt += 64) {
            const int j = tt / 6, comp = tt - 6 * j;
            double acc = 0.0;
            for (int e = (j ? icnt[j - 1] : 0); e < icnt[j]; ++e) {
                const double* x = sm + L1::o_x0c + 3 * e;
                if (comp < 3) {
                    const double* J = sm + S::o_J + j * 36 + comp * 12 + 3 * (act[e] & 3);
                    acc += J[0] * x[0] + J[1] * x[1] + J[2] * x[2];
                } else {
                    acc += x[comp - 3];
                }
            }
            TF[tt] = acc;
        }
        __syncthreads();
        for (int k = lane; k < n; k += 64) {
            const int i = k / 12, kk = k - 12 * i;
            const double acc = gx_row<N>(CP, TF, i, kk, dt, dt2, dtm, dt2m);
            sm[L1::o_gx + k] = SQ[kk] * a.s * acc;
        }
        __syncthreads();
        gt_tables(sm + L1::o_gx);
        __syncthreads();
        for (int c = lane; c < n_eff; c += 64) sm[S::o_px0 + c] = gt_eval(c) + a.rs2 * sm[L1::o_x0c + c];
    } else {
        for (int c = lane; c < n_eff; c += 64) sm[S::o_px0 + c] = 0.0;
    }

    if constexpr (PHI) {
        double* phi = ws + W::o_phi;
        // the x0 the gradient above was formed with (NOT re-read from the staging array afterwards: the host may already have
        // written the measured state there while this kernel runs)
        const double x0_keep = (lane < 13) ? sm[S::o_x0 + lane] : 0.0;
        for (int kc = 0; kc < 13; ++kc) {
            __syncthreads();
            if (lane < 13) sm[S::o_x0 + lane] = (lane == kc) ? 1.0 : 0.0;
            __syncthreads();
            for (int k = lane; k < n; k += 64) {
                const int i = k / 12, kk = k - 12 * i;
                sm[L1::o_eh + k] = SQ[kk] * free_response<N, L1>(a, sm, i, kk);
            }
            __syncthreads();
            gt_tables(sm + L1::o_eh);
            __syncthreads();
            for (int c = lane; c < n_eff; c += 64) phi[c * 13 + kc] = gt_eval(c);
        }
        __syncthreads();
        if (lane < 13) sm[S::o_x0 + lane] = x0_keep;
        __syncthreads();
    }
    WSTAMP(a, b, 3);
    // ================= K = G'G + R s^2 + sigma + A' rho A: the rank-6 form, every lane its own C-layout entries (srbdqp_common.hpp) ====================
    v4d Kt[NT][NT];
    __syncthreads();   // the inputs / error vector / warm-start vectors under the table rows are dead
    {
        double* AB = sm + L1::o_ab;
        kasm_rows<N>(sm + S::o_J, CP, DE, SQ, act, n_eff, a.s, dt2m, dtm, AB, lane, 64, 16 * NT);
        __syncthreads();
        typedef double d2 __attribute__((ext_vector_type(2)));
        const double dgxy = uni(a.rs2 + a.sigma + 2.0 * rho_b), dgz = uni(a.rs2 + a.sigma + (4.0 * a.mu * a.mu + a.rho_fz) * rho_b);
        // same axis <=> r = c (mod 3); r = 16 ta + kq + 4 q = ta + q + kq, c = 16 tb + mcol = tb + mcol (mod 3): per lane ONE residue decides, per entry a compile-time one
        // (both residues as ONE unsigned division by 3 of a lane constant each; until round 22 a signed one here and one per tile column for the axis of dcol below)
        const int d3 = (int)((unsigned)(mcol - kq + 3) % 3u);
        const int m3 = (int)((unsigned)mcol % 3u);
        const double ind[3] = {d3 == 0 ? 1.0 : 0.0, d3 == 1 ? 1.0 : 0.0, d3 == 2 ? 1.0 : 0.0};
        double eqd[4];                                       // the lane's entry q of a diagonal tile is ON the diagonal
#pragma unroll
        for (int q = 0; q < 4; ++q) eqd[q] = (kq + 4 * q == mcol) ? 1.0 : 0.0;
        double Bv[NT][8], dcol[NT];
#pragma unroll
        for (int tb = 0; tb < NT; ++tb) {
            const int c = 16 * tb + mcol;
            const d2* row = reinterpret_cast<const d2*>(AB + kAbStride * c + 8);
#pragma unroll
            for (int i = 0; i < 4; ++i) { const d2 v = row[i]; Bv[tb][2 * i] = v[0]; Bv[tb][2 * i + 1] = v[1]; }
            dcol[tb] = (c < n_eff) ? ((m3 != (5 - tb % 3) % 3) ? dgxy : dgz) : 1.0;     // (c mod 3 = tb + mcol mod 3 = the axis, z where it is 2; padding -> identity)
        }
#pragma unroll
        for (int ta = 0; ta < NT; ++ta) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = 16 * ta + kq + 4 * q;
                const d2* row = reinterpret_cast<const d2*>(AB + kAbStride * r);
                double Av[8];
#pragma unroll
                for (int i = 0; i < 4; ++i) { const d2 v = row[i]; Av[2 * i] = v[0]; Av[2 * i + 1] = v[1]; }
#pragma unroll
                for (int tb = ta; tb < NT; ++tb) {
                    double v = Av[0] * Bv[tb][0];
#pragma unroll
                    for (int i = 1; i < 6; ++i) v = fma(Av[i], Bv[tb][i], v);
                    const double ft = fma(Av[7], Bv[tb][7], Av[6] * Bv[tb][6]);
                    v = fma(ind[((ta + q - tb) % 3 + 3) % 3], ft, v);
                    if (ta == tb) v = fma(eqd[q], dcol[tb], v);
                    Kt[ta][tb][q] = v;
                }
            }
        }
    }
    __syncthreads();   // the phase-A arrays are dead; the scratch tile is used from here on
    WSTAMP(a, b, 4);
    WSTAMP(a, b, 5);
    if constexpr (DUMP) {   // assembly dump (srbdqp_assemble_f64), see dump_presolved()
        dump_presolved<N>(a, b, n_eff, na, sm + S::o_q, act, [&](auto&& put) {
#pragma unroll
            for (int ta = 0; ta < NT; ++ta)
#pragma unroll
                for (int tb = ta; tb < NT; ++tb)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (16 * ta + kq + 4 * q <= 16 * tb + mcol) put(16 * ta + kq + 4 * q, 16 * tb + mcol, Kt[ta][tb][q]);   // (the upper triangle: put() mirrors it)
        });
        return false;
    }

    // A-operand form of a C-layout tile X (operand[r] at lane (i, k') = X[i][4r + k']): read from the wave-private tile, where diag16_invert_dpp_packed leaves
    // W_jj with row i at PkTile::wrow(i) (the only operand that contracts over its COLUMN index since the W phase went: round 20) -- one lane base, the four reads
    // at immediate offsets.  The identity the inversions start from goes into its tile once, here.
    double* scr = sm + L1::o_scr;
    pk_ident_store(scr, lane);
    const double* const wop = scr + PkTile::wrow(mcol) + kq;
    auto a_operand_read = [&](double (&op)[4]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) op[r] = wop[4 * r];
        asm volatile("" ::: "memory");
    };
    const v4d zero4 = (v4d){0.0, 0.0, 0.0, 0.0};
    // The live size of the LAST block.  Rows and columns KS .. 16 NT - 1 of K are padding for every n_eff <= KS: kasm_rows zeroes the table rows from n_eff up to
    // 16 NT, so K is zero there off the diagonal, and dcol puts 1.0 on it.  F keeps them so: the panel and the trailing update put W_jj * 0 and U' * 0 on those
    // columns, +-0 wherever the operands are finite.  PAD of them (a compile-time value: 4 at N = 10 / MAXS = 2, 8 at N = 4 / MAXS = 2, 0 where KS is a whole number
    // of tiles) make PAD / 4 whole k-steps of every product that contracts over block row NT - 1, and kLastSteps live ones:
    //   the inversion of tile (NT - 1, NT - 1) runs its 16 - PAD real pivots (diag16_invert_dpp_packed<NP>: the padded rows of W stay the identity's, as the full
    //   routine leaves them);
    //   P_{NT-1} = W'W leaves out rows 16 - PAD .. 15 of W: e_i rows, whose products with the real columns are +0 * +0 (the padded diagonal block of
    //   P_{NT-1} comes out 0 where the full product has the identity: positions at or beyond KS in both indices, which no lane's row and no stored K^-1 holds);
    //   in I, Kt[g][NT-1] x Xc[NT-1] leaves out rows 16 - PAD .. 15 of -V_{NT-1,g} = -U_{g,NT-1}' W_gg, which are (+-0)' W_gg = +-0, against rows of X that are
    //   +-0 but for the identity block of P_{NT-1}.
    // Every term left out is +-0 and would be added to an accumulator that is the sum of real terms (or to the zero4 the chain starts from, behind real terms), so
    // no entry in rows and columns below KS changes by a bit unless it is itself an exact zero, whose sign nobody reads (the row masks below, the iterations'
    // products).  Non-finite inputs: a NaN or an infinity in K sits in a real row and column and reaches a real pivot -- of its own tile if that is a diagonal one,
    // of tile (b, b) through the trailing update if it sits in tile (a, b) -- in the arithmetic in front of the products concerned, which is untouched; all_ok sees
    // it as before.  What a skipped k-step no longer does is carry 0 * NaN from a failed tile into K^-1, which the failed QP does not read.
    constexpr int PAD = 16 * NT - W::KS;
    static_assert(PAD >= 0 && PAD < 16, "KS ends inside the last tile");
    constexpr int kLastSteps = 4 - PAD / 4;                  // live k-steps of a contraction over block row NT - 1
    constexpr int kLastPivots = 16 - 4 * (PAD / 4);          // (whole k-steps only: a PAD of 2 would keep its rows)

    // ================= F: K = U'U; on the way out tile (j, j) becomes P_j = W_jj' W_jj (W_jj = L_jj^-1) and tile (j, l > j) becomes -V_lj = -U_jl' W_jj =================
    // (V_lj' = W_jj' U_jl = U_jj^-1 U_jl is all the K^-1 recurrence below needs of block row j: both products contract over the ROW index of their C-layout
    //  operands, so neither leaves the register file, and they hang on nothing the next inversion waits for.  The form that saves them -- U_jj^-1 U_jb = P_j K'_jb
    //  straight from the Schur complement, trailing update K'_ja' (P_j K'_jb), no triangular panel -- forms the Schur complements with S_jj^-1 and loses a factor
    //  kappa: 1e-9 .. 2e-5 relative in K^-1 against 1e-12 .. 1e-10, tests/test_kinv_recurrence_cpu.py.)
    bool all_ok = true;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        bool ok;
        // (the packed DPP elimination, srbdqp_mfma.hpp: no matrix-core instruction and no v_readlane; exact zeros above the diagonal, and W is left in the tile in
        //  the form a_operand stores: the A operand is read straight from it.
        //  Round 35: the first panel tile of the block row, K_{j,j+1}, rides the elimination in the DPP row whose copy of R nobody read, and comes out as
        //  U_{j,j+1} = L_jj^-1 K_{j,j+1} by forward substitution -- the four matrix-core instructions of W_jj K_{j,j+1} are gone, the elimination issues what it
        //  issued.  The tiles further right still take the product with W_jj; the last block row has no panel.)
        const v4d w = (j == NT - 1) ? diag16_invert_dpp_packed<kLastPivots>(Kt[j][j], lane, ok, scr)      // (j is a constant of the unrolled loop)
                                    : diag16_invert_dpp_packed<16, true>(Kt[j][j], lane, ok, scr, &Kt[j][j + 1 < NT ? j + 1 : j]);
        all_ok = all_ok && ok;
        if (j + 1 < NT) {
            if (j + 2 < NT) {
                double wa[4];
                a_operand_read(wa);
#pragma unroll
                for (int bb = j + 2; bb < NT; ++bb) {   // panel: U_jb = L_jj^-1 K_jb
                    v4d o = zero4;
#pragma unroll
                    for (int r = 0; r < 4; ++r) o = mfma_f64(wa[r], Kt[j][bb][r], o);
                    Kt[j][bb] = o;
                }
            }
#pragma unroll
            for (int aa = j + 1; aa < NT; ++aa)      // trailing: K_ab -= U_ja' U_jb
#pragma unroll
                for (int bb = aa; bb < NT; ++bb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) Kt[aa][bb] = mfma_f64(-Kt[j][aa][r], Kt[j][bb][r], Kt[aa][bb]);
#pragma unroll
            for (int l = j + 1; l < NT; ++l) {      // -V_lj = -U_jl' W_jj (U_jl is not needed any more)
                v4d o = zero4;
#pragma unroll
                for (int r = 0; r < 4; ++r) o = mfma_f64(-Kt[j][l][r], w[r], o);
                Kt[j][l] = o;
            }
        }
        v4d pj = zero4;                              // P_j = W_jj' W_jj = S_jj^-1
#pragma unroll
        for (int r = 0; r < (j == NT - 1 ? kLastSteps : 4); ++r) pj = mfma_f64(w[r], w[r], pj);   // (the last block: its live rows alone, see PAD)
        Kt[j][j] = pj;
    }
    if (!all_ok && lane == 0) sm[S::o_misc] = 1.0;
    WSTAMP(a, b, 6);
    WSTAMP(a, b, 7);                                 // (until round 19 behind the W phase, L^-1 block row by block row: gone, stamp 7 = stamp 6)

    // ================= I: X = K^-1 by block recurrence from the factor, U X = L^-1 (block lower-triangular, W_jj on its diagonal): =================
    //     X_jj = P_j - sum_{l>j} V_lj' X_lj,   X_jb = -sum_{l>j} V_lj' X_lb  (b > j),   X_lb = X_bl' for l > b
    // block column by block column from the LAST, each from its diagonal block upwards: column cb forms its blocks (g, cb), g = cb .. 0, in C layout -- NT - 1 - g
    // tile products each, 20 at NT = 4 as W'W took, but with no W phase in front (16 products and three LDS round trips; the six V products of F come back) -- from the
    // blocks below them in the same column.  Those are the column's own down to the diagonal, and below it transposes of blocks an EARLIER (later-numbered) column
    // formed: (l, cb) = (cb, l)' for l > cb.  These wait in registers (Ku: up to five tiles at NT = 4) and go through the staging tiles: stored transposed, read back
    // in C layout.  split: stored as produced, both triangles; fused: one row per lane.
    double kin[W::KS];
    {
        if constexpr (!FUSED) {
            for (int i = lane; i < S::o_R; i += 64) ws[i] = sm[i];
        }
        // fused: one K^-1 row per lane -- the blocks of a column are staged as row-major tiles in the dead phase-A arrays, those below the diagonal transposed (the
        // same store the recurrence reads back), so that lane (g, i) pulls row i of tile g with the same 16-byte reads whichever kind it is (rows 18 doubles apart: with
        // 16 the sixteen lanes of a read pass hit two banks, an 8-way conflict on every one of the 32 reads; the transposed store, 16 lanes of a row 144 bytes
        // apart, is free of conflicts as well).
        double* stg = sm + L1::o_cp;
        static_assert(L1::o_end - L1::o_cp >= NT * L1::kStgTile, "staging of one block column of K^-1");
        [[maybe_unused]] double* kinv = FUSED ? nullptr : ws + W::o_kinv;
        [[maybe_unused]] const int grp = lane >> 4;
        v4d Ku[NT][NT];                                      // Ku[g][c], g < c: block (g, c), from column c to column g
#pragma unroll
        for (int cb = NT - 1; cb >= 0; --cb) {
            v4d Xc[NT];                                      // block (l, cb) in C layout
            asm volatile("" ::: "memory");
#pragma unroll
            for (int l = cb + 1; l < NT; ++l)                // (l, cb) = (cb, l)': row mcol of the staged tile = column mcol of the block
#pragma unroll
                for (int q = 0; q < 4; ++q) stg[l * L1::kStgTile + mcol * L1::kStgRow + kq + 4 * q] = Ku[cb][l][q];
            asm volatile("" ::: "memory");
#pragma unroll
            for (int l = cb + 1; l < NT; ++l)
#pragma unroll
                for (int q = 0; q < 4; ++q) Xc[l][q] = stg[l * L1::kStgTile + (kq + 4 * q) * L1::kStgRow + mcol];
            asm volatile("" ::: "memory");
#pragma unroll
            for (int g = cb; g >= 0; --g) {
                v4d o = (g == cb) ? Kt[cb][cb] : zero4;
#pragma unroll
                for (int l = g + 1; l < NT; ++l)
#pragma unroll
                    for (int r = 0; r < (l == NT - 1 ? kLastSteps : 4); ++r) o = mfma_f64(Kt[g][l][r], Xc[l][r], o);   // (block row NT - 1: its live k-steps, see PAD)
                Xc[g] = o;
                if (g < cb) Ku[g][cb] = o;
                if constexpr (FUSED) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) stg[g * L1::kStgTile + (kq + 4 * q) * L1::kStgRow + mcol] = o[q];
                } else {
                    const int col = 16 * cb + mcol;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int row = 16 * g + kq + 4 * q;
                        if (row < n_eff && col < W::KS) kinv[row * W::KS + col] = (col < n_eff) ? o[q] : 0.0;
                        if (g != cb && col < n_eff && row < W::KS) kinv[col * W::KS + row] = (row < n_eff) ? o[q] : 0.0;
                    }
                }
            }
            if constexpr (FUSED) {
                asm volatile("" ::: "memory");
                const double2* rowp = reinterpret_cast<const double2*>(stg + grp * L1::kStgTile + mcol * L1::kStgRow);
#pragma unroll
                for (int h = 0; h < 8; ++h) {
                    if (16 * cb + 2 * h + 1 < W::KS + 1) {
                        const double2 v = rowp[h];
                        if (16 * cb + 2 * h < W::KS) kin[16 * cb + 2 * h] = v.x;
                        if (16 * cb + 2 * h + 1 < W::KS) kin[16 * cb + 2 * h + 1] = v.y;
                    }
                }
                asm volatile("" ::: "memory");
            }
        }
    }
    if constexpr (FUSED) {
        // The lane's K^-1 row is masked to the presolved block only where there is something to mask (wave-uniform: n_eff comes out of LDS, the same for every
        // lane).  With n_eff == KS (configs[1]: 60 of 60) the column test holds for every c, and the row test concerns lanes KS..63 alone: their entries are
        // K^-1 between a padded and a real variable -- K has zero rows (kasm_rows) and an identity diagonal (dcol) there, F, W and I reach those positions only
        // through products with exact zeros -- and the iterations read neither the right-hand side nor any maximum of a lane past KS.  ~120 v_cndmask_b32 per pass.
        if (__builtin_amdgcn_readfirstlane(n_eff) < W::KS) {
#pragma unroll
            for (int c = 0; c < W::KS; ++c) kin[c] = (lane < n_eff && c < n_eff) ? kin[c] : 0.0;
        }
        __syncthreads();
        WSTAMP(a, b, 8);
        WSTAMP(a, b, 9);
        static_assert(L1::o_end >= SplitSmem<N, MAXS>::o_end, "the ADMM body's vectors live in this kernel's LDS");
        if constexpr (RP == 0) {
            admm_wave_body<N, MAXS>(a, b, rho_b, sm, kin);
        } else {
            WaveRestart rs;
            const int left = a.max_iter - rs_done;                                   // the cap is on the total
            rs.pass = rs_pass;
            rs.more = rs_pass < a.restart_max && a.restart_every < left;
            rs.kcap = rs.more ? a.restart_every : left;
            rs.park = park;
            int status = -1, iters = 0;
            admm_wave_iterations<N, MAXS, true>(a, io, RP == 1 ? a.warm_u : nullptr, RP == 1 ? a.warm_y : nullptr, b, rho_b, sm, kin, sm + SplitSmem<N, MAXS>::o_xs,
                                                status, iters, &rs);
            rs_done += iters;
            if (status == 2 && rs.more) {   // (wave-uniform) at the mark, not converged: another pass
                rho_b = restart_rho_of(rho_b, rs.v);
                ++rs_pass;
                __syncthreads();
                return true;
            }
            admm_wave_finish<N, MAXS>(a, io, b, sm, status, rs_done);
        }
        WSTAMP(a, b, 10);
        WSTAMP(a, b, 11);
        WSTAMP_RT(a, b, 13);
    }
    return false;
}

template <int N, int MAXS, bool FUSED, bool DUMP = false, bool PHI = false, bool RST = false>
__global__ __launch_bounds__(64, 2) void srbdqp_setup1_kernel(KArgs a) {
    static_assert(!(PHI && FUSED), "dq/dx0 is a hand-over of the split pipeline");
    static_assert(!RST || (FUSED && !DUMP), "the restart in place belongs to the fused solve");
    static_assert(Setup1Smem<N, MAXS>::supported, "one wave holds all tiles: at most 4 x 4 tiles");
    static_assert(4 * N <= 64, "one ballot compacts the contact flags");
    extern __shared__ __attribute__((aligned(16))) double sm[];
    if ((int)blockIdx.x >= a.B) return;
    if (a.count_ptr && (int)blockIdx.x >= *a.count_ptr) return;
    const int b = SRBDQP_QP_INDEX(a);
    if (SRBDQP_RESTART_SKIP(a, b)) return;
    double rho_b = SRBDQP_RHO_OF(a, b);
    int rs_pass = 0, rs_done = 0;
    const QpIo io = io_of(a);
    if constexpr (!RST) {
        setup1_pass<N, MAXS, FUSED, DUMP, PHI, 0>(a, io, b, sm, rho_b, rs_pass, rs_done);
    } else {
        // (round 5: the continued passes as three straight copies instead of a loop -- a loop around the body has the compiler hoist the body's index arithmetic and
        //  constants in front of it and keep them live through it: 256 VGPRs + 52 bytes of scratch at N = 10.  Exact for rho_restart_count <= 3; with more
        //  re-balancings allowed the third continued pass runs on to the iteration cap)
        bool again = setup1_pass<N, MAXS, FUSED, DUMP, PHI, 1>(a, io, b, sm, rho_b, rs_pass, rs_done);
        if (!again) return;
        again = setup1_pass<N, MAXS, FUSED, DUMP, PHI, 2>(a, io, b, sm, rho_b, rs_pass, rs_done);
        if (!again) return;
        again = setup1_pass<N, MAXS, FUSED, DUMP, PHI, 2>(a, io, b, sm, rho_b, rs_pass, rs_done);
        if (!again) return;
        KArgs al = a;
        al.restart_max = 0;
        setup1_pass<N, MAXS, FUSED, DUMP, PHI, 2>(al, io, b, sm, rho_b, rs_pass, rs_done);
    }
}

// ---- deferred tails (SRBDQP_FLAG_DEFER_TAIL) --------------------------------------------------------------------------------------------------------------
// A launch of the restart kernel above lasts as long as its slowest QP: up to three set-ups and 250 iterations on one wave (0.24 ms alone on the device, when
// the bulk of 4096 QPs is done after 0.12 ms) -- which is why the step rate of round 3 leaned on a longest-first dispatch hint and on a second stream.  Here no
// workgroup runs more than ONE pass: a QP that reaches a restart mark unconverged parks (x, y), re-balances its rho and appends itself -- with the pointers
// of its own launch -- to a list in HBM; the first tail_wgs workgroups of the NEXT launch on the same stream (another batch, other buffers) each take one record,
// rebuild the strip from the QP's inputs and run its next pass.  Same passes, same arithmetic, same statuses and iteration counts as the restart in place; the
// outputs of a deferred QP arrive one or two launches later (status[] says SRBDQP_PENDING until then; srbdqp_flush() runs what is left).  No loop around the
// body anywhere: both arms are straight-line code.
__device__ __forceinline__ unsigned long long unis_u64(unsigned long long v) {
    int lo, hi;
    asm volatile("s_nop 1\n\tv_readfirstlane_b32 %0, %2\n\tv_readfirstlane_b32 %1, %3" : "=s"(lo), "=s"(hi) : "v"((int)(unsigned)v), "v"((int)(unsigned)(v >> 32)));
    return ((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo;
}
template <typename T> __device__ __forceinline__ T* unis_ptr(T* p) { return reinterpret_cast<T*>(unis_u64(reinterpret_cast<unsigned long long>(p))); }

// a free record of the list this launch appends to, or null: the list is full (round 5: the lists are sized for a quarter of a launch's QPs, not for all of them
// three times over; the count may run past tail_cap -- the reader clamps it -- and a QP that finds no room runs its remaining passes in place)
__device__ __forceinline__ double* tail_claim(const KArgs& a) {
    int slot = 0;
    if (threadIdx.x == 0) slot = atomicAdd(a.tail_cnt + a.tail_iout, 1);
    slot = __builtin_amdgcn_readfirstlane(slot);
    if (slot >= a.tail_cap) return nullptr;
    return reinterpret_cast<double*>(a.tail_lists) + ((size_t)a.tail_iout * (size_t)a.tail_cap + (size_t)slot) * kTailRecDoubles;
}

__device__ __forceinline__ bool tail_export(const KArgs& a, const QpIo& io, int b, double rho_b, int rs_pass, int rs_done, const double* park) {
    const int lane = threadIdx.x;
    double* rec = tail_claim(a);
    if (!rec) return false;
    if (lane == 0) {
        TailRecHead* hd = reinterpret_cast<TailRecHead*>(rec);
        hd->b = b; hd->pass = rs_pass; hd->done = rs_done; hd->pad = 0; hd->rho = rho_b; hd->io = io;
        if (io.status) io.status[b] = kStatusPending;
    }
    rec[16 + lane] = park[lane]; rec[80 + lane] = park[64 + lane]; rec[144 + lane] = park[128 + lane];
    return true;
}

// FLUSH: the continuations alone (srbdqp_flush: a launch with no QPs of its own; a kernel of its own name, so that profiles keep the two apart).  Nothing comes
// behind a flush that could pick a record up, so here a workgroup runs ALL the passes its QP has left, the later ones in place as the restart kernel does (the
// loop's hoisted registers cost this instantiation only): one flush launch instead of rho_restart_count of them.
template <int N, int MAXS, bool FLUSH = false>
__global__ __launch_bounds__(64, 2) void srbdqp_wave_defer_kernel(KArgs a) {
    static_assert(Setup1Smem<N, MAXS>::supported && 4 * N <= 64, "the one-wave kernel's limits");
    extern __shared__ __attribute__((aligned(16))) double sm[];
    using L1 = Setup1Smem<N, MAXS>;
    const int lane = threadIdx.x;
    const int T = a.tail_wgs;
    double* const park = sm + L1::o_end;
    // the passes a QP has left, in place: three straight copies of the body (see below), in each arm on its own -- the arms share nothing, so that the first passes
    // (96 % of the workgroups) run the code they ran before there was an overflow path
    auto in_place = [&](const QpIo& io, const int b, double rho_b, int rs_pass, int rs_done) __attribute__((always_inline)) {
        bool again = setup1_pass<N, MAXS, true, false, false, 2>(a, io, b, sm, rho_b, rs_pass, rs_done);
        if (!again) return;
        again = setup1_pass<N, MAXS, true, false, false, 2>(a, io, b, sm, rho_b, rs_pass, rs_done);
        if (!again) return;
        KArgs al = a;
        al.restart_max = 0;
        setup1_pass<N, MAXS, true, false, false, 2>(al, io, b, sm, rho_b, rs_pass, rs_done);
    };
    if ((int)blockIdx.x < T) {
        // ---- a continuation of an earlier launch (first in the grid: these are the long ones)
        const int i = blockIdx.x;
        int cnt = a.tail_cnt[a.tail_iin];
        cnt = cnt < a.tail_cap ? cnt : a.tail_cap;                                          // (claims past the end of a full list found no room: tail_claim)
        if (i == 0 && lane == 0) a.tail_cnt[a.tail_izero] = 0;                             // the list the NEXT launch appends to
        // (cnt <= T: the host launches one tail workgroup per record the list can hold -- a bound it knows, srbdqp.hip launch_wave_defer)
        const double* lin = reinterpret_cast<const double*>(a.tail_lists) + (size_t)a.tail_iin * (size_t)a.tail_cap * kTailRecDoubles;
        if (i >= cnt) return;
        const double* rec = lin + (size_t)i * kTailRecDoubles;
        const TailRecHead* hd = reinterpret_cast<const TailRecHead*>(rec);
        QpIo io;
        io.x0 = unis_ptr(hd->io.x0); io.xref = unis_ptr(hd->io.xref); io.foot = unis_ptr(hd->io.foot); io.pcom = unis_ptr(hd->io.pcom);
        io.contact = unis_ptr(hd->io.contact); io.u_out = unis_ptr(hd->io.u_out); io.x_out = unis_ptr(hd->io.x_out); io.y_out = unis_ptr(hd->io.y_out);
        io.status = unis_ptr(hd->io.status); io.iters = unis_ptr(hd->io.iters);
        const int b = __builtin_amdgcn_readfirstlane(hd->b);
        int rs_pass = __builtin_amdgcn_readfirstlane(hd->pass), rs_done = __builtin_amdgcn_readfirstlane(hd->done);
        double rho_b = unis(hd->rho);
        park[lane] = rec[16 + lane]; park[64 + lane] = rec[80 + lane]; park[128 + lane] = rec[144 + lane];
        __syncthreads();
        if (!setup1_pass<N, MAXS, true, false, false, 3>(a, io, b, sm, rho_b, rs_pass, rs_done)) return;
        // at a mark, unconverged: on to the next launch on the stream -- or, when the list has no room left (or nothing comes behind a flush), the passes it has left
        // in place, as the restart kernel runs them (the strip is in place by now).  Same passes, same arithmetic either way.
        if constexpr (!FLUSH) { if (tail_export(a, io, b, rho_b, rs_pass, rs_done, park)) return; }
        in_place(io, b, rho_b, rs_pass, rs_done);
    } else if constexpr (!FLUSH) {
        // ---- a QP of this launch: its first pass
        const int wg = (int)blockIdx.x - T;
        if (wg >= a.B) return;
        const int b = a.perm ? a.perm[wg] : wg;
        double rho_b = a.rho_qp ? a.rho_qp[b] : a.rho;
        int rs_pass = 0, rs_done = 0;
        const QpIo io = io_of(a);
        if (!setup1_pass<N, MAXS, true, false, false, 1>(a, io, b, sm, rho_b, rs_pass, rs_done)) return;
        if (tail_export(a, io, b, rho_b, rs_pass, rs_done, park)) return;
        // The list is full (rare: the lists hold a quarter of a launch).  In place, but NOT as a loop: a loop around the body has the compiler hoist the body's index
        // arithmetic and constants in front of it and keep them live through it (256 VGPRs + 72 bytes of scratch for the whole kernel) -- three straight copies
        // instead, which cover rho_restart_count <= 3 exactly (values above 3 mean 3: srbdqp.h).
        in_place(io, b, rho_b, rs_pass, rs_done);
    }
}

}  // namespace srbdqp
