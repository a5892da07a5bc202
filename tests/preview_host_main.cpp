// A host build of the foothold preview's arithmetic (g1_locomotion_amd/csrc/srbdqp_steer.hpp: preview_lands, preview_touchdown, preview_foothold beside
// steer_table, steer_landing and steer_touchdown), stand-alone: tests/test_preview_cpu.py compiles this file with a host compiler, feeds it cases on standard
// input and holds what it prints against tests/preview_twin.py.
//   input:  mode.
//           mode 0: the number of cases; per case P ds p0 N (p0 = -1: standing)
//           mode 1: dt, N, P, ds, hip_offset_y, foot_half_length, the number of cases; per case p0, x0[13], command[3]
//   output: mode 0: per case N lines "lands left right": the foot that lands at step k, the latest touchdown steps of the two feet up to k
//           mode 1: per case one line "lx ly landing_yaw heel_x heel_y toe_x toe_y" -- the landing point of the call and the touchdown the plant makes of it --
//                   then N lines "lands heel_x heel_y toe_x toe_y psi_l" for k = 0 ... N - 1 (zeros where no foot lands), %.17g
#include <cstdio>

#include "srbdqp_steer.hpp"

static bool read(double* v, int n) {
    for (int i = 0; i < n; ++i) if (std::scanf("%lf", v + i) != 1) return false;
    return true;
}

int main() {
    double mode;
    if (!read(&mode, 1)) return 2;
    if ((int)mode == 0) {
        double cases;
        if (!read(&cases, 1)) return 2;
        for (int c = 0; c < (int)cases; ++c) {
            double q[4];
            if (!read(q, 4)) return 3;
            const int P = (int)q[0], ds = (int)q[1], p0 = (int)q[2], N = (int)q[3];
            for (int k = 0; k < N; ++k)
                std::printf("%d %d %d\n", srbdqp::preview_lands(p0, k, P, ds), srbdqp::preview_touchdown(p0, k, P, ds, false), srbdqp::preview_touchdown(p0, k, P, ds, true));
        }
        return 0;
    }
    double head[7];
    if (!read(head, 7)) return 2;
    const double dt = head[0], hip = head[4], half = head[5];
    const int N = (int)head[1], P = (int)head[2], ds = (int)head[3];
    if (N < 1 || N > srbdqp::kSteerSteps - 1 || P < 1) return 2;
    const double half_T = 0.5 * ((double)P * dt);
    for (int c = 0; c < (int)head[6]; ++c) {
        double ph, x0[13], cmd[3];
        double px[srbdqp::kSteerSteps], py[srbdqp::kSteerSteps], vx[srbdqp::kSteerSteps], vy[srbdqp::kSteerSteps];
        if (!read(&ph, 1) || !read(x0, 13) || !read(cmd, 3)) return 3;
        const int p0 = (int)ph;
        const double wz = cmd[2];
        srbdqp::steer_table(x0[2], x0[3], x0[4], cmd[0], cmd[1], wz, dt, N, px, py, vx, vy);
        {   // the call's own landing point, as the kernel computes it, and the plant's touchdown of it
            const int ph0 = p0 < 0 ? 0 : p0 % (2 * P);
            const bool cl = p0 < 0 || ph0 < P || (ph0 % P) < ds;
            const double psi_l = x0[2] + wz * half_T;
            double lx, ly, heel[2], toe[2];
            srbdqp::steer_landing(x0, psi_l, cl ? -1.0 : 1.0, hip, half_T, vx[0], vy[0], lx, ly);
            srbdqp::steer_touchdown(lx, ly, half, psi_l, heel, toe);
            std::printf("%.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", lx, ly, psi_l, heel[0], heel[1], toe[0], toe[1]);
        }
        for (int k = 0; k < N; ++k) {
            const int lands = srbdqp::preview_lands(p0, k, P, ds);
            double heel[2] = {0.0, 0.0}, toe[2] = {0.0, 0.0}, psi_l = 0.0;
            if (lands) {
                const bool now = k == 1;
                const double psi = now ? x0[2] : srbdqp::steer_yaw(x0[2], wz, (double)(k - 1), dt);
                srbdqp::preview_foothold(psi, px[k - 1], py[k - 1], now ? x0[9] : vx[k - 1], now ? x0[10] : vy[k - 1], vx[k - 1], vy[k - 1], wz, lands == 1 ? 1.0 : -1.0,
                                         hip, half_T, half, heel, toe, psi_l);
            }
            std::printf("%d %.17g %.17g %.17g %.17g %.17g\n", lands, heel[0], heel[1], toe[0], toe[1], psi_l);
        }
    }
    return 0;
}
