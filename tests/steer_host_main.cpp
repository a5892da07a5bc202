// A host build of the steering arithmetic (g1_locomotion_amd/csrc/srbdqp_steer.hpp), stand-alone: tests/test_steer_cpu.py compiles this file with a host
// compiler, feeds it cases on standard input and holds what it prints against tests/steer_twin.py.
//   input:  dt, N, hip_offset_y, half_T, foot_half_length, the number of cases; per case x0[13], command[3], side
//   output: per case N + 1 lines of px py vwx vwy, then one line of landing_x landing_y psi_L heel_x heel_y toe_x toe_y, %.17g
#include <cstdio>

#include "srbdqp_steer.hpp"

static bool read(double* v, int n) {
    for (int i = 0; i < n; ++i) if (std::scanf("%lf", v + i) != 1) return false;
    return true;
}

int main() {
    double dt, horizon, hip, half_T, half, cases;
    if (!read(&dt, 1) || !read(&horizon, 1) || !read(&hip, 1) || !read(&half_T, 1) || !read(&half, 1) || !read(&cases, 1)) return 2;
    const int N = (int)horizon;
    if (N < 1 || N > srbdqp::kSteerSteps - 1) return 2;
    for (int c = 0; c < (int)cases; ++c) {
        double x0[13], cmd[3], side;
        double px[srbdqp::kSteerSteps], py[srbdqp::kSteerSteps], vx[srbdqp::kSteerSteps], vy[srbdqp::kSteerSteps];
        if (!read(x0, 13) || !read(cmd, 3) || !read(&side, 1)) return 3;
        srbdqp::steer_table(x0[2], x0[3], x0[4], cmd[0], cmd[1], cmd[2], dt, N, px, py, vx, vy);
        for (int k = 0; k <= N; ++k) std::printf("%.17g %.17g %.17g %.17g\n", px[k], py[k], vx[k], vy[k]);
        const double psi_l = x0[2] + cmd[2] * half_T;
        double lx, ly, heel[2], toe[2];
        srbdqp::steer_landing(x0, psi_l, side, hip, half_T, vx[0], vy[0], lx, ly);
        srbdqp::steer_touchdown(lx, ly, half, psi_l, heel, toe);
        std::printf("%.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", lx, ly, psi_l, heel[0], heel[1], toe[0], toe[1]);
    }
    return 0;
}
