// A host build of the momentum observer's two functions (g1_locomotion_amd/csrc/srbdqp_observer.hpp), stand-alone: tests/test_observer_cpu.py compiles this
// file with a host compiler, feeds it cases on standard input and holds what it prints against tests/observer_twin.py.
//   input:  mass, inertia[3], dt, gain, torque_max, force_max, the number of cases; per case x0[13], x1[13], p[12], f[12], w_est[6]
//   output: per case one line of w_meas[6] and one of w_est'[6], %.17g
#include <cstdio>

#include "srbdqp_observer.hpp"

static bool read(double* v, int n) {
    for (int i = 0; i < n; ++i) if (std::scanf("%lf", v + i) != 1) return false;
    return true;
}

int main() {
    double mass, inertia[3], dt, gain, tmax, fmax, cases;
    if (!read(&mass, 1) || !read(inertia, 3) || !read(&dt, 1) || !read(&gain, 1) || !read(&tmax, 1) || !read(&fmax, 1) || !read(&cases, 1)) return 2;
    for (int c = 0; c < (int)cases; ++c) {
        double x0[13], x1[13], p[12], f[12], we[6], wm[6];
        if (!read(x0, 13) || !read(x1, 13) || !read(p, 12) || !read(f, 12) || !read(we, 6)) return 3;
        srbdqp::observer_measure(mass, inertia, dt, x0, x1, p, f, wm);
        srbdqp::observer_update(gain, tmax, fmax, wm, we);
        for (int i = 0; i < 6; ++i) std::printf("%.17g%c", wm[i], i == 5 ? '\n' : ' ');
        for (int i = 0; i < 6; ++i) std::printf("%.17g%c", we[i], i == 5 ? '\n' : ' ');
    }
    return 0;
}
