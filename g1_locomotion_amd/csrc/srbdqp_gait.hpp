// The gait schedule of the cascade (include/srbdqp_cascade.h, srbdqp_gait): fixed-period alternating single support with a double-support overlap, as
// msgs.AlternatingGait.contact_horizon has it.  One definition for every kernel that asks which foot stands: srbdqp_mpc_inputs_kernel (srbdqp_cascade.hpp) fills
// its contact horizon from it, srbdqp_fleet_advance_kernel (srbdqp_fleet.hpp) finds the touchdowns with it.
#pragma once
#include <hip/hip_runtime.h>

namespace srbdqp {

// phase of the horizon's step 0 in [0, 2 period): the gait's clock is the step index floor(stamp / dt + 1e-9)
__device__ __forceinline__ int gait_phase0(double stamp, double dt, int period) {
#pragma clang fp contract(off)   // compared bit for bit with the host's stamp / dt + 1e-9
    const long long k0 = (long long)floor(stamp / dt + 1e-9);
    long long ph = k0 % (2LL * period);
    if (ph < 0) ph += 2LL * period;
    return (int)ph;
}

// stance flags of the left (cl) and the right (cr) foot k steps behind phase p0; p0 < 0: standing, both feet down
__device__ __forceinline__ void gait_flags(int p0, int k, int period, int ds, bool& cl, bool& cr) {
    const int ph = (p0 + k) % (2 * period);
    const bool stand = p0 < 0, left_stance = ph < period, dsup = (ph % period) < ds;
    cl = stand || left_stance || dsup; cr = stand || !left_stance || dsup;
}

}  // namespace srbdqp
