// srbdqp_wrench_lat_ew.hip -- the low-latency side-input instantiations of the general kernel in a code object of their own: MODE 7 (the staged wrench calls:
// srbdqp_solve_staged_wrench_f64, srbdqp_update_wrench_f64) and MODE 4 (the staged normals calls: srbdqp_solve_staged_normals_f64, srbdqp_update_normals_f64);
// srbdqp_wrench_lat_ew.hpp says why.  Host side: one launcher over the mode.
#include <hip/hip_runtime.h>

#include <cstring>
#include <utility>

#include "srbdqp.h"
#include "srbdqp_common.hpp"
#include "srbdqp_wrench.hpp"
#include "srbdqp_wrench_lat_ew.hpp"
#include "srbdqp_fleet.hpp"
#include "srbdqp_observer.hpp"

namespace srbdqp {
namespace {

// what differs between the two modes: the grid kernel, its *_in twin, the struct that carries the side input of one QP in the argument segment, the doubles
// kept behind the layout
template <int MODE> struct LatSide;
template <> struct LatSide<kModeExtWrench> {           // the wrench's rows for the roll-out behind the mode's slots
    template <int N> using Arg = StagedWrench<N>;
    template <int N, int XW> static constexpr auto grid() { return &srbdqp_wrench_ew_lat_kernel<N, XW>; }
    template <int N, int XW> static constexpr auto in() { return &srbdqp_wrench_ew_lat_kernel_in<N, XW>; }
    static constexpr int xd(int N) { return wrench_lat_ew_xd(N); }
};
template <> struct LatSide<kModeNormals> {             // the table L in the persistent strip; no doubles behind the layout
    template <int N> using Arg = StagedNormals<N>;
    template <int N, int XW> static constexpr auto grid() { return &srbdqp_wrench_cn_lat_kernel<N, XW>; }
    template <int N, int XW> static constexpr auto in() { return &srbdqp_wrench_cn_lat_kernel_in<N, XW>; }
    static constexpr int xd(int) { static_assert(WrenchMode<kModeNormals>::xd == 0); return 0; }
};

// the waves and the pipeline of the plain call's low-latency instantiation (srbdqp.hip launch_wrench_t) on the layout of MODE
template <int N, int MODE>
hipError_t launch_t(bool set_attr, const KArgs& a, const void* in, const double* side_host, const double* side_dev, hipStream_t st) {
    using M = LatSide<MODE>;
    constexpr int XW = (N >= 8) ? 2 : 1;
    using SL = WrenchLayout<N, MODE, 8, 5, XW>;
    constexpr size_t lds = SL::bytes + M::xd(N) * sizeof(double);
    static_assert(lds <= 163840 && SL::BT == WrenchSmem<N, 8, 5, XW>::BT, "one QP must fit the LDS of a CU");
    if (!in) {
        auto k = M::template grid<N, XW>();
        if (set_attr) if (const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) return e;
        hipLaunchKernelGGL(k, dim3((unsigned)a.B), dim3(SL::BT), lds, st, a, side_dev);
        return hipGetLastError();
    }
    auto k = M::template in<N, XW>();
    if (set_attr) if (const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) return e;
    typename M::template Arg<N> side;
    std::memcpy(&side, side_host, sizeof(side));
    hipLaunchKernelGGL(k, dim3(1), dim3(SL::BT), lds, st, a, *static_cast<const StagedIn<N>*>(in), side);
    return hipGetLastError();
}

template <int MODE>
hipError_t launch_n(int N, bool set_attr, const KArgs& a, const void* in, const double* side_host, const double* side_dev, hipStream_t st) {
    if (N == 4) return launch_t<4, MODE>(set_attr, a, in, side_host, side_dev, st);
    if (N == 8) return launch_t<8, MODE>(set_attr, a, in, side_host, side_dev, st);
    if (N == 10) return launch_t<10, MODE>(set_attr, a, in, side_host, side_dev, st);
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_wrench_side_lat(int mode, int N, bool set_attr, const KArgs& a, const void* in, const double* side_host, const double* side_dev, hipStream_t st) {
    if (mode == kModeExtWrench) return launch_n<kModeExtWrench>(N, set_attr, a, in, side_host, side_dev, st);   // (the wrench's kernels first: the order of the code object)
    if (mode == kModeNormals) return launch_n<kModeNormals>(N, set_attr, a, in, side_host, side_dev, st);
    return hipErrorInvalidValue;
}

// The fleet's plant step (srbdqp_fleet.hpp) is instantiated here too, behind the low-latency kernels, for their reason: srbdqp.hip's code object stays what it
// was, and the library keeps its two code objects (tests/test_staged_side_cpu.py counts them).
hipError_t launch_fleet_advance(const FleetArgs& a, hipStream_t st, const TerrainMap* map, const double* landing_yaw) {
    const long long tiles = (a.B + kFleetTile - 1) / kFleetTile;   // one tile of 64 robots per workgroup pass
    const dim3 grid((unsigned)(tiles < 1 ? 1 : (tiles > 256 * 32 ? 256 * 32 : tiles)));
    if (landing_yaw) {   // the steered instantiations: heel and toe turned by the landing's heading
        const FleetSteer steer{landing_yaw};
        if (map) hipLaunchKernelGGL((srbdqp_fleet_advance_kernel<kFleetTile, TerrainMap, FleetSteer>), grid, dim3(kFleetTile), 0, st, a, *map, steer);
        else hipLaunchKernelGGL((srbdqp_fleet_advance_kernel<kFleetTile, FleetSteer>), grid, dim3(kFleetTile), 0, st, a, steer);
    } else if (map) hipLaunchKernelGGL((srbdqp_fleet_advance_kernel<kFleetTile, TerrainMap>), grid, dim3(kFleetTile), 0, st, a, *map);
    else hipLaunchKernelGGL(srbdqp_fleet_advance_kernel<kFleetTile>, grid, dim3(kFleetTile), 0, st, a);
    return hipGetLastError();
}

// ... the momentum observer behind it (srbdqp_observer.hpp): the push a period's forces do not explain, as the external wrench of the next solve
hipError_t launch_wrench_observer(const ObserverArgs& a, hipStream_t st) {
    const long long tiles = (a.B + kObserverTile - 1) / kObserverTile;   // one tile of 64 robots per workgroup pass
    const dim3 grid((unsigned)(tiles < 1 ? 1 : (tiles > 256 * 32 ? 256 * 32 : tiles)));
    hipLaunchKernelGGL(srbdqp_wrench_observer_kernel<kObserverTile>, grid, dim3(kObserverTile), 0, st, a);
    return hipGetLastError();
}

// ... and the two kernels of the ground under it (srbdqp_terrain.hpp): the sample of the map at M points, the normals and the height reference of B robots
hipError_t launch_terrain_sample(const TerrainSampleArgs& a, hipStream_t st) {
    const long long want = (a.M + 255) / 256;                      // grid-stride: enough 256-thread workgroups to fill 256 CUs several times over, no more
    hipLaunchKernelGGL(srbdqp_terrain_sample_kernel<256>, dim3((unsigned)(want < 1 ? 1 : (want > 256 * 16 ? 256 * 16 : want))), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_terrain_inputs(const TerrainInputsArgs& a, hipStream_t st) {
    const long long tiles = (a.B + kTerrainTile - 1) / kTerrainTile;   // one tile of 32 robots per workgroup pass
    const dim3 grid((unsigned)(tiles < 1 ? 1 : (tiles > 256 * 32 ? 256 * 32 : tiles)));
    hipLaunchKernelGGL(srbdqp_terrain_inputs_kernel<kTerrainTile>, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

// ... and the step before the QP of a fleet that steers or follows its path (srbdqp_steer.hpp; DESIGN.md sections 20, 21), behind every other kernel of this
// code object, which keeps their order: one instantiation per tabulated horizon and the live one, with track... empty (steered) or one TrackPose (tracked)
namespace {
template <int... Ns, class... TRACK>
hipError_t launch_commanded(std::integer_sequence<int, Ns...>, const SteerInputsArgs& a, bool live, hipStream_t st, const TRACK&... track) {
    const long long tiles = (a.B + 31) / 32;                       // one tile of 32 robots per workgroup pass
    const dim3 grid((unsigned)(tiles < 1 ? 1 : (tiles > 256 * 32 ? 256 * 32 : tiles)));
    if (a.N < 1 || a.N > kSteerSteps - 1) return hipErrorInvalidValue;   // (a table holds 25 entries a robot)
    auto go = [&](auto n) { hipLaunchKernelGGL((srbdqp_mpc_inputs_commanded_kernel<decltype(n)::value, TRACK...>), grid, dim3(256), 0, st, a, track...); return true; };
    if (live || !((a.N == Ns && go(std::integral_constant<int, Ns>{})) || ...)) go(std::integral_constant<int, 0>{});   // (a live or untabulated horizon: a.N at run time)
    return hipGetLastError();
}
}  // namespace

hipError_t launch_mpc_inputs_commanded(const SteerInputsArgs& a, const TrackPose* track, bool live, hipStream_t st, const PreviewFeet* preview) {
    using Tabulated = std::integer_sequence<int, 4, 8, 10, 12, 16, 20, 24>;
    // (the previewed instantiations, DESIGN.md section 22, stand behind the plain ones of their form)
    if (preview) return track ? launch_commanded(Tabulated{}, a, live, st, *track, *preview) : launch_commanded(Tabulated{}, a, live, st, *preview);
    return track ? launch_commanded(Tabulated{}, a, live, st, *track) : launch_commanded(Tabulated{}, a, live, st);
}

// ... and the ground under footholds that differ from step to step, those of srbdqp_mpc_inputs_previewed_* (srbdqp_terrain.hpp)
hipError_t launch_terrain_inputs_previewed(const TerrainPreviewArgs& a, hipStream_t st) {
    if (a.N < 1 || a.N > 24) return hipErrorInvalidValue;             // (the kernel's table of heights holds 24 steps a robot)
    const long long tiles = (a.B + kTerrainTile - 1) / kTerrainTile;
    const dim3 grid((unsigned)(tiles < 1 ? 1 : (tiles > 256 * 32 ? 256 * 32 : tiles)));
    hipLaunchKernelGGL(srbdqp_terrain_inputs_previewed_kernel<kTerrainTile>, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace srbdqp
