// The ground under a fleet (include/srbdqp_cascade.h, srbdqp_set_terrain): a height map on a regular grid, the sample S(x, y) -> (z, n)
// of it -- ONE definition, terrain_sample() below, which the sample kernel, the inputs kernel and the terrain instantiation of the plant step (srbdqp_fleet.hpp)
// all inline, and which tests/terrain_twin.py follows operation for operation -- and the two kernels that hand it to a caller and to the solve.
//
// The kernels are templates so that they are emitted only where they are instantiated: in srbdqp_wrench_lat_ew.hip, the library's second code object, beside the
// plant step.  srbdqp.hip sees the argument structures and the launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace srbdqp {

struct TerrainMap {
    const double* h;         // [ny][nx], x fastest: node (i, j) at (x0 + i cell, y0 + j cell)
    int32_t nx, ny;          // >= 2 each
    double x0, y0, cell;
};

// S(x, y): bilinear height and the unit normal of the bilinear patch at the point, every line one rounded operation in the order of include/srbdqp_cascade.h (no
// fused multiply-add: z is compared bit for bit with the twin; the division and the square root are IEEE operations of the target, not pinned by the pragma).  A
// point off the map is the clamped point; a coordinate that is not finite gives z = NaN on flat ground.
__host__ __device__ __forceinline__ void terrain_sample(const TerrainMap& m, double x, double y, double& z, double (&n)[3]) {
#pragma clang fp contract(off)
    if (!(isfinite(x) && isfinite(y))) { z = __builtin_nan(""); n[0] = 0.0; n[1] = 0.0; n[2] = 1.0; return; }
    const double umax = (double)(m.nx - 1), vmax = (double)(m.ny - 1);
    double u = (x - m.x0) / m.cell, v = (y - m.y0) / m.cell;
    u = u < 0.0 ? 0.0 : (u > umax ? umax : u);
    v = v < 0.0 ? 0.0 : (v > vmax ? vmax : v);
    int i = (int)floor(u), j = (int)floor(v);
    i = i > m.nx - 2 ? m.nx - 2 : i;
    j = j > m.ny - 2 ? m.ny - 2 : j;
    const double fx = u - (double)i, fy = v - (double)j;
    const double* r0 = m.h + (size_t)j * (size_t)m.nx + (size_t)i;   // two pairs of neighbouring doubles
    const double* r1 = r0 + m.nx;
    const double h00 = r0[0], h10 = r0[1], h01 = r1[0], h11 = r1[1];
    const double dx0 = h10 - h00, dx1 = h11 - h01, dy0 = h01 - h00, dy1 = h11 - h10;
    const double a = h00 + fx * dx0, b = h01 + fx * dx1;
    z = a + fy * (b - a);
    const double gx = (dx0 + fy * (dx1 - dx0)) / m.cell, gy = (dy0 + fx * (dy1 - dy0)) / m.cell;
    const double s = sqrt((gx * gx + gy * gy) + 1.0);
    n[0] = -gx / s; n[1] = -gy / s; n[2] = 1.0 / s;
}

struct TerrainSampleArgs {
    TerrainMap map;
    const double* xy;        // [M][2]
    double* z;               // [M]
    double* normal;          // [M][3] or null
    long long M;
};

struct TerrainInputsArgs {
    TerrainMap map;
    const double* feet;      // [B][12]
    double* x_ref;           // [B][N][13]  in/out: column 5 gains the mean height of the robot's four contact points
    double* normals;         // [B][N][12]  out: S(contact i's xy).n, repeated over the steps (the layout of srbdqp_set_contact_normals)
    int32_t N;
    long long B;
};

constexpr int kTerrainTile = 32;   // robots per workgroup pass of srbdqp_terrain_inputs_kernel

// the launches on st (srbdqp_wrench_lat_ew.hip)
hipError_t launch_terrain_sample(const TerrainSampleArgs& a, hipStream_t st);
hipError_t launch_terrain_inputs(const TerrainInputsArgs& a, hipStream_t st);

// One point per lane, grid-stride: lane l of a wave reads its two coordinates from the wave's 1 KB of xy (every byte of every line it touches is used), the four
// heights of its cell as two pairs of neighbouring doubles through L2 (a map is read-mostly and small beside the points), and writes z -- 512 contiguous bytes a
// wave -- and the normal's three doubles (the wave's 1.5 KB, contiguous).
template <int BT>
__global__ __launch_bounds__(BT) void srbdqp_terrain_sample_kernel(TerrainSampleArgs a) {
    const long long stride = (long long)gridDim.x * BT;
    for (long long p = (long long)blockIdx.x * BT + threadIdx.x; p < a.M; p += stride) {
        double z, n[3];
        terrain_sample(a.map, a.xy[2 * p], a.xy[2 * p + 1], z, n);
        a.z[p] = z;
        if (a.normal) { a.normal[3 * p] = n[0]; a.normal[3 * p + 1] = n[1]; a.normal[3 * p + 2] = n[2]; }
    }
}

// A workgroup takes tiles of R consecutive robots, as srbdqp_mpc_inputs_kernel does: their footholds (12 doubles each) are staged in LDS with coalesced loads, one
// thread per contact point samples the map into the tile's 12 R normals, one per robot sums the four heights, and the tile's rows of both outputs -- contiguous
// in memory -- leave element by element, 512 contiguous bytes per store instruction of a wave: the normals N times over, x_ref read and written back whole with
// the mean height added to column 5.  The horizon is a.N, at run time.
template <int R>
__global__ __launch_bounds__(256) void srbdqp_terrain_inputs_kernel(TerrainInputsArgs a) {
#pragma clang fp contract(off)
    static_assert(4 * R <= 128 && R <= 128, "one thread per contact point in the lower half of the workgroup, one per robot in the upper");
    const int N = a.N;
    __shared__ double sft[R * 12], sn[R * 12], szg[R];
    const int t = threadIdx.x;
    const long long tiles = (a.B + R - 1) / R;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long b0 = tile * R;
        const int nr = (int)((a.B - b0 < R) ? (a.B - b0) : R);
        for (int i = t; i < nr * 12; i += 256) sft[i] = a.feet[b0 * 12 + i];
        __syncthreads();
        if (t < nr * 4) {                                                // contact point t of the tile: its normal (a swing contact's too)
            double z, n[3];
            terrain_sample(a.map, sft[3 * t], sft[3 * t + 1], z, n);
            sn[3 * t] = n[0]; sn[3 * t + 1] = n[1]; sn[3 * t + 2] = n[2];
        }
        if (t >= 128 && t - 128 < nr) {                                  // (another wave) the mean of the four heights AS HANDED IN
            const double* f = sft + 12 * (t - 128);
            szg[t - 128] = (((f[2] + f[5]) + f[8]) + f[11]) * 0.25;
        }
        __syncthreads();
        double* cn = a.normals + b0 * ((long long)N * 12);
        for (int e = t; e < nr * N * 12; e += 256) {                     // normals[r][k][c]
            const int row = e / 12, c = e - 12 * row, r = row / N;
            cn[e] = sn[12 * r + c];
        }
        double* xr = a.x_ref + b0 * ((long long)N * 13);
        for (int e = t; e < nr * N * 13; e += 256) {                     // x_ref[r][k][c]
            const int row = e / 13, c = e - 13 * row, r = row / N;
            const double v = xr[e];
            xr[e] = (c == 5) ? v + szg[r] : v;
        }
        __syncthreads();
    }
}

// The same between srbdqp_mpc_inputs_previewed_* and the solve: the footholds differ from step to step, so every (robot, step, contact)
// is sampled under its own point.  A previewed point gets z = S(own xy).z, the plant's touchdown rule; the height reference of step k follows the four heights
// of foot[b][k] after that write.
struct TerrainPreviewArgs {
    TerrainMap map;
    double* foot;            // [B][N][12]  in/out: the z of a previewed point
    const uint8_t* previewed;// [B][N][4] or null (none previewed)
    double* x_ref;           // [B][N][13]  in/out: column 5 of step k gains the mean height of foot[b][k]
    double* normals;         // [B][N][12]  out
    int32_t N;
    long long B;
};

hipError_t launch_terrain_inputs_previewed(const TerrainPreviewArgs& a, hipStream_t st);

// The tiling of srbdqp_terrain_inputs_kernel.  One thread per (robot, step, contact) reads its point -- a wave's 64 points are 1.5 KB of contiguous foot --,
// samples the map, writes the normal (the wave's 1.5 KB, contiguous) and, where the point is previewed, its height; the four heights of a step wait in LDS
// (24 KB at N = 24) for the x_ref loop, which adds their mean to column 5 in the order (((z0 + z1) + z2) + z3) 0.25.  a.N <= 24.
template <int R>
__global__ __launch_bounds__(256) void srbdqp_terrain_inputs_previewed_kernel(TerrainPreviewArgs a) {
#pragma clang fp contract(off)
    constexpr int NMAX = 24;
    const int N = a.N;
    __shared__ double sz[R * NMAX * 4];
    const int t = threadIdx.x;
    const long long tiles = (a.B + R - 1) / R;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long b0 = tile * R;
        const int nr = (int)((a.B - b0 < R) ? (a.B - b0) : R);
        const long long p0 = b0 * ((long long)N * 4);                    // the tile's first point
        for (int e = t; e < nr * N * 4; e += 256) {                      // point e of the tile: contact e & 3 of row e >> 2
            double* f = a.foot + (p0 + e) * 3;
            double z, n[3];
            terrain_sample(a.map, f[0], f[1], z, n);
            double* cn = a.normals + (p0 + e) * 3;
            cn[0] = n[0]; cn[1] = n[1]; cn[2] = n[2];
            if (a.previewed && a.previewed[p0 + e]) { f[2] = z; sz[e] = z; }
            else sz[e] = f[2];
        }
        __syncthreads();
        double* xr = a.x_ref + b0 * ((long long)N * 13);
        for (int e = t; e < nr * N * 13; e += 256) {                     // x_ref[r][k][c]
            const int row = e / 13, c = e - 13 * row;
            if (c == 5) { const double* z = sz + 4 * row; xr[e] = xr[e] + (((z[0] + z[1]) + z[2]) + z[3]) * 0.25; }
        }
        __syncthreads();
    }
}

}  // namespace srbdqp
